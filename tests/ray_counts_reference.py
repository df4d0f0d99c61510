"""The off-menu ray counts: which nominal counts the suite holds the environment kernels to besides 12 / 16 / 32, what each of them
reaches in the code, the fixtures recorded from the reference at those counts (tests/golden/make_golden.py rays), the harvested
oracle states the GPU tests step, and the comparisons both dtypes must pass.  numpy and the CPU oracle only: the host tests and the
GPU tests share it.

Car(num_rays=n) builds one ray per angle of range(0, 360, 360 // n) (car_env.py:269) and checks collisions on the rays
range(0, n, n // 4) (car_env.py:389): R rays are measured and observed, nc of them decide a crash or a gate."""
import functools
import os

import numpy as np

from conftest import GOLDEN, TRACKS      # (puts the repository root on sys.path)

import oracle

STATE = ("px", "py", "vx", "vy", "rot", "time_step", "next_gate", "passed")
OBS_TOL_F32 = 1.2e-7    # one float32 ulp just below 1.0 (tests/test_env_gpu.py)
MARGIN_PX = 1e-9        # only below this margin may a threshold test fall on the other side than the reference's
REWARD_SCALING = 0.1
RPL_MENU = (1, 2, 3, 5, 6, 9, 12, 17, 33)     # ray slots per lane K1 is instantiated for (float64 handles: up to 17)

#        n  step   R    D  collision rays             track        what it reaches
TABLE = [(4, 90, 4, 10, (0, 1, 2, 3), "track"),                    # the minimum; every ray a collision ray
         (5, 72, 5, 11, (0, 1, 2, 3, 4), "track"),                 # R not a power of two; lanes without a ray
         (7, 51, 8, 14, (0, 1, 2, 3, 4, 5, 6), "big_track"),       # R > n; nc = 7
         (11, 32, 12, 18, (0, 2, 4, 6, 8, 10), "track"),           # R and D of n = 12, other angles, nc = 6
         (31, 11, 33, 39, (0, 7, 14, 21, 28), "big_track"),        # the rays of n = 32, other collision rays
         (90, 4, 90, 96, (0, 22, 44, 66, 88), "big_track"),        # R > 64; collision rays past the 64-bit mask
         (181, 1, 360, 366, (0, 45, 90, 135, 180), "track")]       # the maximum R; reversing into a wall
for _n, _step, _R, _D, _col, _track in TABLE:
    assert _step == 360 // _n and _R == len(range(0, 360, _step)) and _D == 6 + _R, _n
    assert _col == tuple(range(0, _n, _n // 4)), _n
CASES = [(t[5], t[0]) for t in TABLE]                    # (track, n), as ENV_CONFIGS
CASE_IDS = [f"{t}-n{n}" for t, n in CASES]
TRACK_OF = {n: t for t, n in CASES}


def geometry(n):
    """-> step in degrees, R, collision rays"""
    step = 360 // n
    return step, len(range(0, 360, step)), list(range(0, n, n // 4))


def fixture_path(track, n):
    return os.path.join(GOLDEN, f"rays_{track}_n{n}.npz")


@functools.lru_cache(maxsize=None)
def load(track, n):
    """The fixture of one case as a dict of arrays [T, N] (make_golden.py's run_group records).  ret_obs is not stored: the vector
    env hands back the reset observation where the step ended the episode and the step's own observation elsewhere."""
    with np.load(fixture_path(track, n)) as z:
        g = {k: z[k] for k in z.files}
    done = g["terminated"] | g["truncated"]
    g["ret_obs"] = np.where(done[..., None], g["reset_obs"], g["step_obs"])
    return g


def flat(g):
    """a fixture with its [T, N] arrays as rows [T * N]"""
    T, N = g["action"].shape
    keep = ("reset_obs", "reset_state", "walls", "gates", "num_rays_nominal", "reward_scaling")
    return {k: (v if k in keep else v.reshape((T * N,) + v.shape[2:])) for k, v in g.items()}


def collision_ray_distances(segs, px, py, rot, n):
    """[rows, nc] float64: what Car.check_collision's rays read against `segs` from each pose"""
    step, _, col = geometry(n)
    return np.array([[oracle.ray_distance(float(x), float(y), float(r) + float(c * step), segs) for c in col]
                     for x, y, r in zip(px, py, rot)], np.float64).reshape(len(px), len(col))


def high_ray_only_crashes(g, track, n):
    """bool per row of a flat record: the step crashed and every collision ray below 10 px has an index of 64 or more"""
    _, _, col = geometry(n)
    walls = oracle.Track(TRACKS[track]).walls
    out = np.zeros(len(g["action"]), bool)
    idx = np.flatnonzero(g["terminated"])
    if len(idx):
        d = collision_ray_distances(walls, g["post_px"][idx], g["post_py"][idx], g["post_rot"][idx], n)
        low = (d < 10.0) & (np.array(col) < 64)[None, :]
        out[idx] = (d < 10.0).any(1) & ~low.any(1)
    return out


def biased_actions(rng, T, N):
    """random actions, forward-biased so that episodes reach gates and last longer than pure noise (tests/test_env_gpu.py)"""
    a = rng.integers(0, 9, size=(T, N))
    fwd = rng.random((T, N)) < 0.35
    a[fwd] = rng.choice([0, 4, 5], size=int(fwd.sum()))
    return a.astype(np.int64)


def oracle_step_rows(track, n, pre, action, margins=True):
    """One CarEnv.step of the oracle from each pre-state: a flat record with the fixtures' keys."""
    tr = oracle.Track(TRACKS[track])
    M = len(action)
    env = oracle.OracleVecEnv(tr, M, num_rays=n, threads=8)
    reset_obs = oracle.OracleVecEnv(tr, 1, num_rays=n).reset()[0]
    env.set_state(destroyed=0, **{k: pre[k] for k in STATE})
    obs, rew, term, trunc = env.raw_step(action)
    g = {f"pre_{k}": np.array(pre[k]) for k in STATE}
    g.update({f"post_{k}": getattr(env, k).copy() for k in STATE})
    g.update(action=np.asarray(action, np.int64), step_obs=obs, reward=rew, reward_scaled=rew * REWARD_SCALING, terminated=term,
             truncated=trunc, reset_obs=reset_obs, reward_scaling=np.float64(REWARD_SCALING),
             reset_state=np.array([tr.start_x, tr.start_y, 0.0, 0.0, tr.start_rot]))
    g["ret_obs"] = np.where((term | trunc)[:, None], reset_obs, obs)
    if margins:     # as run_group records them: the next gate from the pre-step pose, the walls from the post-step pose
        gate = np.array([tr.gates[k] for k in g["pre_next_gate"]])
        gd = np.array([collision_ray_distances(gate[i], g["pre_px"][i:i + 1], g["pre_py"][i:i + 1], g["pre_rot"][i:i + 1], n)[0]
                       for i in range(M)])
        wd = collision_ray_distances(tr.walls, g["post_px"], g["post_py"], g["post_rot"], n)
        g["gate_margin"] = np.abs(gd - 10.0).min(1)
        g["wall_margin"] = np.abs(wd - 10.0).min(1)
    return g


def free_run_states(track, n, seed):
    """The oracle free-running from reset under biased random actions: every pre-state and its action, rows [T * N]."""
    N, T = (300, 100) if geometry(n)[1] >= 90 else (600, 150)
    actions = biased_actions(np.random.default_rng(seed), T, N)
    env = oracle.OracleVecEnv(oracle.Track(TRACKS[track]), N, num_rays=n, reward_scaling=REWARD_SCALING, threads=8)
    env.reset()
    pre = {k: np.zeros((T, N), getattr(env, k).dtype) for k in STATE}
    for t in range(T):
        for k in STATE:
            pre[k][t] = getattr(env, k)
        env.step(actions[t])
    return {k: v.reshape(-1) for k, v in pre.items()}, actions.reshape(-1)


@functools.lru_cache(maxsize=None)
def harvest(track, n, rows=2048, seed=0):
    """At most `rows` oracle pre-states with their actions and the oracle's outcome: a flat record with the fixtures' keys, plus
    `differs_at_32` (n = 31) and `n_high_ray_only`.  In this order:
      - n = 181: the fixture's crashes through rays 64 and up alone (`n_high_ray_only` rows, first of all);
      - n = 31: the rows on which 31 and 32 nominal rays disagree, at most rows / 2;
      - n = 90 and 181: the free run's own crashes through rays 64 and up alone, at most rows / 4;
      - 64 rows one step before the time limit;
      - rows with a crash, a gate or a lap: a random choice of them, since the free run holds more than fit -- all but 256 of the
        rows that are left;
      - random rows for the rest, so that steps on which nothing happens are compared too."""
    rng = np.random.default_rng(1000 + seed)
    pre, action = free_run_states(track, n, seed)
    all_rows = oracle_step_rows(track, n, pre, action, margins=False)
    M = len(action)
    picked, differs = [], np.zeros(M, bool)
    if n == 31:
        at32 = oracle_step_rows(track, 32, pre, action, margins=False)
        differs = (at32["terminated"] != all_rows["terminated"]) | (at32["reward"] != all_rows["reward"])
        picked += list(rng.permutation(np.flatnonzero(differs))[:rows // 2])
    if max(geometry(n)[2]) >= 64:      # the free run's own crashes through rays 64 and up alone: first
        picked += list(np.flatnonzero(high_ray_only_crashes(all_rows, track, n))[:rows // 4])
    extra = None
    if n == 181:
        f = flat(load(track, n))
        hi = np.flatnonzero(high_ray_only_crashes(f, track, n))
        extra = ({k: f[f"pre_{k}"][hi] for k in STATE}, f["action"][hi])
    taken = set(picked)
    near_limit = [i for i in rng.permutation(M) if i not in taken][:64]
    taken.update(near_limit)
    event = all_rows["terminated"] | all_rows["truncated"] | (all_rows["reward"] > 0.5)
    budget = rows - len(picked) - 64 - (0 if extra is None else len(extra[1]))
    # (the free run holds more events than fit: a random choice of them, and 256 rows kept for steps on which nothing happens)
    events = [i for i in rng.permutation(np.flatnonzero(event)) if i not in taken][:budget - 256]
    taken.update(events)
    rest = [i for i in rng.permutation(M) if i not in taken][:budget - len(events)]
    order = np.array(picked + near_limit + events + rest, np.int64)
    sel = {k: v[order].copy() for k, v in pre.items()}
    lo = len(picked)
    sel["time_step"][lo:lo + 64] = 999
    act = action[order]
    if extra is not None:
        sel = {k: np.concatenate([extra[0][k], sel[k]]) for k in STATE}
        act = np.concatenate([extra[1], act])
    g = oracle_step_rows(track, n, sel, act)
    g["differs_at_32"] = np.concatenate([np.zeros(0 if extra is None else len(extra[1]), bool), differs[order]])
    g["n_high_ray_only"] = 0 if extra is None else len(extra[1])
    return g


# --------------------------------------------------------------------------------------------------------------------------------
# the comparisons (tests/test_env_gpu.py: test_teacher_forced_f64_bit_exact, test_teacher_forced_f32), on flat records
# --------------------------------------------------------------------------------------------------------------------------------
def assert_step_f64(out, st, g):
    """out = (obs, rew, term, trunc, final_obs, gates_passed) of one teacher-forced step, st = the state after it"""
    obs, rew, term, trunc, fin, gp = out
    done = g["terminated"] | g["truncated"]
    assert np.array_equal(fin, g["step_obs"])
    assert np.array_equal(obs, g["ret_obs"])
    assert np.array_equal(rew, g["reward_scaled"].astype(np.float32))
    assert np.array_equal(term, g["terminated"])
    assert np.array_equal(trunc, g["truncated"])
    assert np.array_equal(gp, g["post_passed"])
    for k in STATE:
        assert np.array_equal(st[k][~done], g[f"post_{k}"][~done]), k
    assert np.all(st["time_step"][done] == 0) and np.all(st["px"][done] == g["reset_state"][0])
    assert np.all(st["rot"][done] == g["reset_state"][4]) and np.all(st["vx"][done] == 0)


def assert_step_f32(out, st, g):
    """-> (the worst observation error, the rows inside a threshold margin)"""
    obs, rew, term, trunc, fin, gp = out
    worst = float(np.abs(fin - g["step_obs"]).max())
    assert worst <= OBS_TOL_F32, worst
    hdr, ref_hdr = fin[:, :6], g["step_obs"][:, :6]
    diff = np.abs(hdr - ref_hdr)
    assert (diff <= np.spacing(np.maximum(np.abs(ref_hdr), np.float32(1e-6)))).all() and (diff != 0).mean() < 1e-3, \
        (diff.max(), (diff != 0).mean())
    wall_ok = g["wall_margin"] > MARGIN_PX
    gate_ok = g["gate_margin"] > MARGIN_PX
    term_ref, trunc_ref = g["terminated"], g["truncated"]
    assert np.array_equal(term[wall_ok], term_ref[wall_ok])
    assert np.array_equal(trunc[wall_ok], trunc_ref[wall_ok])
    assert np.array_equal(gp[gate_ok], g["post_passed"][gate_ok])
    both = wall_ok & gate_ok
    assert both.mean() > 0.99
    assert np.array_equal(rew[both], g["reward_scaled"].astype(np.float32)[both])
    same = (term == term_ref) & (trunc == trunc_ref)
    assert np.abs(obs - g["ret_obs"])[same].max() <= OBS_TOL_F32
    live = both & ~(term_ref | trunc_ref)
    assert np.array_equal(st["next_gate"][live], g["post_next_gate"][live])
    assert np.array_equal(st["time_step"][live], g["post_time_step"][live])
    assert np.array_equal(st["rot"][live], g["post_rot"][live]) or np.abs(st["rot"][live] - g["post_rot"][live]).max() < 1e-9
    for k in ("px", "py", "vx", "vy"):
        assert np.abs(st[k][live] - g[f"post_{k}"][live]).max() < 1e-12, k
    return worst, int((~both).sum())
