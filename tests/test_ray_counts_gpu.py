"""The per-step kernel K1 at the off-menu ray counts of tests/ray_counts_reference.py (4, 5, 7, 11, 31, 90, 181 nominal rays): against the
fixtures recorded from the reference and against harvested oracle states, in both dtypes, in every lane geometry, on mixed tracks.

Bars, as in tests/test_env_gpu.py: float64 handles bit-exact in everything; float32 handles within OBS_TOL_F32 = 1.2e-7 of the
reference's observations, events equal wherever the reference's own threshold margin exceeds 1e-9 px, at least 99 % of the rows
outside those margins."""
import numpy as np
import pytest
import torch

import oracle
import ppo_car_amd as pc
import ray_counts_reference as rc
from conftest import TRACKS
from ray_counts_reference import CASE_IDS, CASES, OBS_TOL_F32, STATE

pytestmark = pytest.mark.gpu

cases = pytest.mark.parametrize("track,n", CASES, ids=CASE_IDS)
dtypes = pytest.mark.parametrize("dtype", ["f64", "f32"])
FORMS = [1, 2]      # PC_OPT_STEP_FORM: K1, and K1f where the shape has it -- none of these counts has: K1 again
SOURCES = {"fixture": lambda track, n: rc.flat(rc.load(track, n)), "harvest": rc.harvest}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


GUARD = -7.5     # the row after the last env's in the observation buffers handed to a step: a store from a ray slot past R would land there


def _step(env, actions):
    N, D = env.num_envs, env.obs_dim
    obs_g, fin_g = (torch.full((N + 1, D), GUARD, device="cuda") for _ in range(2))
    gp = torch.empty(N, dtype=torch.int32, device="cuda")
    out = (obs_g[:N], torch.empty(N, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda"))
    obs, rew, term, trunc, _ = env.step(_cuda(actions), out=out, final_obs=fin_g[:N], gates_passed=gp)
    torch.cuda.synchronize()
    assert bool((obs_g[N] == GUARD).all()) and bool((fin_g[N] == GUARD).all())      # nothing written past the rows
    c = lambda t: t.cpu().numpy()
    return c(obs), c(rew), c(term) != 0, c(trunc) != 0, c(fin_g[:N]), c(gp)


def _forced(track, n, dtype, g, lanes=None, form=None, tracks=None, track_id=None):
    """One teacher-forced step of the rows of g -> (outputs, state after, the handle); None where the handle refuses `lanes`"""
    M = len(g["action"])
    env = pc.VecCarEnv(M, tracks or TRACKS[track], num_rays=n, reward_scaling=float(g["reward_scaling"]), dtype=dtype, track_id=track_id)
    if lanes is not None:
        try:
            env.set_lanes_per_env(lanes)
        except pc.PpoCarError:      # a geometry the handle refuses: nothing to step
            env.close()
            return None
    if form is not None:
        env.set_option("step_form", form)
    env.reset()
    env.set_state(**{k: g[f"pre_{k}"] for k in STATE})
    out = _step(env, g["action"])
    return out, env.get_state(), env


def _check(dtype, out, st, g, what):
    if dtype == "f64":
        rc.assert_step_f64(out, st, g)
    else:
        worst, near = rc.assert_step_f32(out, st, g)
        print(f"{what}: float32 observations within {worst:.3g} of the reference's, {near} of {len(g['action'])} rows inside a threshold margin")


# ------------------------------------------------------------------------------------------------
# teacher-forced: the reference's recorded transitions and the harvested oracle states
# ------------------------------------------------------------------------------------------------
@cases
@dtypes
@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("form", FORMS)
def test_teacher_forced(track, n, dtype, source, form):
    g = SOURCES[source](track, n)
    out, st, env = _forced(track, n, dtype, g, form=form)
    assert env.last_step_kernel() == "K1"          # n = 11 and n = 31 too: the table-driven kernel is for 12 / 16 / 32 nominal rays
    assert env.obs_dim == 6 + rc.geometry(n)[1]
    _check(dtype, out, st, g, f"{track} n={n} {source} form {form}")
    env.close()


@cases
@dtypes
def test_step_many_equals_three_steps(track, n, dtype):
    g = rc.harvest(track, n)
    M = len(g["action"])
    acts = np.stack([g["action"], np.roll(g["action"], 1), np.roll(g["action"], 2)])
    res = []
    for many in (False, True):
        env = pc.VecCarEnv(M, TRACKS[track], num_rays=n, reward_scaling=0.1, dtype=dtype)
        env.reset()
        env.set_state(**{k: g[f"pre_{k}"] for k in STATE})
        if many:
            o, r, te, tr = env.step_many(_cuda(acts))
        else:
            rows = [env.step(_cuda(acts[t])) for t in range(3)]
            o, r, te, tr = (torch.stack([row[k].clone() for row in rows]) for k in range(4))
        torch.cuda.synchronize()
        assert env.last_step_kernel() == "K1"
        res.append([x.cpu().numpy() for x in (o, r, te, tr)] + [env.get_state()])
        env.close()
    for a, b in zip(res[0][:4], res[1][:4]):
        assert np.array_equal(a, b)
    for k in STATE:
        assert np.array_equal(res[0][4][k], res[1][4][k]), k
    assert res[0][2].sum() > 100           # crashes among them


# ------------------------------------------------------------------------------------------------
# free-running from reset against the oracle
# ------------------------------------------------------------------------------------------------
def _free_run(env, actions):
    T, N = actions.shape
    acts = _cuda(actions)
    o = torch.empty(T, N, env.obs_dim, device="cuda")
    r, te, tr = (torch.empty(T, N, device="cuda") for _ in range(3))
    env.reset()
    for t in range(T):
        env.step(acts[t], out=(o[t], r[t], te[t], tr[t]))
    torch.cuda.synchronize()
    assert env.last_step_kernel() == "K1"
    return o.cpu().numpy(), r.cpu().numpy(), te.cpu().numpy() != 0, tr.cpu().numpy() != 0


def _oracle_run(track, n, actions):
    T, N = actions.shape
    ora = oracle.OracleVecEnv(oracle.Track(TRACKS[track]), N, num_rays=n, reward_scaling=0.1, threads=8)
    ora.reset()
    O, R = np.zeros((T, N, ora.D), np.float32), np.zeros((T, N), np.float64)
    TE, TR = np.zeros((T, N), bool), np.zeros((T, N), bool)
    for t in range(T):
        O[t], R[t], TE[t], TR[t] = ora.step(actions[t])
    return O, R.astype(np.float32), TE, TR, ora


@cases
@dtypes
def test_free_running_vs_oracle(track, n, dtype):
    T, N = 64, 300
    actions = rc.biased_actions(np.random.default_rng(40 + n), T, N)
    O, R, TE, TR, ora = _oracle_run(track, n, actions)
    assert TE.sum() >= 100
    env = pc.VecCarEnv(N, TRACKS[track], num_rays=n, reward_scaling=0.1, dtype=dtype)
    o, r, te, tr = _free_run(env, actions)
    if dtype == "f64":
        assert np.array_equal(te, TE) and np.array_equal(tr, TR)
        assert np.array_equal(r, R)
        assert np.array_equal(o, O)
        st = env.get_state()
        for k in STATE:
            assert np.array_equal(st[k], getattr(ora, k).astype(st[k].dtype)), k
    else:
        # a float32 trajectory may leave the float64 one after a flipped near-tie (test_full_size_f64_vs_oracle_and_replication): until
        # an env's first event mismatch its observations and rewards are held to the bars, and at least 99 % of the envs never have one
        mism = (te != TE) | (tr != TR)
        first_bad = np.where(mism.any(0), mism.argmax(0), T)
        ok = np.arange(T)[:, None] < first_bad[None, :]
        assert (first_bad == T).mean() >= 0.99, (first_bad == T).mean()
        assert np.abs(o - O)[ok].max() <= OBS_TOL_F32
        assert np.array_equal(r[ok], R[ok])
    env.close()


# ------------------------------------------------------------------------------------------------
# every lane geometry against the oracle; the instances the seven counts visit
# ------------------------------------------------------------------------------------------------
LANES = (1, 2, 4, 8, 16, 32, 64)


@cases
@dtypes
def test_every_lane_geometry_against_the_oracle(track, n, dtype):
    g = rc.harvest(track, n)
    R = rc.geometry(n)[1]
    seen = []
    for lanes in LANES:
        res = _forced(track, n, dtype, g, lanes=lanes)
        if res is None:
            continue
        out, st, env = res
        info = env.launch_info()
        G, rpl = info["lanes_per_env"], info["rays_per_lane"]
        assert G >= lanes and G * rpl >= R and rpl in rc.RPL_MENU and (dtype == "f32" or rpl <= 17)
        if (G, rpl) not in seen:           # (too few lanes for the menu are doubled by the handle: the same geometry again)
            _check(dtype, out, st, g, f"{track} n={n} {G} lanes x {rpl} slots")
            seen.append((G, rpl))
        env.close()
    assert seen == _geometries(n, dtype, len(g["action"]))
    print(f"{track} n={n} {dtype}: (lanes, slots) {seen}")


def _geometries(n, dtype, N=2048):
    """The (lanes per env, ray slots per lane) a handle of N envs takes when asked for 1, 2, 4 ... 64 lanes, without repeats: what
    test_every_lane_geometry_against_the_oracle steps and compares (it asserts this very list)."""
    seen = []
    env = pc.VecCarEnv(N, TRACKS[rc.TRACK_OF[n]], num_rays=n, dtype=dtype)
    for lanes in LANES:
        try:
            env.set_lanes_per_env(lanes)
        except pc.PpoCarError:
            continue
        info = env.launch_info()
        if (info["lanes_per_env"], info["rays_per_lane"]) not in seen:
            seen.append((info["lanes_per_env"], info["rays_per_lane"]))
    env.close()
    return seen


def test_the_seven_counts_visit_every_instance_of_the_menu():
    """Over the seven counts the geometry test above runs every instance of K1: float32 handles every slot count of the menu, float64
    handles all but 33; and the geometries with padded slots and ray-less lanes are among them."""
    visited = {(dtype, n): _geometries(n, dtype) for dtype in ("f64", "f32") for _, n in CASES}
    slots = lambda dtype: {rpl for (d, _), seen in visited.items() if d == dtype for _, rpl in seen}
    print("float32 slot counts visited:", sorted(slots("f32")), "float64:", sorted(slots("f64")))
    assert slots("f32") == set(rc.RPL_MENU)
    assert slots("f64") == set(rc.RPL_MENU) - {33}
    for dtype in ("f64", "f32"):
        assert (8, 1) in visited[(dtype, 5)]          # R = 5 on 8 lanes: three lanes of every env own no ray
        assert (1, 9) in visited[(dtype, 7)]          # R = 8 on one lane: 9 slots, the last one masked
        assert (64, 6) in visited[(dtype, 181)]       # R = 360 on 64 lanes: 384 slots
    assert (4, 33) in visited[("f32", 90)]            # R = 90 on 4 lanes: 132 slots


# ------------------------------------------------------------------------------------------------
# mixed tracks, interleaved i & 1 (the MIXED instances)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 31])
@dtypes
def test_interleaved_tracks_equal_the_single_track_runs(n, dtype):
    """track and big_track in one handle, env i on track i & 1, 300 envs x 64 steps from reset: each env must equal the single-track
    run of its own track bit for bit, in every geometry the mixed handle takes (at most 17 slots per lane); the float64 single-track
    runs are the oracle's, every bit."""
    T, N = 64, 300
    actions = rc.biased_actions(np.random.default_rng(70 + n), T, N)
    names = ("track", "big_track")
    singles = {}
    for k, name in enumerate(names):
        env = pc.VecCarEnv(N, TRACKS[name], num_rays=n, reward_scaling=0.1, dtype=dtype)
        singles[k] = _free_run(env, actions) + (env.get_state(),)
        env.close()
        if dtype == "f64":
            ref = _oracle_run(name, n, actions)[:4]
            assert ref[2].sum() >= 50
            for a, b in zip(singles[k][:4], ref):
                assert np.array_equal(a, b), name
    tid = (np.arange(N) & 1).astype(np.uint8)
    seen = set()
    for lanes in (0, 1, 2, 4, 8, 16, 32):
        env = pc.VecCarEnv(N, [TRACKS[x] for x in names], num_rays=n, reward_scaling=0.1, dtype=dtype, track_id=tid)
        if lanes:
            env.set_lanes_per_env(lanes)
        rpl = env.launch_info()["rays_per_lane"]
        assert rpl <= 17
        if lanes and rpl in seen:
            env.close()
            continue
        seen.add(rpl)
        out = _free_run(env, actions)
        st = env.get_state()
        for k in (0, 1):
            m = tid == k
            for a, b in zip(out, singles[k][:4]):
                assert np.array_equal(a[:, m], b[:, m]), (lanes, k)
            for key in STATE:
                assert np.array_equal(st[key][m], singles[k][4][key][m]), (lanes, k, key)
        env.close()
    assert seen == ({1, 2, 5, 9} if n == 7 else {1, 2, 3, 5, 9, 17}), seen      # (R = 8: 9 / 5 / 2 / 1 slots; R = 33: 17 ... 1)


# ------------------------------------------------------------------------------------------------
# the persistent rollout at the look-alike counts: 11 (R and D of 12) and 31 (the rays of 32)
# ------------------------------------------------------------------------------------------------
# The fast and literal forms of pc_rollout carry four collision rays and the angles of 12 / 16 / 32 nominal rays as constants: 11 and 31
# nominal rays must take a generic form -- which reads both from the handle -- or be refused.  pc_env_last_rollout_kernel names the
# literal forms of float64 handles; for float32 handles "K9" / "K9s" cover the fast and the generic mode alike, so there the proof is
# the bits: the per-step kernel K1 (held to the oracle above) and the oracle's own replay, which a kernel that takes 11 for 12 or 31
# for 32 cannot pass (tests/test_ray_counts_host.py: the rows on which 31 and 32 disagree).
GENERIC_KERNELS = {"f32": ("K9", "K9s"), "f64": ("K9d-selector", "K9d-filter")}


@pytest.mark.parametrize("n_envs", [1000, 20000])
@dtypes
@pytest.mark.parametrize("n", [11, 31])
def test_persistent_rollout_at_the_look_alike_counts(n, dtype, n_envs):
    from ppo_car_amd.ppo import PPOConfig, Trainer
    from test_rollout_baseline_gpu import _oracle_replay_check, _snap, strided_population
    track = TRACKS[rc.TRACK_OF[n]]
    D = 6 + rc.geometry(n)[1]
    # (float64 handles: what these counts can take is the generic kernel K9d, a big-form kernel with the unsplit policy arithmetic at any
    # batch size -- the per-step path is given the same summation order, as in tests/test_rollout_f64_gpu.py)
    split = 0 if dtype == "f64" else -1
    res, first = {}, None
    for mode in ("steps", "mega"):
        cfg = PPOConfig(n_envs=n_envs, n_steps=64, num_rays=n, track=track, rollout_kernel=mode, use_graphs=False, seed=5, env_dtype=dtype,
                        policy_split=split)
        tr = Trainer(cfg, device="cuda")
        if first is None:
            first = tr.next_obs.clone()
        for _ in range(2):
            tr.rollout()
            tr.buffer.ptr = 0
        torch.cuda.synchronize()
        assert tr.obs_dim == (D,)
        res[mode] = _snap(tr)
        res[mode + "_state"] = tr.envs.get_state()
        res[mode + "_ran"] = (tr.rollout_mode, tr.envs.last_rollout_kernel(), tr.envs.last_step_kernel())
        tr.close()
    assert res["steps_ran"] == ("steps-eager", "none", "K1")
    accepted = res["mega_ran"][0] == "mega"
    print(f"pc_rollout at {n} nominal rays, {n_envs} envs, {dtype}: "
          + (f"accepted, kernel {res['mega_ran'][1]}" if accepted else "PC_ERR_UNSUPPORTED, the per-step kernels ran"))
    if accepted:
        assert res["mega_ran"][1] in GENERIC_KERNELS[dtype], res["mega_ran"]
    else:       # (any answer of pc_rollout but PC_ERR_UNSUPPORTED raises in Trainer.rollout)
        assert res["mega_ran"] == ("steps-eager", "none", "K1")
    if n == 11:
        assert accepted      # R = 12, D = 18 on two or four lanes: the generic forms are built for these slots
    for i, (a, b) in enumerate(zip(res["steps"], res["mega"])):
        assert torch.equal(a, b), i
    for k in res["mega_state"]:
        assert np.array_equal(res["mega_state"][k], res["steps_state"][k]), k
    assert float(res["mega"][5].sum()) > 0
    # 200 steps from reset replayed on the oracle: the persistent launch where the shape has one, else what the automatic mode runs
    cfg = PPOConfig(n_envs=n_envs, n_steps=200, num_rays=n, track=track, rollout_kernel="mega" if accepted else "auto", use_graphs=False,
                    seed=5, env_dtype=dtype, policy_split=split)
    tr = Trainer(cfg, device="cuda")
    tr.rollout()
    torch.cuda.synchronize()
    assert tr.rollout_mode == ("mega" if accepted else "steps-eager")
    if not accepted:
        assert tr.envs.last_step_kernel() == "K1" and tr.envs.last_rollout_kernel() == "none"
    _oracle_replay_check(cfg, _snap(tr), first, f"rays={n} N={n_envs} {dtype}", sel=strided_population(n_envs, per_wave=4, limit=256),
                         exact=dtype == "f64")
    tr.close()
