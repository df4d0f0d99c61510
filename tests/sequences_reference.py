"""Plain reference of pc_env_rollout_sequences on the CPU oracle, the inputs the tests score and the host regeneration of the
planner's candidate table.

rollout(): every row replicated K times, one copy per sequence (copy m * K + k); OracleVecEnv.set_state once, raw_step H times; a copy
that terminated or truncated is frozen (what the oracle goes on computing for it is ignored).  Per step and copy the reward is
np.float32(rew * reward_scale) widened and summed in float64, in step order; gates and laps are read off the reward codes of
step_poses_reference."""
import os

import numpy as np

import step_poses_reference as R      # (first: through conftest it puts the repository root on sys.path)
import safe_actions_reference as S
import draw_reference as D

import oracle  # noqa: E402

CONFIGS = R.CONFIGS
REWARD_SCALE = R.REWARD_SCALE
STATE_KEYS = S.STATE_KEYS
RECIPES = ("edge", "near_gate", "pre_crash")
ROWS = {"edge": 300, "near_gate": 240, "pre_crash": 256}
RUNNING, TERMINATED, TRUNCATED = 0, 1, 2
LAP_CODES = (11, 8)      # of step_poses_reference.GATE_CODES: the gate closed a lap (alone / with the -3 of a crash)
OUT_KEYS = ("ret", "steps", "status", "gates", "laps")
BEST_KEYS = ("best_k", "best_action", "best_ret")
_THREADS = max(1, min(16, os.cpu_count() or 1))
K_REF, H_REF = 64, 12
NEAR10_PX = 1e-6

# What the inputs give on the CPU oracle at K = 64, H = 12, per config.  Pooled over the three recipes (796 rows, 50944 pairs):
# pairs that ended terminated / truncated / still running, pairs with a gate fired; pairs with a lap closed on edge + near_gate (540
# rows); rows whose sequences end in mixed statuses, rows whose best sequence is a drawn one (best_k >= 9), rows whose maximum is unique.
COUNT_KEYS = ("terminated", "truncated", "running", "gate", "lap", "mixed_rows", "drawn_best_rows", "unique_max_rows")
# the least the issue asks of them: shares of the pairs (lap: of the edge + near_gate pairs), then row counts
NEED = dict(terminated=0.10, truncated=0.10, running=0.10, gate=0.15, lap=0.05, mixed_rows=50, drawn_best_rows=40, unique_max_rows=40)
COUNTS = {("big_track", 16): dict(terminated=18853, truncated=17825, running=14266, gate=23389, lap=12890, mixed_rows=74, drawn_best_rows=57,
                                  unique_max_rows=82),
          ("track", 12): dict(terminated=19144, truncated=17606, running=14194, gate=23380, lap=13139, mixed_rows=70, drawn_best_rows=57,
                              unique_max_rows=70),
          ("oval64", 16): dict(terminated=18737, truncated=18082, running=14125, gate=25172, lap=13214, mixed_rows=167, drawn_best_rows=57,
                               unique_max_rows=77)}


def table(H, K, seed=5):
    """uint8 [H, K] time-major: default_rng(seed).integers(0, 9, (H, K)) with columns 0 .. 8 overwritten by the constant actions"""
    t = np.random.default_rng(seed).integers(0, 9, (H, K)).astype(np.uint8)
    c = min(K, 9)
    t[:, :c] = np.arange(c, dtype=np.uint8)
    return t


def rollout(name, n, state, actions, reward_scale=REWARD_SCALE):
    """state: dict of px, py, vx, vy, rot (float64), time_step, next_gate (integers), M entries each.  actions: [H, K] shared or
    [M, H, K] per state, values 0 .. 8.  Returns a dict: ret float64, steps, gates, laps int32, status uint8, each [M, K]; best_k int32,
    best_action int64, best_ret float64, each [M]; `state`, the oracle's state of every copy after its last step ([M * K] each); and
    `near10` bool [M, K]: in one of the copy's steps one of check_collision's rays came within NEAR10_PX of the 10 px threshold, as far as
    the float32 observation resolves it (one float32 ulp of 0.01 is 0.93e-6 px) -- where another arithmetic may decide the crash the
    other way."""
    M = len(state["px"])
    actions = np.asarray(actions)
    if actions.ndim == 2:
        actions = np.broadcast_to(actions, (M,) + actions.shape)
    H, K = actions.shape[1:]
    assert actions.min() >= 0 and actions.max() <= 8
    env = oracle.OracleVecEnv(R.track(name), M * K, n, threads=_THREADS)
    env.set_state(passed=0, destroyed=0, **{k: np.repeat(np.asarray(state[k]), K) for k in STATE_KEYS})
    ret = np.zeros(M * K, np.float64)
    steps, gates, laps = (np.zeros(M * K, np.int32) for _ in range(3))
    status = np.zeros(M * K, np.uint8)
    final = {k: getattr(env, k).copy() for k in STATE_KEYS}
    near = np.zeros(M * K, bool)
    rays = 6 + np.arange(0, n, n // 4)
    for t in range(H):
        a = actions[:, t, :].reshape(-1).astype(np.int64)
        obs, rew, term, trunc = env.raw_step(a)
        live = status == RUNNING
        near |= live & (np.abs(obs[:, rays].astype(np.float64) * 1000.0 - 10.0) <= NEAR10_PX + 1e-6).any(1)
        code = np.rint(rew - 0.01 * np.isin(a, (0, 4, 5))).astype(np.int64)
        ret[live] += (rew * reward_scale).astype(np.float32).astype(np.float64)[live]
        steps[live] += 1
        gates[live] += np.isin(code, R.GATE_CODES)[live]
        laps[live] += np.isin(code, LAP_CODES)[live]
        status[live] = np.where(term, TERMINATED, np.where(trunc, TRUNCATED, RUNNING))[live]
        for k in STATE_KEYS:
            final[k][live] = getattr(env, k)[live]
    out = dict(ret=ret.reshape(M, K), steps=steps.reshape(M, K), status=status.reshape(M, K), gates=gates.reshape(M, K),
               laps=laps.reshape(M, K), state=final, near10=near.reshape(M, K))
    out["best_k"] = out["ret"].argmax(1).astype(np.int32)      # the first maximum
    out["best_action"] = actions[np.arange(M), 0, out["best_k"]].astype(np.int64)
    out["best_ret"] = out["ret"][np.arange(M), out["best_k"]]
    return out


_ref = {}


def states(name, n, recipe):
    s = S.RECIPES[recipe](name, n)
    assert len(s["px"]) == ROWS[recipe], (recipe, len(s["px"]))
    return s


def reference(name, n, recipe, H=H_REF, K=K_REF):
    """(state rows, rollout of the shared table(H, K)): computed once per key, never modified"""
    key = (name, n, recipe, H, K)
    if key not in _ref:
        s = states(name, n, recipe)
        _ref[key] = (s, rollout(name, n, s, table(H, K)))
    return _ref[key]


def pooled(name, n):
    """The three recipes' rows in one set: (state rows, names of the recipe of every row)"""
    rows = [states(name, n, r) for r in RECIPES]
    keys = STATE_KEYS + ("turns",)
    return {k: np.concatenate([np.asarray(r[k]) for r in rows]) for k in keys}, np.repeat(RECIPES, [ROWS[r] for r in RECIPES])


def counts(name, n, H=H_REF, K=K_REF):
    """dict over COUNT_KEYS of the references at (H, K), and the number of pairs / lap pairs they are shares of"""
    refs = {r: reference(name, n, r, H, K)[1] for r in RECIPES}
    cat = lambda key, rs=RECIPES: np.concatenate([refs[r][key] for r in rs])
    status, ret = cat("status"), cat("ret")
    c = dict(terminated=int((status == TERMINATED).sum()), truncated=int((status == TRUNCATED).sum()), running=int((status == RUNNING).sum()),
             gate=int((cat("gates") > 0).sum()), lap=int((cat("laps", ("edge", "near_gate")) > 0).sum()),
             mixed_rows=int((status.min(1) != status.max(1)).sum()), drawn_best_rows=int((cat("best_k") >= 9).sum()),
             unique_max_rows=int(((ret == ret.max(1, keepdims=True)).sum(1) == 1).sum()))
    return c, status.size, (ROWS["edge"] + ROWS["near_gate"]) * K


def meets(c, pairs, lap_pairs):
    """the issue's input conditions on one config's counts"""
    for k in COUNT_KEYS:
        base = lap_pairs if k == "lap" else pairs
        need = NEED[k] * base if isinstance(NEED[k], float) else NEED[k]
        assert c[k] >= need, (k, c[k], need)


# ---- the planner's candidate table, regenerated on the host from the documented stream -----------------------------------------------
def planner_draw(H, K, seed, step_index):
    """(uint8 [H, K] table of Planner.candidate_table(step_index), the least margin of its drawn entries): entry (t, k) is element
    t * K + k of pc_sample on all-zero logits [H * K][9] at (seed, offset = step_index); columns 0 .. 8 hold the constant actions.  The
    margin is the distance of an element's uniform to the nearest boundary i / 9 of the CDF: the device forms that CDF in float32, so
    only an element within ~1e-6 of a boundary could be decided the other way there."""
    u = D.uniform(seed, step_index, np.arange(H * K))
    a, _, _, margin = D.draw_f64(np.zeros((H * K, 9)), u)
    t = a.astype(np.uint8).reshape(H, K)
    t[:, :9] = np.arange(9, dtype=np.uint8)
    drawn = np.ones((H, K), bool)
    drawn[:, :9] = False
    return t, float(margin.reshape(H, K)[drawn].min()) if drawn.any() else np.inf
