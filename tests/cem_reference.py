"""Plain numpy reference of the cross-entropy planner's two integer steps (include/ppocar.h: pc_cem_sample, pc_cem_refit), of the
planner's iteration loop with a scoring callback, and the `driven` states the tests plan from.

Weights are uint32 [M, H, 9]; every reader clamps a value to 65536 and takes a row that sums to 0 as nine ones (read_weights).
  sample   element (m, t, k), idx = (m * H + t) * K + k: x = word offset & 3 of draw_reference.philox_words(seed, offset, idx) -- the raw
           word --, r = (x * S) >> 32 with S the row's sum, action = the least a with r < w[0] + .. + w[a]
  refit    the K returns ordered by value descending then k ascending (a stable sort of the negated values: -0.0 == 0.0), the first E
           are the elites; c[t][a] counts their entries (above 8: 8); f = (c << 16) // E; w' = min(65536, max(w_min, w - (w >> s) + (f >> s)))
  plan     iterations x (sample at offset0 + i with the constant columns and, from the second on, the previous best sequence in
           column 9; score; refit)"""
import numpy as np

import step_poses_reference as R      # (first: through conftest it puts the repository root on sys.path)
import safe_actions_reference as S
import sequences_reference as Q
import draw_reference as D

import oracle  # noqa: E402

CONFIGS = Q.CONFIGS
W_MAX = 65536
INIT_WEIGHT = 7281      # 65536 // 9: CEMPlanner's default
H_REF, K_REF, E_REF, ITERATIONS_REF, SEED_REF = 12, 64, 8, 4, 3
DRIVEN_ROWS = 256

# What plan() gives from the driven rows on the CPU oracle at H = 12, K = 64, E = 8, 4 iterations, seed 3, offset0 0, shift 1, w_min 64,
# weights INIT_WEIGHT: rows whose best return is higher after the last iteration than after the first; rows whose best first action
# differs between the two; rows whose last best sequence is one drawn in that iteration (best_k >= 10: not a constant column, not the
# kept one).  The best return of a row never falls from one iteration to the next.
COUNT_KEYS = ("improved", "action_changed", "drawn_best")
NEED = dict(improved=50, action_changed=40, drawn_best=20)
COUNTS = {("big_track", 16): dict(improved=139, action_changed=107, drawn_best=45),
          ("track", 12): dict(improved=111, action_changed=73, drawn_best=55),
          ("oval64", 16): dict(improved=81, action_changed=62, drawn_best=31)}


def read_weights(w):
    """uint64 copy of the weights as both kernels read them"""
    w = np.minimum(np.asarray(w).astype(np.uint64), np.uint64(W_MAX))
    w[w.sum(-1) == 0] = 1
    return w


def sample(w, K, seed, offset, const_columns=True, keep=None, active=None, out=None):
    """uint8 [M, H, K].  keep: uint8 [M, H] or None.  active: [M] or None; rows with 0 keep what `out` (or zeros) holds."""
    w = np.asarray(w)
    M, H, _ = w.shape
    x = D.philox_words(seed, offset, np.arange(M * H * K, dtype=np.uint64))[int(offset) & 3].reshape(M, H, K)
    cum = np.cumsum(read_weights(w), -1)      # [M, H, 9]
    r = (x * cum[:, :, -1:]) >> np.uint64(32)      # x < 2^32 and S < 2^20: exact in uint64
    t = (r[..., None] >= cum[:, :, None, :]).sum(-1).astype(np.uint8)
    assert t.max() <= 8
    if const_columns:
        c = min(K, 9)
        t[:, :, :c] = np.arange(c, dtype=np.uint8)
    if keep is not None and K > 9:
        t[:, :, 9] = keep
    res = np.zeros((M, H, K), np.uint8) if out is None else np.array(out, np.uint8)
    on = np.ones(M, bool) if active is None else np.asarray(active) != 0
    res[on] = t[on]
    return res


def order(ret):
    """[M, K] int64: the sequences by return descending, then k ascending"""
    return np.argsort(-np.asarray(ret, np.float64), axis=1, kind="stable")


def refit(w, ret, table, E, shift, w_min, active=None, best_seq=None):
    """(new weights uint32 [M, H, 9], best_seq uint8 [M, H]); rows with active == 0 keep w and best_seq (or zeros)"""
    w, table = np.asarray(w), np.asarray(table)
    M, H, K = table.shape
    o = order(ret)
    elites = np.minimum(table, 8)[np.arange(M)[:, None, None], np.arange(H)[None, :, None], o[:, None, :E]]      # [M, H, E]
    c = np.stack([(elites == a).sum(2) for a in range(9)], -1).astype(np.uint64)
    f = (c << np.uint64(16)) // np.uint64(E)
    old = read_weights(w)
    s = np.uint64(shift)
    new = np.minimum(np.uint64(W_MAX), np.maximum(np.uint64(w_min), old - (old >> s) + (f >> s))).astype(np.uint32)
    top = table[np.arange(M), :, o[:, 0]]
    on = np.ones(M, bool) if active is None else np.asarray(active) != 0
    res_w = np.array(w, np.uint32)
    res_b = np.zeros((M, H), np.uint8) if best_seq is None else np.array(best_seq, np.uint8)
    res_w[on], res_b[on] = new[on], top[on]
    return res_w, res_b


def plan(w, score, K, E, iterations, seed, offset0, shift=1, w_min=64):
    """score(tables uint8 [M, H, K]) -> a dict with ret [M, K], best_k, best_action, best_ret [M] (sequences_reference.rollout's).
    Returns the last iteration's dict with `weights` (after the last refit), `tables` (the last ones), `best_seq`, `iter_best_ret` and
    `iter_best_action` [iterations, M] added."""
    w = np.array(w, np.uint32)
    keep, best, first = None, [], []
    for i in range(iterations):
        tables = sample(w, K, seed, offset0 + i, True, keep)
        out = dict(score(tables))
        best.append(np.array(out["best_ret"]))
        first.append(np.array(out["best_action"]))
        w, keep = refit(w, out["ret"], tables, E, shift, w_min)
    out.update(weights=w, tables=tables, best_seq=keep, iter_best_ret=np.stack(best), iter_best_action=np.stack(first))
    return out


def oracle_scorer(name, n, state):
    return lambda tables: Q.rollout(name, n, state, tables)


def uniform_weights(M, H, value=INIT_WEIGHT):
    return np.full((M, H, 9), value, np.uint32)


_driven = {}


def driven(name, n):
    """256 states a planner has driven to: 16 oracle envs from reset, 128 steps without auto-reset under uniform shooting (sample on
    uniform weights, K = 64, H = 12, seed 2, offset = the step, the constant columns in, scored by sequences_reference.rollout, each env
    taking its best first action); after every 8th step the envs still alive give a row each.  The rows go through
    safe_actions_reference.with_turns: the rotation a handle starts from."""
    if (name, n) not in _driven:
        N, K, H = 16, 64, 12
        env = oracle.OracleVecEnv(R.track(name), N, n)
        env.reset()
        alive = np.ones(N, bool)
        rows = {k: [] for k in Q.STATE_KEYS}
        w = uniform_weights(N, H)
        for t in range(128):
            state = {k: getattr(env, k).copy() for k in Q.STATE_KEYS}
            act = Q.rollout(name, n, state, sample(w, K, 2, t))["best_action"]
            _, _, term, trunc = env.raw_step(act)
            alive &= ~(term | trunc)
            if t % 8 == 7:
                for k in Q.STATE_KEYS:
                    rows[k].append(getattr(env, k)[alive].copy())
        s = S.with_turns(name, {k: np.concatenate(v) for k, v in rows.items()})
        assert len(s["px"]) == DRIVEN_ROWS, len(s["px"])
        _driven[(name, n)] = s
    return {k: v.copy() for k, v in _driven[(name, n)].items()}


_ref = {}


def reference(name, n):
    """(driven rows, plan() on them at the *_REF parameters scored by the oracle): computed once per config, never modified"""
    if (name, n) not in _ref:
        s = driven(name, n)
        _ref[(name, n)] = (s, plan(uniform_weights(len(s["px"]), H_REF), oracle_scorer(name, n, s), K_REF, E_REF, ITERATIONS_REF, SEED_REF, 0))
    return _ref[(name, n)]


def counts(ref):
    first, last = ref["iter_best_ret"][0], ref["iter_best_ret"][-1]
    return dict(improved=int((last > first).sum()), action_changed=int((ref["iter_best_action"][0] != ref["iter_best_action"][-1]).sum()),
                drawn_best=int((ref["best_k"] >= 10).sum()))
