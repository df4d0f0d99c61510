"""Plain reference of pc_env_safe_actions on the CPU oracle, and the state recipes the tests search from.

    safe(s, a, 1) = not terminated(step(s, a))
    safe(s, a, d) = not terminated(s' = step(s, a)) and (truncated(s') or exists a' in 0 .. 8: safe(s', a', d - 1))

masks(): every row replicated 9^d times, one copy per action sequence; OracleVecEnv.set_state once, raw_step d times; a copy that
terminated or truncated is frozen (what the oracle goes on computing for it is ignored); folded back to [M, 9] over the sequences that
share a first action.  A copy's fate after j steps depends on its first j actions only, so the same run gives the masks of every depth
1 .. d."""
import os

import numpy as np

import step_poses_reference as R      # (first: through conftest it puts the repository root on sys.path)

import oracle  # noqa: E402
from oracle.scenarios import rot_after  # noqa: E402

CONFIGS = R.CONFIGS
STATE_KEYS = ("px", "py", "vx", "vy", "rot", "time_step", "next_gate")
PRE_CRASH_ACTIONS = (0, 0, 4, 5, 4, 5, 8, 2, 3)
# Row i lies 1 + i % PRE_CRASH_LEAD steps before its env's crash.  The shares asked of the rows -- at least 5 % empty, 5 % full and 10 %
# partial masks for every config at depths 1, 2, 3 -- are kept; the lead is what gives way.  A lead of 6 leaves 7.8 % / 9.8 % / 8.6 %
# partial masks at depth 1 (big_track / track / oval64), and a WIDER one dilutes them further (10: 6.2 % / 7.8 % / 4.3 %): a mask is
# mixed only in the last steps before the wall.  2 has no full mask left at depth 3; 3 holds every share (partial >= 15 %, empty >= 22 %,
# full >= 14 %), 4 and 5 miss on big_track at depth 1 (9.4 %).
PRE_CRASH_LEAD = 3
SHARES = (0.05, 0.10, 0.05)      # (empty, partial, full)
# (rows, [(empty, partial, full) at depth 1, 2, 3]) of pre_crash_states on the CPU oracle; no env of the 256 reaches the time limit
PRE_CRASH_COUNTS = {("big_track", 16): (256, [(62, 39, 155), (107, 62, 87), (145, 65, 46)]),
                    ("track", 12): (256, [(57, 46, 153), (110, 60, 86), (144, 70, 42)]),
                    ("oval64", 16): (256, [(57, 47, 152), (107, 64, 85), (147, 73, 36)])}
# the other two recipes: near_gate's 240 rows are all full at every depth (open road; they are there for the time limit: a third truncate)
EDGE_COUNTS = {("big_track", 16): [(16, 8, 276), (26, 12, 262), (31, 12, 257)], ("track", 12): [(20, 8, 272), (30, 12, 258), (34, 13, 253)],
               ("oval64", 16): [(12, 8, 280), (22, 12, 266), (26, 14, 260)]}
_THREADS = max(1, min(16, os.cpu_count() or 1))


def sequences(depth):
    """[9^depth, depth] int64: every action sequence, the first action the slowest index"""
    return np.stack(np.unravel_index(np.arange(9 ** depth), (9,) * depth), 1).astype(np.int64)


def masks(name, n, state, depth):
    """state: dict of px, py, vx, vy, rot (float64), time_step (integers), M entries each (next_gate optional: gates play no part).
    Returns [depth][M, 9] bool: entry d - 1 is the mask at depth d."""
    M = len(state["px"])
    seq = sequences(depth)
    K = len(seq)
    env = oracle.OracleVecEnv(R.track(name), M * K, n, threads=_THREADS)
    env.set_state(passed=0, destroyed=0, **{k: np.repeat(np.asarray(state[k]), K) for k in STATE_KEYS if k in state})
    dead = np.zeros(M * K, bool)
    frozen = np.zeros(M * K, bool)
    out = []
    for j in range(depth):
        _, _, term, trunc = env.raw_step(np.tile(seq[:, j], M))
        dead |= term & ~frozen
        frozen |= term | trunc
        alive = (~dead).reshape(M, 9, K // 9)      # [state][first action][the rest of the sequence]
        out.append(alive.any(2))
    return out


def with_turns(name, s):
    """The rows with the turn count of their rotation, and the rotation that count names (the one-way sum): what a handle starts from."""
    start = R.track(name).start_rot
    s = dict(s)
    s["turns"] = R.turns_of(s["rot"], start)
    s["rot"] = np.array([rot_after(start, int(k)) for k in s["turns"]])
    return s


def edge_states(name):
    return R.edge_states(name)


def near_gate_states(name):
    return R.near_gate_states(name)


_pre = {}


def pre_crash_states(name, n, lead=PRE_CRASH_LEAD):
    """256 oracle envs driven from reset without auto-reset under actions drawn by default_rng(11) from PRE_CRASH_ACTIONS; row i is env
    i's state 1 + i % lead steps before its crash (the state its crashing step starts from is 1 step before).  Envs that reach the
    time limit are dropped.  Real approaches to a wall at speed; the rotation is put on the one-way row of its turn count."""
    key = (name, n, lead)
    if key in _pre:
        return {k: v.copy() for k, v in _pre[key].items()}
    N = 256
    env = oracle.OracleVecEnv(R.track(name), N, n)
    env.reset()
    rng = np.random.default_rng(11)
    table = np.asarray(PRE_CRASH_ACTIONS, np.int64)
    history = []
    crash = np.full(N, -1)
    over = np.zeros(N, bool)
    for t in range(1000):
        history.append({k: getattr(env, k).copy() for k in STATE_KEYS})
        _, _, term, trunc = env.raw_step(table[rng.integers(0, len(table), N)])
        crash[term & ~over] = t
        over |= term | trunc
        if over.all():
            break
    rows = [i for i in range(N) if crash[i] >= 0]
    at = [max(int(crash[i]) - i % lead, 0) for i in rows]
    s = {k: np.array([history[t][k][i] for i, t in zip(rows, at)]) for k in STATE_KEYS}
    _pre[key] = with_turns(name, s)
    return pre_crash_states(name, n, lead)


def classes(mask):
    """(empty, partial, full) rows of a [M, 9] mask"""
    c = mask.sum(1)
    return int((c == 0).sum()), int(((c > 0) & (c < 9)).sum()), int((c == 9).sum())


RECIPES = {"edge": lambda name, n: edge_states(name), "near_gate": lambda name, n: near_gate_states(name), "pre_crash": pre_crash_states}
_ref = {}


def reference(name, n, recipe, depth=3):
    """(state rows, [depth][M, 9] masks): computed once per config and recipe at the deepest depth asked so far, never modified"""
    key = (name, n, recipe)
    if key not in _ref or len(_ref[key][1]) < depth:
        s = RECIPES[recipe](name, n)
        _ref[key] = (s, masks(name, n, s, depth))
    return _ref[key]
