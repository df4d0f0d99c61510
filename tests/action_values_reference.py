"""pc_sequences_action_values (K28) restated in numpy: the rules of include/ppocar.h, one state and one sequence at a time.  Never the
code under test.  Also the synthetic tables the host and GPU tests share."""
import numpy as np

N_ACTIONS = 9
TERMINATED = 1      # PC_FIRST_TERMINATED
SENTINEL = 77
MS = (1, 3, 4, 5, 9)
KS = (1, 9, 63, 64, 65, 129, 4096)
TEMPERATURES = (0.0, 0.05, 1.0)
# returns are drawn from this small set, so exact ties within an action and across actions are frequent; -0.0 and 0.0 compare equal and
# differ in bits (the FIRST maximum's bits are kept).  With case()'s 0.5 the spread is 1.25: at temperature 0.05 the smallest non-zero
# target entry is above exp(-25) / 9 = 1.5e-12, a normal float32 (asserted in test_action_values_host.py).
VALUES = np.array([-0.75, -0.5, -0.0, 0.0, 0.125, 0.25], dtype=np.float64)


def empty(M):
    """the outputs before a state's first call"""
    return dict(q=np.full((M, N_ACTIONS), -np.inf), count=np.zeros((M, N_ACTIONS), np.int32), alive=np.zeros((M, N_ACTIONS), np.uint8),
                target=np.zeros((M, N_ACTIONS), np.float32))


def action_values(ret, first, steps=None, status=None, active=None, accumulate=False, temperature=0.0, prev=None):
    """ret [M, K] float64; first [K] (shared) or [M, K] uint8: the table's first time row; steps / status [M, K] or None; active [M] or
    None; prev: the outputs to merge into (accumulate) and to leave alone where a row is inactive.  Returns a dict of new arrays."""
    ret = np.asarray(ret, np.float64)
    M, K = ret.shape
    first = np.broadcast_to(np.asarray(first, np.uint8), (M, K))
    out = {k: v.copy() for k, v in (prev if prev is not None else empty(M)).items()}
    for m in range(M):
        if active is not None and active[m] == 0:
            continue
        q = np.full(N_ACTIONS, -np.inf)
        count = np.zeros(N_ACTIONS, np.int32)
        alive = np.zeros(N_ACTIONS, np.uint8)
        for k in range(K):
            a = min(int(first[m, k]), 8)
            v = ret[m, k]
            if count[a] == 0 or v > q[a]:
                q[a] = v
            count[a] += 1
            dead = status is not None and status[m, k] == TERMINATED and steps[m, k] == 1
            if not dead:
                alive[a] = 1
        if status is None:
            alive = (count > 0).astype(np.uint8)
        if accumulate:
            old = out["q"][m]
            q = np.where(q > old, q, old)
            count = count + out["count"][m]
            alive = alive | out["alive"][m]
        out["q"][m], out["count"][m], out["alive"][m] = q, count, alive
        out["target"][m] = target_row(q, alive, temperature)
    return out


def target_row(q, alive, temperature):
    t = np.zeros(N_ACTIONS, np.float32)
    S = [a for a in range(N_ACTIONS) if alive[a]]
    if not S:
        return t
    qmax = max(q[a] for a in S)
    if temperature == 0.0:
        top = [a for a in S if q[a] == qmax]
        for a in top:
            t[a] = np.float32(1.0 / len(top))
        return t
    e = {a: np.exp((q[a] - qmax) / temperature) for a in S}
    total = 0.0
    for a in S:      # ascending a
        total += e[a]
    for a in S:
        t[a] = np.float32(e[a] / total)
    return t


def case(M, K, per_state, seed):
    """One synthetic table: ret, first, steps, status, active.  Bytes run over 0 .. 255 (those above 8 act as 8).  By construction:
      row 0                 every sequence dead at once (M >= 1)
      row 1                 only the sequences of actions 0 .. 2 alive; the row's maximum belongs to a dead action (M >= 3)
      row 2 where M >= 4    inactive, between two active rows
    and with K < 9 some action has count 0 in every row."""
    rng = np.random.default_rng(seed)
    ret = VALUES[rng.integers(0, len(VALUES), (M, K))]
    shape = (M, K) if per_state else (K,)
    first = rng.integers(0, 9, shape).astype(np.uint8)
    wide = rng.random(shape) < 0.15
    first = np.where(wide, rng.integers(9, 256, shape), first).astype(np.uint8)
    fm = np.broadcast_to(first, (M, K))
    status = rng.integers(0, 3, (M, K)).astype(np.uint8)
    steps = rng.integers(1, 4, (M, K)).astype(np.int32)
    status[0], steps[0] = TERMINATED, 1
    if M >= 3:
        dead = np.minimum(fm[1], 8) > 2
        status[1] = np.where(dead, TERMINATED, 0)
        steps[1] = np.where(dead, 1, 3)
        if dead.any():
            ret[1] = np.where(dead, ret[1], np.minimum(ret[1], 0.125))
            ret[1, np.argmax(dead)] = 0.5      # the row's maximum: a sequence that is dead at once
    active = np.ones(M, np.uint8)
    if M >= 4:
        active[2] = 0
    return dict(ret=ret, first=first, steps=steps, status=status, active=active)


def cases():
    """(id, M, K, per_state, seed) of every table the tests run"""
    out = []
    for i, M in enumerate(MS):
        for j, K in enumerate(KS):
            for per_state in (False, True):
                out.append((f"M{M}-K{K}-{'own' if per_state else 'shared'}", M, K, per_state, 1000 + 100 * i + 10 * j + per_state))
    return out
