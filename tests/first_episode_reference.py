"""Plain numpy reference of pc_first_episodes' state (include/ppocar.h): per env, forward in t, float64.  A helper of the evaluation
tests, like draw_reference.py; no GPU, no library.

state [8, N]: 0 return (float64 sum of the float32 scaled rewards)  1 length  2 gates  3 laps  4 status (0 running, 1 terminated,
2 truncated; both flags = terminated)  5 the step count at the last lap close (0 = none)  6 best lap in steps (+inf = none)
7 first lap in steps (+inf = none).  Only the FIRST episode of an env counts: an env whose status is not 0 is left alone."""
import numpy as np

ROWS = 8
RUNNING, TERMINATED, TRUNCATED = 0, 1, 2


def new_state(N):
    s = np.zeros((ROWS, N), np.float64)
    s[6:] = np.inf
    return s


def buffer_flags(term, trunc, last_term, last_trunc):
    """Buffer layout -> step layout: step t's flags sit in row t + 1, step T - 1's in last_* (row 0 is not read)."""
    return (np.concatenate([term[1:], np.asarray(last_term)[None]], axis=0),
            np.concatenate([trunc[1:], np.asarray(last_trunc)[None]], axis=0))


def first_episodes_ref(rew, term, trunc, scale, state=None):
    """rew, term, trunc [T, N] in the STEP layout (flags[t] belong to rew[t]) -> the state after the window (a new array)."""
    rew = np.asarray(rew, np.float32)
    T, N = rew.shape
    s = new_state(N) if state is None else np.array(state, np.float64)
    for t in range(T):
        for e in range(N):
            if s[4, e] != RUNNING:
                continue
            r = np.float64(rew[t, e])
            k = int(np.rint(r / scale))
            s[0, e] += r
            s[1, e] += 1
            s[2, e] += k in (1, 11, -2, 8)
            if k in (11, 8):
                lap = s[1, e] - s[5, e]
                if s[3, e] == 0:
                    s[7, e] = lap
                s[6, e] = min(s[6, e], lap)
                s[5, e] = s[1, e]
                s[3, e] += 1
            s[4, e] = TERMINATED if term[t, e] != 0 else (TRUNCATED if trunc[t, e] != 0 else RUNNING)
    return s
