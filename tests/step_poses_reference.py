"""Plain reference of pc_env_step_poses: one CarEnv.step (car_env.py:693-760) of caller-supplied states without auto-reset, through the
oracle's raw step, plus the two state recipes the GPU tests step: the injected edge states and the near-gate states."""
import numpy as np

from conftest import TRACKS      # (first: it puts the repository root on sys.path)

import oracle  # noqa: E402
from oracle.scenarios import injected_state, rot_after  # noqa: E402

CONFIGS = (("big_track", 16), ("track", 12), ("oval64", 16))
REWARD_SCALE = 0.1
GATE_CODES = (1, 11, -2, 8)      # rint(reward - 0.01 * forward): a gate, a gate closing a lap, the same two with the -3 of a crash
# what the recipes give on the CPU oracle, under any action (near-gate) / over all 9 actions (edge)
NEAR_GATE_COUNTS = {("big_track", 16): dict(gates=198, laps=96, truncated=80, terminated=0),
                    ("track", 12): dict(gates=210, laps=108, truncated=80, terminated=0),
                    ("oval64", 16): dict(gates=211, laps=108, truncated=80, terminated=0)}
EDGE_COUNTS = {("big_track", 16): dict(terminated=172, truncated=468), ("track", 12): dict(terminated=212, truncated=468),
               ("oval64", 16): dict(terminated=142, truncated=468)}

_tracks = {}


def track(name):
    if name not in _tracks:
        _tracks[name] = oracle.Track(TRACKS[name])
    return _tracks[name]


def turns_of(rot, start_rot):
    return np.rint((np.asarray(rot, np.float64) - start_rot) / 5.0).astype(np.int32)


def step(name, n, state, actions, reward_scale=REWARD_SCALE):
    """state: dict of px, py, vx, vy, rot (float64), time_step, next_gate (integers), M entries each; actions [M] in 0 .. 8.  Returns
    a dict: obs [M, D] float32, reward float32 = np.float32(rew * reward_scale), terminated, truncated, gate (bool), and the new
    px, py, vx, vy, rot, time_step, next_gate."""
    t = track(name)
    actions = np.ascontiguousarray(actions, np.int64)
    M = len(actions)
    env = oracle.OracleVecEnv(t, M, n)
    env.set_state(passed=0, destroyed=0, **{k: state[k] for k in ("px", "py", "vx", "vy", "rot", "time_step", "next_gate")})
    obs, rew, term, trunc = env.raw_step(actions)
    fwd = np.isin(actions, (0, 4, 5))
    code = np.rint(rew - 0.01 * fwd).astype(np.int64)
    out = dict(obs=obs, reward=(rew * reward_scale).astype(np.float32), terminated=term, truncated=trunc, gate=np.isin(code, GATE_CODES))
    for k in ("px", "py", "vx", "vy", "rot", "time_step", "next_gate"):
        out[k] = getattr(env, k).copy()
    return out


def edge_states(name):
    """oracle.scenarios.injected_state of envs 0 .. 299: the time limit, +-990 turns, a crash in the step in which the limit falls due;
    with the turn count of every rotation."""
    t = track(name)
    s = injected_state(TRACKS[name], np.arange(300))
    s["turns"] = turns_of(s["rot"], t.start_rot)
    return s


def near_gate_states(name):
    """240 rows on the approach to a gate: row i is 2 + (i // 2) % 10 px before the midpoint of gate gi (G - 1 for even i, else
    (7 i) % (G - 1)) on the line from the previous gate's midpoint, heading the nearest turn count of that line, 6 px per step along
    it, next_gate = gi, time_step 999 for i % 3 == 0, else 100."""
    t = track(name)
    n = 240
    mid = np.stack([(t.gates[:, 0] + t.gates[:, 2]) / 2, (t.gates[:, 1] + t.gates[:, 3]) / 2], 1)
    s = {k: np.zeros(n, np.float64) for k in ("px", "py", "vx", "vy", "rot")}
    s["time_step"], s["next_gate"], s["turns"] = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
    for i in range(n):
        gi = t.G - 1 if i % 2 == 0 else (7 * i) % (t.G - 1)
        u = mid[gi] - mid[gi - 1]
        u = u / np.linalg.norm(u)
        back = 2.0 + (i // 2) % 10
        k = int(np.rint((np.degrees(np.arctan2(u[1], u[0])) - t.start_rot) / 5.0))
        s["px"][i], s["py"][i] = mid[gi] - back * u
        s["vx"][i], s["vy"][i] = 6.0 * u
        s["rot"][i], s["turns"][i] = rot_after(t.start_rot, k), k
        s["next_gate"][i] = gi
        s["time_step"][i] = 999 if i % 3 == 0 else 100
    return s


def all_actions(state):
    """The state's rows under each of the 9 actions: [9 * M] rows, action a in rows a * M .. (a + 1) * M - 1."""
    M = len(state["px"])
    rep = {k: np.tile(v, 9) for k, v in state.items()}
    return rep, np.repeat(np.arange(9, dtype=np.int64), M)


def counts(ref, next_gate_after):
    return dict(gates=int(ref["gate"].sum()), laps=int((ref["gate"] & (next_gate_after == 0)).sum()),
                truncated=int(ref["truncated"].sum()), terminated=int(ref["terminated"].sum()))
