"""K25 / K26 (pc_env_rollout_sequences_value / _value_state; VecCarEnv.rollout_sequences / score_sequences with gamma, bootstrap, agent),
the planners with a critic and evaluate.py's options on the GPU.

Every comparison is an equality of bits, except the one tolerance check of the value against the float64 critic.  F64 handles against the
CPU oracle (sequences_value_reference), F32 handles against H chained pc_env_step_poses calls on the same handle.  The value the references
combine is what ONE Agent.act(greedy=True) call gives for the reference's end observations as one [M * K, D] tensor."""
import json

import numpy as np
import pytest
import torch

import ppo_car_amd as pc
from ppo_car_amd import _capi
from ppo_car_amd.evaluation import EVAL_KEYS
from conftest import TRACKS
import oracle
import step_poses_reference as R
import sequences_reference as Q
import sequences_value_reference as V
import cem_reference as X

pytestmark = pytest.mark.gpu

F64_KEYS = ("px", "py", "vx", "vy")
K22_OUT = (("ret", torch.float64, True), ("steps", torch.int32, True), ("status", torch.uint8, True), ("gates", torch.int32, True),
           ("laps", torch.int32, True), ("best_k", torch.int32, False), ("best_action", torch.int64, False), ("best_ret", torch.float64, False))
NEW_OUT = (("end_obs", torch.float32), ("end_value", torch.float32), ("end_discount", torch.float64), ("ret_env", torch.float64))
K22_KEYS = tuple(o[0] for o in K22_OUT)
NEW_KEYS = tuple(o[0] for o in NEW_OUT)
NO_POLICY_KEYS = K22_KEYS + ("end_obs", "end_discount", "ret_env")
REQUIRED = ("ret", "steps", "status")
INVARIANT = ("steps", "status", "gates", "laps")      # never depend on gamma, bootstrap or the policy
SENTINEL = 77
MODE_NAMES = {v: k for k, v in V.MODES.items()}


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _same(got, want, keys, what):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(_bits(g), _bits(w)), (what, k, np.argwhere(_bits(g) != _bits(w))[:8])


def _env(track, n, dtype, N=1):
    return pc.VecCarEnv(N, TRACKS[track], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype=dtype)


_agents = {}


def _agent(n):
    """(the config's test policy on the GPU, its weights as numpy arrays): one per obs dim"""
    if n not in _agents:
        agent, w = V.agent_for(n)
        _agents[n] = (agent.cuda(), w)
    return _agents[n]


def _value(agent, end_obs):
    """ONE greedy policy step over end_obs [M, K, D] as [M * K, D]: float32 [M, K]"""
    M, K, D = end_obs.shape
    x = torch.from_numpy(np.ascontiguousarray(end_obs.reshape(M * K, D))).cuda()
    return agent.act(x, greedy=True)[2].cpu().numpy().reshape(M, K)


def _filled(M, K, D, keys):
    out = {name: torch.full((M, K) if per_lane else (M,), SENTINEL, dtype=dtype, device="cuda") for name, dtype, per_lane in K22_OUT
           if name in keys}
    for name, dtype in NEW_OUT:
        if name in keys:
            out[name] = torch.full((M, K, D) if name == "end_obs" else (M, K), SENTINEL, dtype=dtype, device="cuda")
    return out


def _tensors(s, table, track_id=None, active=None):
    t = {k: _dev(s[k], torch.float64) for k in F64_KEYS}
    t.update(turns=_dev(s["turns"], torch.int32), next_gate=_dev(s["next_gate"], torch.int32), time_step=_dev(s["time_step"], torch.int32))
    if track_id is not None:
        t["track_id"] = _dev(track_id, torch.uint8)
    if active is not None:
        t["active"] = _dev(active, torch.uint8)
    t["actions"] = _dev(table, torch.uint8)
    return t


def _score(env, s, table, gamma=None, mode=None, agent=None, keys=None, track_id=None, active=None):
    """One rollout_sequences call on device copies of the numpy rows s, the outputs pre-filled with a sentinel: dict of numpy arrays.
    The inputs must come back as they went in.  gamma / mode / agent all None: the K22 call."""
    plain = gamma is None and mode is None and agent is None
    if keys is None:
        keys = K22_KEYS if plain else (K22_KEYS + NEW_KEYS if agent is not None else NO_POLICY_KEYS)
    t = _tensors(s, table, track_id, active)
    keep = {k: v.clone() for k, v in t.items()}
    M, K = len(s["px"]), t["actions"].shape[-1]
    out = _filled(M, K, env.obs_dim, keys)
    kw = {} if plain else dict(gamma=gamma, bootstrap=None if mode is None else MODE_NAMES[mode], agent=agent)
    got = env.rollout_sequences(t["px"], t["py"], t["vx"], t["vy"], t["turns"], t["actions"], next_gate=t["next_gate"], time_step=t["time_step"],
                                track_id=t.get("track_id"), active=t.get("active"), out=out, **kw)
    assert set(got) == set(keys) and all(got[k].data_ptr() == out[k].data_ptr() for k in keys)
    for k in t:
        assert torch.equal(t[k], keep[k]), k      # read only
    return {k: v.cpu().numpy() for k, v in out.items()}


def _expected(tr, gamma, mode, value):
    """the reference's outputs from a trace (sequences_value_reference.trace's dict, or the chain's) and the policy step's value"""
    ret_env, disc = V.discounted(tr, gamma)
    want = {k: tr[k] for k in INVARIANT}
    want.update(ret_env=ret_env, end_discount=disc, end_obs=tr["end_obs"])
    if value is not None:
        want["end_value"] = value
    want["ret"] = V.combine(ret_env, disc, value, tr["status"], mode) if value is not None else ret_env
    want["best_k"], want["best_action"], want["best_ret"] = V.best(want["ret"], tr["actions"])
    return want


def _consistent(got, table, mode, what):
    """what the definitions alone demand of one call's outputs: ret from its own ret_env, end_discount, end_value and status; K22's rule"""
    M, K = got["ret"].shape
    table = np.asarray(table)
    tabs = np.broadcast_to(table, (M,) + table.shape) if table.ndim == 2 else table
    ret = V.combine(got["ret_env"], got["end_discount"], got["end_value"], got["status"], mode)
    k, a, r = V.best(ret, tabs)
    _same(got, dict(ret=ret, best_k=k, best_action=a, best_ret=r), ("ret",) + Q.BEST_KEYS, what)


# ---- 1. gamma 1, no bootstrap, no policy: K22's bits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("K,H", [(64, 12), (70, 12), (1, 1)])
def test_gamma_one_without_a_policy_is_k22_bit_for_bit(dtype, K, H):
    track, n = "big_track", 16
    s, _ = Q.pooled(track, n)
    M = len(s["px"])
    table = Q.table(H, K)
    env = _env(track, n, dtype)
    want = _score(env, s, table)
    got = _score(env, s, table, gamma=1.0, mode=V.NONE)
    _same(got, want, K22_KEYS, "all")
    assert np.array_equal(_bits(got["ret_env"]), _bits(want["ret"])) and (got["end_discount"] == 1.0).all()
    assert np.isfinite(got["end_obs"]).all() and (got["end_obs"] != SENTINEL).any(2).all()
    part = _score(env, s, table, gamma=1.0, mode=V.NONE, keys=REQUIRED)      # every optional array NULL, the new ones included
    _same(part, want, REQUIRED, "required only")
    only = _score(env, s, table, gamma=1.0, keys=REQUIRED + ("best_k", "ret_env"))
    _same(only, dict(want, ret_env=want["ret"]), REQUIRED + ("best_k", "ret_env"), "some")
    env.close()
    # the state form on a handle put into those rows: score_sequences with gamma = 1 against score_sequences
    env = _env(track, n, dtype, M)
    env.reset()
    env.set_state(passed=0, **{k: s[k] for k in Q.STATE_KEYS})
    before = env.get_state()
    tab = _dev(table, torch.uint8)
    want = {k: v.cpu().numpy() for k, v in env.score_sequences(tab).items()}
    out = _filled(M, K, env.obs_dim, NO_POLICY_KEYS)
    got = env.score_sequences(tab, out=out, gamma=1.0, bootstrap="none")
    assert set(got) == set(NO_POLICY_KEYS)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    _same(got, want, K22_KEYS, "state form")
    assert np.array_equal(_bits(got["ret_env"]), _bits(want["ret"])) and (got["end_discount"] == 1.0).all()
    req = env.score_sequences(tab, out=_filled(M, K, env.obs_dim, REQUIRED), gamma=1.0)
    assert set(req) == set(REQUIRED)
    _same({k: v.cpu().numpy() for k, v in req.items()}, want, REQUIRED, "state form, required only")
    after = env.get_state()
    for k in before:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k      # the env state is not touched
    env.close()


# ---- 2. F64 handles: the CPU oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H", [(64, 1), (64, 3), (64, 12), (70, 12), (1, 12)])
@pytest.mark.parametrize("track,n", Q.CONFIGS)
def test_f64_equals_the_reference(track, n, K, H):
    s, tr = V.pooled_trace(track, n, H, K)
    table = Q.table(H, K)
    agent, _ = _agent(n)
    value = _value(agent, tr["end_obs"])
    env = _env(track, n, "f64")
    k22 = _score(env, s, table)
    _same(k22, tr, INVARIANT, "K22 against the trace")
    for gamma in V.GAMMAS:
        for mode in (V.NONE, V.BOOT_RUNNING, V.BOOT_RUNNING_TRUNCATED):
            got = _score(env, s, table, gamma=gamma, mode=mode, agent=agent)
            _same(got, _expected(tr, gamma, mode, value), K22_KEYS + NEW_KEYS, (gamma, mode))
            _same(got, k22, INVARIANT, (gamma, mode, "K22"))
        nop = _score(env, s, table, gamma=gamma)      # no policy: the discounted sum alone, end_value not asked for
        _same(nop, _expected(tr, gamma, V.NONE, None), NO_POLICY_KEYS, (gamma, "no policy"))
    # the modes do differ on these inputs, and each covers what it says
    st = tr["status"]
    if K > 1:
        assert (st == V.RUNNING).any() and (st == V.TRUNCATED).any() and (st == V.TERMINATED).any()
    e = {m: _expected(tr, 0.99, m, value)["ret"] for m in (V.NONE, V.BOOT_RUNNING, V.BOOT_RUNNING_TRUNCATED)}
    assert np.array_equal(e[V.NONE][st == V.TERMINATED], e[V.BOOT_RUNNING_TRUNCATED][st == V.TERMINATED])
    assert np.array_equal(e[V.NONE][st == V.TRUNCATED], e[V.BOOT_RUNNING][st == V.TRUNCATED])
    if (st == V.RUNNING).any():
        assert (e[V.NONE] != e[V.BOOT_RUNNING])[st == V.RUNNING].mean() > 0.99
    if (st == V.TRUNCATED).any():
        assert (e[V.BOOT_RUNNING] != e[V.BOOT_RUNNING_TRUNCATED])[st == V.TRUNCATED].mean() > 0.99
    env.close()


# ---- 3. F32 handles: H chained K20 calls on the same handle --------------------------------------------------------------------------------
def _chained(env, s, table, track_id=None):
    """sequences_value_reference.trace's dict with pc_env_step_poses on `env` in the oracle's place"""
    M = len(s["px"])
    table = np.asarray(table)
    tabs = np.broadcast_to(table, (M,) + table.shape) if table.ndim == 2 else table
    H, K = tabs.shape[1:]
    rep = lambda a, dt: _dev(np.repeat(np.asarray(a), K), dt)
    px, py, vx, vy = (rep(s[k], torch.float64) for k in F64_KEYS)
    turns, ng, ts = rep(s["turns"], torch.int32), rep(s["next_gate"], torch.int32), rep(s["time_step"], torch.int32)
    tid = None if track_id is None else rep(track_id, torch.uint8)
    steps, gates, laps = (torch.zeros(M * K, dtype=torch.int32, device="cuda") for _ in range(3))
    status = torch.zeros(M * K, dtype=torch.uint8, device="cuda")
    end_obs = torch.zeros(M * K, env.obs_dim, dtype=torch.float32, device="cuda")
    rew, lives = [], []
    for t in range(H):
        live = status == Q.RUNNING
        acts = _dev(np.minimum(tabs[:, t, :].reshape(-1), 8), torch.int64)
        r = env.step_poses(px, py, vx, vy, turns, acts, next_gate=ng, time_step=ts, track_id=tid, active=live.to(torch.uint8))
        rew.append(r.reward.to(torch.float64).cpu().numpy())      # (a frozen row's outputs are stale: `live` masks them)
        lives.append(live.cpu().numpy())
        end_obs = torch.where(live[:, None], r.obs, end_obs)
        steps += live.to(torch.int32)
        gate = live & (r.gate != 0)
        gates += gate.to(torch.int32)
        laps += (gate & (ng == 0)).to(torch.int32)
        now = torch.where(r.terminated != 0, Q.TERMINATED, torch.where(r.truncated != 0, Q.TRUNCATED, Q.RUNNING)).to(torch.uint8)
        status = torch.where(live, now, status)
    tr = {k: v.reshape(M, K).cpu().numpy() for k, v in dict(steps=steps, status=status, gates=gates, laps=laps).items()}
    tr.update(rew=np.stack(rew), live=np.stack(lives), end_obs=end_obs.cpu().numpy().reshape(M, K, -1), actions=tabs)
    return tr


@pytest.mark.parametrize("track,n", Q.CONFIGS)
def test_f32_equals_chained_step_poses(track, n):
    K, H = Q.K_REF, Q.H_REF
    s, _ = Q.pooled(track, n)
    table = Q.table(H, K)
    env = _env(track, n, "f32")
    agent, _ = _agent(n)
    tr = _chained(env, s, table)
    assert len(np.unique(tr["status"])) == 3
    value = _value(agent, tr["end_obs"])
    for gamma, mode in ((0.99, V.BOOT_RUNNING), (0.99, V.BOOT_RUNNING_TRUNCATED), (0.5, V.BOOT_RUNNING), (0.0, V.BOOT_RUNNING_TRUNCATED),
                        (1.0, V.NONE), (1.0, V.BOOT_RUNNING)):
        got = _score(env, s, table, gamma=gamma, mode=mode, agent=agent)
        _same(got, _expected(tr, gamma, mode, value), K22_KEYS + NEW_KEYS, (gamma, mode))
    env.close()


# ---- 4. the value against the float64 critic -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("track,n", Q.CONFIGS)
def test_end_value_is_the_critic_of_end_obs(track, n, dtype):
    """The tolerance tests/test_policy_draw_gpu.py holds the policy step's value to (_verify_policy): |value - float64 critic| below 4e-6
    relative to max(1, the largest float64 logit magnitude)."""
    K, H = 64, 4
    s, _ = Q.pooled(track, n)
    env = _env(track, n, dtype)
    agent, w = _agent(n)
    got = _score(env, s, Q.table(H, K), gamma=0.99, mode=V.BOOT_RUNNING, agent=agent)
    L64, V64 = V.critic_f64(w, got["end_obs"])
    mag = max(1.0, float(np.abs(L64).max()))
    err = float(np.abs(got["end_value"].astype(np.float64) - V64).max()) / mag
    print(f"{track} {n} {dtype}: value error {err:.2e} relative to {mag:.2f}, values {V64.min():.3f} .. {V64.max():.3f}")
    assert err < 4e-6
    _consistent(got, Q.table(H, K), V.BOOT_RUNNING, "consistent")
    env.close()


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------------
def _mixed_rows(track, n, M):
    s, _ = Q.pooled(track, n)
    perm = np.random.default_rng(3).permutation(len(s["px"]))[:M]
    return {k: v[perm] for k, v in s.items()}


LANE_KEYS = INVARIANT + ("ret_env", "end_discount", "end_obs")      # what does not pass through the policy step (whose form depends on N)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_per_state_tables_equal_single_state_calls(dtype):
    track, n, M, H, K = "big_track", 16, 37, 7, 20
    s = _mixed_rows(track, n, M)
    tabs = np.stack([Q.table(H, K, seed=100 + m) for m in range(M)])
    env = _env(track, n, dtype)
    agent, _ = _agent(n)
    got = _score(env, s, tabs, gamma=0.99, mode=V.BOOT_RUNNING_TRUNCATED, agent=agent)
    assert len(np.unique(got["status"])) == 3
    _consistent(got, tabs, V.BOOT_RUNNING_TRUNCATED, "all states")
    nop = _score(env, s, tabs, gamma=0.99)
    for m in range(M):
        row = {k: v[m:m + 1] for k, v in s.items()}
        one = _score(env, row, tabs[m], gamma=0.99, mode=V.BOOT_RUNNING_TRUNCATED, agent=agent)
        _same({k: got[k][m:m + 1] for k in got}, one, LANE_KEYS, m)
        _consistent(one, tabs[m], V.BOOT_RUNNING_TRUNCATED, m)
        _same({k: nop[k][m:m + 1] for k in nop}, _score(env, row, tabs[m], gamma=0.99), NO_POLICY_KEYS, (m, "no policy"))
    if dtype == "f64":
        tr = V.trace(track, n, s, tabs)
        _same(got, _expected(tr, 0.99, V.BOOT_RUNNING_TRUNCATED, _value(agent, tr["end_obs"])), K22_KEYS + NEW_KEYS, "oracle")
    env.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_inactive_rows_unknown_tracks_and_action_bytes(dtype):
    track, n, M, H, K = "big_track", 16, 257, 6, 13      # 257 x 13 lanes: no multiple of a wave or a workgroup
    s = _mixed_rows(track, n, M)
    env = _env(track, n, dtype, 3)
    env.reset()
    before = env.get_state()
    agent, _ = _agent(n)
    table = Q.table(H, K)
    mode = V.BOOT_RUNNING_TRUNCATED
    full = _score(env, s, table, gamma=0.99, mode=mode, agent=agent)
    assert len(np.unique(full["status"])) == 3 and (full["steps"] >= 1).all() and (full["steps"] <= H).all()
    _consistent(full, table, mode, "full")
    _same(_score(env, s, table, gamma=0.99, mode=mode, agent=agent), full, K22_KEYS + NEW_KEYS, "repeat")
    # active == 0: the sentinel stays in every output array but end_value
    active = (np.arange(M) % 3 != 1).astype(np.uint8)
    on = active != 0
    part = _score(env, s, table, gamma=0.99, mode=mode, agent=agent, active=active)
    for k in K22_KEYS + NEW_KEYS:
        assert np.array_equal(_bits(part[k][on]), _bits(full[k][on])), k
        if k != "end_value":
            assert (part[k][~on] == SENTINEL).all(), k
    nop = _score(env, s, table, gamma=0.99, active=active)
    for k in NO_POLICY_KEYS:
        assert (nop[k][~on] == SENTINEL).all(), k
    # a track the handle does not have: K22's zeros, an end_obs row of zeros, end_discount 1, ret_env 0, never bootstrapped
    tid = np.zeros(M, np.uint8)
    tid[[0, 100, 256]] = (1, 255, 7)
    bad = tid != 0
    got = _score(env, s, table, gamma=0.99, mode=mode, agent=agent, track_id=tid)
    for k in K22_KEYS + NEW_KEYS:
        assert np.array_equal(_bits(got[k][~bad]), _bits(full[k][~bad])), k
        if k != "end_value":
            assert (got[k][bad] == {"best_action": 8, "end_discount": 1}.get(k, 0)).all(), k
    zero_value = _value(agent, np.zeros((1, 1, env.obs_dim), np.float32))[0, 0]
    assert zero_value != 0.0 and np.abs(got["end_value"][bad] - zero_value).max() < 1e-5      # the critic of the zero row: not added
    both = _score(env, s, table, gamma=0.99, mode=mode, agent=agent, track_id=tid, active=active)
    for k in K22_KEYS + NEW_KEYS:
        assert np.array_equal(_bits(both[k][on]), _bits(got[k][on])), k
        assert k == "end_value" or (both[k][~on] == SENTINEL).all(), k
    # an action byte outside 0 .. 8 acts as 8
    eight = table.copy()
    eight[2, 10] = eight[4, 12] = eight[0, 9] = 8
    odd = eight.copy()
    odd[eight == 8] = 200
    odd[:, 8], eight[:, 8] = 9, 8
    odd[0, 8] = 255
    a, b = (_score(env, s, t, gamma=0.99, mode=mode, agent=agent) for t in (odd, eight))
    _same(a, b, K22_KEYS + NEW_KEYS, "bytes above 8")
    assert (a["best_action"] <= 8).all()
    after = env.get_state()
    for k in before:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k      # the handle's own state is neither read nor written
    env.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_two_tracks_in_one_wave(dtype):
    n, M, H, K = 16, 200, 8, 9      # 7 states per wave: both tracks sit in every wave
    s = _mixed_rows("big_track", n, M)
    table = Q.table(H, K)
    agent, _ = _agent(n)
    mode = V.BOOT_RUNNING
    singles = []
    for track in ("track", "big_track"):
        env = _env(track, n, dtype)
        singles.append(_score(env, s, table, gamma=0.99, mode=mode, agent=agent))
        env.close()
    env = pc.VecCarEnv(2, [TRACKS["track"], TRACKS["big_track"]], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype=dtype,
                       track_id=np.array([0, 1], np.uint8))
    tid = (np.arange(M) & 1).astype(np.uint8)
    both = _score(env, s, table, gamma=0.99, mode=mode, agent=agent, track_id=tid)
    _consistent(both, table, mode, "both")
    for k in (0, 1):
        sel = tid == k
        _same({key: both[key][sel] for key in both}, {key: singles[k][key][sel] for key in both}, LANE_KEYS, k)
    assert not np.array_equal(both["end_obs"][0::2], singles[1]["end_obs"][0::2])      # (the two tracks do differ)
    env.close()


def test_the_time_limit_and_a_crash_in_the_step_it_falls_due():
    """time_step 998, H = 3: a lane that survives two steps ends TRUNCATED after them -- bootstrapped in mode 2, not in mode 1.
    time_step 999: the first step is the one in which the limit falls due; a lane that crashes in it is TERMINATED and bootstrapped in
    neither mode, its neighbour that survives it is TRUNCATED."""
    track, n, H, K = "big_track", 16, 3, 64
    pre, near = Q.states(track, n, "pre_crash"), Q.states(track, n, "near_gate")
    s = {k: np.concatenate([np.asarray(pre[k]), np.asarray(near[k])]) for k in Q.STATE_KEYS + ("turns",)}
    table = Q.table(H, K)
    env = _env(track, n, "f64")
    agent, _ = _agent(n)
    for t0, steps_at_limit in ((998, 2), (999, 1)):
        rows = dict(s, time_step=np.full(len(s["px"]), t0, np.asarray(s["time_step"]).dtype))
        tr = V.trace(track, n, rows, table)
        st = tr["status"]
        assert (st == V.RUNNING).sum() == 0 and (st == V.TRUNCATED).sum() > 1000 and (st == V.TERMINATED).sum() > 1000
        assert (tr["steps"][st == V.TRUNCATED] == steps_at_limit).all()
        at_limit = (st == V.TERMINATED) & (tr["steps"] == steps_at_limit)      # crashed in the very step the limit fell due
        assert at_limit.sum() > 100
        value = _value(agent, tr["end_obs"])
        got = {}
        for mode in (V.BOOT_RUNNING, V.BOOT_RUNNING_TRUNCATED):
            got[mode] = _score(env, rows, table, gamma=0.99, mode=mode, agent=agent)
            _same(got[mode], _expected(tr, 0.99, mode, value), K22_KEYS + NEW_KEYS, (t0, mode))
        one, two = got[V.BOOT_RUNNING], got[V.BOOT_RUNNING_TRUNCATED]
        assert np.array_equal(_bits(one["ret"]), _bits(one["ret_env"]))      # mode 1: nothing runs on, nothing is bootstrapped
        trunc = st == V.TRUNCATED
        assert (two["ret"][trunc] != two["ret_env"][trunc]).mean() > 0.99      # mode 2: the lanes that ended at the limit
        assert np.array_equal(_bits(two["ret"][~trunc]), _bits(two["ret_env"][~trunc])) and at_limit[~trunc].sum() == at_limit.sum()
    env.close()


def test_an_agent_off_the_fused_menu_is_refused():
    env = _env("big_track", 16, "f32", 4)
    env.reset()
    table = _dev(Q.table(3, 9), torch.uint8)
    wide = pc.Agent(env.obs_dim, 9, hidden_size=128).cuda()      # the fused step takes 256 hidden units
    with pytest.raises(ValueError, match="menu"):
        env.score_sequences(table, gamma=0.99, bootstrap="running", agent=wide)
    other = pc.Agent(env.obs_dim + 1, 9).cuda()                   # on the menu, another obs dim than the handle's
    with pytest.raises(_capi.PpoCarError):
        env.score_sequences(table, gamma=0.99, bootstrap="running", agent=other)
    with pytest.raises(_capi.PpoCarError):
        env.score_sequences(table, gamma=0.99, bootstrap="running")      # a bootstrap without a policy
    with pytest.raises(ValueError, match="bootstrap"):
        env.score_sequences(table, gamma=0.99, bootstrap="sometimes", agent=_agent(16)[0])
    env.close()


# ---- 6. the planners with a critic ---------------------------------------------------------------------------------------------------------
PLAN_H, PLAN_K, PLAN_SEED, PLAN_ROUNDS, PLAN_GAMMA = 4, 64, 3, 20, 0.99


def _start_rows(track, n, N):
    pre, near = Q.states(track, n, "pre_crash"), Q.states(track, n, "near_gate")
    return {k: np.stack([np.asarray(pre[k][:N // 2]), np.asarray(near[k][:N // 2])], 1).reshape(-1) for k in Q.STATE_KEYS + ("turns",)}


def _critic_scorer(track, n, state, agent, gamma, mode):
    """cem_reference.plan's scoring callback: the oracle's trace, the policy step on its end observations, the combination"""
    def score(tables):
        tr = V.trace(track, n, state, tables)
        want = _expected(tr, gamma, mode, _value(agent, tr["end_obs"]))
        return want
    return score


def test_planner_with_a_critic_equals_the_oracle_driven_loop():
    track, n, N = "big_track", 16, 64
    s0 = _start_rows(track, n, N)
    s0 = {k: s0[k] for k in Q.STATE_KEYS}
    env = _env(track, n, "f64", N)
    env.reset()
    env.set_state(passed=0, **s0)
    orc = oracle.OracleVecEnv(R.track(track), N, n, reward_scaling=R.REWARD_SCALE)
    orc.reset()
    orc.set_state(passed=0, destroyed=0, **s0)
    agent, _ = _agent(n)
    planner = pc.Planner(env, horizon=PLAN_H, candidates=PLAN_K, seed=PLAN_SEED, agent=agent, gamma=PLAN_GAMMA, bootstrap="running")
    plain = pc.Planner(env, horizon=PLAN_H, candidates=PLAN_K, seed=PLAN_SEED)
    taken, done, differ = [], 0, 0
    for step in range(PLAN_ROUNDS):
        table, _ = Q.planner_draw(PLAN_H, PLAN_K, PLAN_SEED, step)
        differ += int((plain.act(step) != planner.act(step)).sum())      # (neither moves the envs)
        act = planner.act(step)
        assert np.array_equal(planner.table.cpu().numpy(), table), step
        state = {k: getattr(orc, k).copy() for k in Q.STATE_KEYS}
        want = _critic_scorer(track, n, state, agent, PLAN_GAMMA, V.BOOT_RUNNING)(table)
        got = {k: v.cpu().numpy() for k, v in planner.out.items()}
        _same(got, want, REQUIRED + Q.BEST_KEYS + ("end_obs", "end_value"), step)
        taken.append(got["best_action"].copy())
        _, _, term, trunc, _ = env.step(act)
        _, _, oterm, otrunc = orc.step(want["best_action"])
        assert np.array_equal(term.cpu().numpy() != 0, oterm) and np.array_equal(trunc.cpu().numpy() != 0, otrunc), step
        done += int(oterm.sum() + otrunc.sum())
    assert done > 0 and len({a.tobytes() for a in taken}) > 1 and differ > 0      # auto-resets included; the critic changes actions
    st = env.get_state()
    for k in Q.STATE_KEYS:
        assert np.array_equal(_bits(st[k]), _bits(getattr(orc, k).astype(st[k].dtype))), k
    env.close()


def test_cem_with_a_critic_equals_the_reference_loop():
    track, n, M, E, iters = "big_track", 16, 64, 8, 4
    s = _start_rows(track, n, M)
    agent, _ = _agent(n)
    ref = X.plan(X.uniform_weights(M, PLAN_H), _critic_scorer(track, n, s, agent, PLAN_GAMMA, V.BOOT_RUNNING), PLAN_K, E, iters, PLAN_SEED,
                 2 * iters)
    env = _env(track, n, "f64")
    planner = pc.CEMPlanner(env, horizon=PLAN_H, candidates=PLAN_K, elites=E, iterations=iters, seed=PLAN_SEED, agent=agent, gamma=PLAN_GAMMA,
                            bootstrap="running")
    t = _tensors(s, Q.table(1, 1))
    states = {k: t[k] for k in F64_KEYS + ("turns", "next_gate", "time_step")}
    planner.plan(2, states=states)      # step_index 2: offsets 8 .. 11
    got = {k: v.cpu().numpy() for k, v in planner.out.items()}
    _same(got, ref, REQUIRED + Q.BEST_KEYS + ("end_obs", "end_value"), "last round")
    assert np.array_equal(planner.weights.cpu().numpy().view(np.uint32), ref["weights"])
    assert np.array_equal(_bits(planner.iter_best_ret.cpu().numpy()), _bits(ref["iter_best_ret"]))
    assert np.array_equal(planner.table.cpu().numpy(), ref["tables"]) and np.array_equal(planner.best_seq.cpu().numpy(), ref["best_seq"])
    assert (np.diff(ref["iter_best_ret"], axis=0) >= 0).all()      # the kept sequence: a state's best never falls
    env.close()


def test_the_image_is_packed_once_per_act_and_once_per_plan(monkeypatch):
    track, n, N = "big_track", 16, 16
    env = _env(track, n, "f32", N)
    env.reset()
    agent, _ = _agent(n)
    packs = []
    real = agent.pack_policy
    monkeypatch.setattr(agent, "pack_policy", lambda: packs.append(1) or real())
    shooting = pc.Planner(env, horizon=4, candidates=16, seed=1, agent=agent, gamma=0.99, bootstrap="running")
    shooting.act(0)
    assert len(packs) == 1
    cem = pc.CEMPlanner(env, horizon=4, candidates=16, elites=4, iterations=3, seed=1, agent=agent, gamma=0.99, bootstrap="running_truncated")
    cem.plan(0)
    assert len(packs) == 2      # three rounds, one pack
    cem.act(1)
    assert len(packs) == 3
    # weights changed between two calls are seen by the second (the same table from the same state: the same end observations)
    shooting.act(0)
    before = shooting.out["end_value"].clone()
    with torch.no_grad():
        agent.critic[2].bias.add_(1.0)
    shooting.act(0)
    with torch.no_grad():
        agent.critic[2].bias.sub_(1.0)
    assert torch.allclose(shooting.out["end_value"], before + 1.0, atol=1e-4) and len(packs) == 5
    agent.pack_policy()
    env.close()


def test_planner_defaults_are_the_planners_of_before():
    track, n, N = "big_track", 16, 64
    s0 = {k: v for k, v in _start_rows(track, n, N).items() if k in Q.STATE_KEYS}
    env = _env(track, n, "f64", N)
    env.reset()
    env.set_state(passed=0, **s0)
    agent, _ = _agent(n)
    # shooting: the defaults against the oracle's K22 reference, as tests/test_sequences_gpu.py holds them; then gamma 1 through K25
    planner = pc.Planner(env, horizon=12, candidates=64, seed=3)
    assert planner._critic == {} and set(planner.out) == {"ret", "steps", "status", "best_k", "best_action", "best_ret"}
    planner.act(0)
    want = Q.rollout(track, n, s0, Q.planner_draw(12, 64, 3, 0)[0])
    got = {k: v.cpu().numpy() for k, v in planner.out.items()}
    _same(got, want, REQUIRED + Q.BEST_KEYS, "defaults")
    same = pc.Planner(env, horizon=12, candidates=64, seed=3, agent=agent, gamma=1.0, bootstrap="none")
    same.act(0)
    _same({k: v.cpu().numpy() for k, v in same.out.items()}, got, REQUIRED + Q.BEST_KEYS, "gamma 1 with an idle critic")
    # CEM: the defaults against cem_reference's loop on the oracle
    cem = pc.CEMPlanner(env, horizon=6, candidates=32, elites=4, iterations=2, seed=5)
    assert cem._critic == {} and set(cem.out) == set(planner.out)
    cem.plan(1)
    ref = X.plan(X.uniform_weights(N, 6), X.oracle_scorer(track, n, s0), 32, 4, 2, 5, 2)
    _same({k: v.cpu().numpy() for k, v in cem.out.items()}, ref, ("ret",) + Q.BEST_KEYS, "cem defaults")
    assert np.array_equal(cem.weights.cpu().numpy().view(np.uint32), ref["weights"])
    env.close()


def test_evaluate_planner_with_a_critic_end_to_end(capsys, tmp_path):
    import evaluate
    agent, _ = _agent(16)
    ckpt = str(tmp_path / "model.dat")
    torch.save(agent.state_dict(), ckpt)
    argv = ["--planner", "cem", "--plan-iterations", "2", "--plan-elites", "4", "--plan-horizon", "4", "--plan-candidates", "16", "--envs", "64",
            "--track", TRACKS["big_track"], "--num-rays", "16", "--plan-gamma", "0.99", "--plan-bootstrap", "running"]
    out = evaluate.main(argv + ["--checkpoint", ckpt])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    assert {k for k in out if k.startswith("eval/")} == set(EVAL_KEYS)
    assert out["eval/episodes"] == 64 and out["path"] == "planner"
    assert out["planner"] == {"kind": "cem", "horizon": 4, "candidates": 16, "iterations": 2, "elites": 4, "gamma": 0.99, "bootstrap": "running"}
    assert 0.0 <= out["eval/crash_rate"] <= 1.0 and 1.0 <= out["eval/episodic_length"] <= 1000.0
    with pytest.raises(SystemExit):      # a bootstrap needs the checkpoint's critic
        evaluate.main(argv)
    assert "--plan-bootstrap other than none needs --checkpoint" in capsys.readouterr().err
