"""K20 (pc_env_step_poses, VecCarEnv.step_poses) and PolicyLandscape.survival() / lookahead() on the GPU.

Held to pc_env_step bit for bit (F32 handles under both step forms, F64 handles), to the plain reference of step_poses_reference.py bit
for bit on F64 handles and within test_env_gpu.py's float32 bars on F32 handles; then the edges, chained in-place calls against
pc_env_step_many, the landscape's two consumers against a loop written here, and evaluate.py in a child process.

F32 handles against the reference: the rays within OBS_TOL_F32, the header within one float32 ulp, flags / reward / counters where the
nearest collision ray at the new pose is more than MARGIN_PX from its 10 px threshold.  The new position and velocity are float64 on
both sides and differ only through the heading's cosine and sine (the handle's 72-entry table of the exact multiples of 5 degrees
against the reference's running sum, a few ulps of the angle apart) times the 0.8 px thrust: they are held to STATE_TOL_PX = 1e-9 px,
a million times that difference and still far below anything a threshold test can see."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ppo_car_amd as pc
from conftest import ROOT, TRACKS
from oracle.scenarios import load_trained_policy, rot_after
from ppo_car_amd.landscape import grid_poses
from test_env_gpu import MARGIN_PX, OBS_TOL_F32
import observe_reference as OR
import step_poses_reference as R
import ray_counts_reference as rc

pytestmark = pytest.mark.gpu

STATE_TOL_PX = 1e-9
F64_KEYS = ("px", "py", "vx", "vy")
SENTINEL = {"obs": -7.5, "reward": -7.5, "terminated": 77, "truncated": 77, "gate": 77}


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _step(env, s, actions, track_id=None, active=None):
    """One step_poses call on copies of the numpy state s (px, py, vx, vy, turns, next_gate, time_step); every output is pre-filled with
    a sentinel.  Returns everything as numpy: the outputs and the state the call left in place."""
    M = len(actions)
    t = {k: _dev(s[k], torch.float64) for k in F64_KEYS}
    t.update({k: _dev(s[k], torch.int32) for k in ("turns", "next_gate", "time_step")})
    out = (torch.full((M, env.obs_dim), SENTINEL["obs"], device="cuda"), torch.full((M,), SENTINEL["reward"], device="cuda"),
           torch.full((M,), 77, dtype=torch.uint8, device="cuda"), torch.full((M,), 77, dtype=torch.uint8, device="cuda"),
           torch.full((M,), 77, dtype=torch.uint8, device="cuda"))
    r = env.step_poses(t["px"], t["py"], t["vx"], t["vy"], t["turns"], _dev(actions, torch.int64), next_gate=t["next_gate"],
                       time_step=t["time_step"], track_id=None if track_id is None else _dev(track_id, torch.uint8),
                       active=None if active is None else _dev(active, torch.uint8), out=out)
    assert r.obs is out[0] and r.next_gate is t["next_gate"] and r.time_step is t["time_step"]
    res = {k: getattr(r, k).cpu().numpy() for k in ("obs", "reward", "terminated", "truncated", "gate")}
    res.update({k: v.cpu().numpy() for k, v in t.items()})
    return res


def _same(a, b, keys, rows=slice(None)):
    for k in keys:
        assert np.array_equal(_bits(a[k])[rows], _bits(b[k])[rows]), k


ALL = ("obs", "reward", "terminated", "truncated", "gate", "px", "py", "vx", "vy", "turns", "next_gate", "time_step")


# ---- 1. the bits of pc_env_step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32-K1", "f32-K1f", "f64"])
@pytest.mark.parametrize("track,n", [("big_track", 16), ("track", 12)])
def test_bits_of_env_step(track, n, mode):
    N, T = 300, 40
    dtype = "f64" if mode == "f64" else "f32"
    env = pc.VecCarEnv(N, TRACKS[track], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype=dtype)
    if dtype == "f32":
        env.set_option("step_form", 1 if mode == "f32-K1" else 2)
    env.reset()
    start = R.track(track).start_rot
    rng = np.random.default_rng(11)
    actions = rng.integers(0, 9, size=(T, N))
    actions[rng.random((T, N)) < 0.4] = 0
    if dtype == "f64":      # env i only ever turns one way -- left for odd i, right for even i: its rotation stays on the one-way table
        odd = (np.arange(N) & 1).astype(bool)
        to_left, to_right = {3: 2, 5: 4, 7: 6}, {2: 3, 4: 5, 6: 7}
        for a, b in to_left.items():
            actions[:, odd] = np.where(actions[:, odd] == a, b, actions[:, odd])
        for a, b in to_right.items():
            actions[:, ~odd] = np.where(actions[:, ~odd] == a, b, actions[:, ~odd])
    fo = torch.zeros(N, env.obs_dim, device="cuda")
    n_term = n_alive = 0
    for t in range(T):
        st = env.get_state()
        s = {k: st[k] for k in F64_KEYS}
        s.update(turns=R.turns_of(st["rot"], start), next_gate=st["next_gate"], time_step=st["time_step"])
        if dtype == "f64":
            assert all(rot_after(start, int(k)) == r for k, r in zip(s["turns"], st["rot"])), t
        got = _step(env, s, actions[t])
        _, rew, term, trunc, _ = env.step(torch.from_numpy(actions[t]).cuda(), final_obs=fo)
        assert np.array_equal(_bits(got["obs"]), _bits(fo.cpu().numpy())), t
        assert np.array_equal(_bits(got["reward"]), _bits(rew.cpu().numpy())), t
        te, tr = term.cpu().numpy() != 0, trunc.cpu().numpy() != 0
        assert np.array_equal(got["terminated"], te.astype(np.uint8)) and np.array_equal(got["truncated"], tr.astype(np.uint8)), t
        after = env.get_state()
        run = ~(te | tr)
        for k in F64_KEYS:
            assert np.array_equal(_bits(got[k])[run], _bits(after[k])[run]), (t, k)
        assert np.array_equal(got["turns"][run], R.turns_of(after["rot"], start)[run]), t
        assert np.array_equal(got["next_gate"][run], after["next_gate"][run]) and np.array_equal(got["time_step"][run], after["time_step"][run]), t
        n_term += int(te.sum())
        n_alive += int(run.sum())
    assert n_term > 0 and n_alive > 0
    if dtype == "f32":
        assert env.last_step_kernel() == ("K1" if mode == "f32-K1" else "K1f")
    env.close()


# ---- 2. the bits of the reference ------------------------------------------------------------------------------------------------
_ref = {}


def _reference(track, n, recipe):
    """(state rows under all 9 actions, actions, the reference's step of them): computed once per config and recipe, never modified"""
    key = (track, n, recipe)
    if key not in _ref:
        rows, acts = R.all_actions(R.edge_states(track) if recipe == "edge" else R.near_gate_states(track))
        _ref[key] = (rows, acts, R.step(track, n, rows, acts))
    return _ref[key]


def _check_counts(track, n, recipe, c):
    """(the off-menu ray counts have no table of known counts: what the recipes are there for must still happen)"""
    if recipe == "edge":
        if (track, n) in R.EDGE_COUNTS:
            assert {k: c[k] for k in ("terminated", "truncated")} == R.EDGE_COUNTS[(track, n)]
        assert c["terminated"] > 0 and c["truncated"] > 0
    else:
        if (track, n) in R.NEAR_GATE_COUNTS:
            assert c == {k: 9 * v for k, v in R.NEAR_GATE_COUNTS[(track, n)].items()}
        assert c["gates"] > 0 and c["laps"] > 0 and c["truncated"] > 0


OFF_MENU = [(rc.TRACK_OF[n], n) for n in (5, 7, 11, 90, 181)]      # tests/ray_counts_reference.py


@pytest.mark.parametrize("recipe", ["edge", "near_gate"])
@pytest.mark.parametrize("track,n", R.CONFIGS)
def test_f64_bits_of_the_reference(track, n, recipe):
    _f64_bits_of_the_reference(track, n, recipe)


@pytest.mark.parametrize("recipe", ["edge", "near_gate"])
@pytest.mark.parametrize("track,n", OFF_MENU)
def test_off_menu_ray_counts_f64_bits_of_the_reference(track, n, recipe):
    _f64_bits_of_the_reference(track, n, recipe)


def _f64_bits_of_the_reference(track, n, recipe):
    rows, acts, ref = _reference(track, n, recipe)
    env = pc.VecCarEnv(1, TRACKS[track], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype="f64")
    got = _step(env, rows, acts)
    assert np.array_equal(_bits(got["obs"]), _bits(ref["obs"]))
    assert np.array_equal(_bits(got["reward"]), _bits(ref["reward"]))
    for k in ("terminated", "truncated", "gate"):
        assert np.array_equal(got[k] != 0, ref[k]) and set(np.unique(got[k])) <= {0, 1}, k
    assert np.array_equal(got["next_gate"], ref["next_gate"]) and np.array_equal(got["time_step"], ref["time_step"])
    for k in F64_KEYS:
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    left, right = np.isin(acts, (2, 4, 6)), np.isin(acts, (3, 5, 7))
    assert np.array_equal(got["turns"], rows["turns"] + right.astype(np.int32) - left.astype(np.int32))
    c = R.counts({k: got[k] != 0 for k in ("gate", "terminated", "truncated")}, got["next_gate"])
    assert c == R.counts(ref, ref["next_gate"])
    _check_counts(track, n, recipe, c)
    env.close()


@pytest.mark.parametrize("recipe", ["edge", "near_gate"])
@pytest.mark.parametrize("track,n", R.CONFIGS)
def test_f32_against_the_reference(track, n, recipe):
    _f32_against_the_reference(track, n, recipe)


@pytest.mark.parametrize("recipe", ["edge", "near_gate"])
@pytest.mark.parametrize("track,n", OFF_MENU)
def test_off_menu_ray_counts_f32_against_the_reference(track, n, recipe):
    _f32_against_the_reference(track, n, recipe)


def _f32_against_the_reference(track, n, recipe):
    rows, acts, ref = _reference(track, n, recipe)
    env = pc.VecCarEnv(1, TRACKS[track], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype="f32")
    got = _step(env, rows, acts)
    walls = R.track(track).walls
    print("f32 max ray error", float(np.abs(got["obs"][:, 6:] - ref["obs"][:, 6:]).max()))
    assert np.abs(got["obs"][:, 6:] - ref["obs"][:, 6:]).max() <= OBS_TOL_F32
    diff = np.abs(got["obs"][:, :6] - ref["obs"][:, :6])
    assert (diff <= np.spacing(np.maximum(np.abs(ref["obs"][:, :6]), np.float32(1e-6)))).all(), diff.max()
    for k in F64_KEYS:
        print("f32 max state difference", k, float(np.abs(got[k] - ref[k]).max()))
        assert np.abs(got[k] - ref[k]).max() <= STATE_TOL_PX, k
    margin = np.array([OR.collision_margin(float(x), float(y), float(r), n, walls) for x, y, r in zip(ref["px"], ref["py"], ref["rot"])])
    ok = margin > MARGIN_PX
    print("rows left out", int((~ok).sum()), "of", len(ok))
    assert (~ok).sum() <= 0.01 * len(ok)
    for k in ("terminated", "truncated", "gate"):
        assert np.array_equal(got[k][ok] != 0, ref[k][ok]), k
    assert np.array_equal(_bits(got["reward"])[ok], _bits(ref["reward"])[ok])
    assert np.array_equal(got["next_gate"][ok], ref["next_gate"][ok]) and np.array_equal(got["time_step"], ref["time_step"])
    c = R.counts({k: (got[k] != 0)[ok] for k in ("gate", "terminated", "truncated")}, got["next_gate"][ok])
    assert c == R.counts({k: ref[k][ok] for k in ("gate", "terminated", "truncated")}, ref["next_gate"][ok])
    if recipe == "edge":
        assert ref["terminated"][ok].any()      # the kept rows include terminations
    if ok.all():
        _check_counts(track, n, recipe, c)
    env.close()


# ---- 3. edges --------------------------------------------------------------------------------------------------------------------
def _edge_rows(track, n, M=257):
    """M rows that crash, truncate, pass gates and close laps: the two recipes interleaved, under mixed actions"""
    e, g = R.edge_states(track), R.near_gate_states(track)
    s = {k: np.concatenate([e[k][:M - M // 2], g[k][:M // 2]]) for k in F64_KEYS + ("turns", "next_gate", "time_step")}
    perm = np.random.default_rng(3).permutation(M)
    return {k: v[perm] for k, v in s.items()}, (np.arange(M) * 5 + 3) % 9


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_edges_one_row_inactive_rows_bad_actions_bad_gates_repeat(dtype):
    track, n = "big_track", 16
    t = R.track(track)
    env = pc.VecCarEnv(3, TRACKS[track], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype=dtype)
    env.reset()
    env.step(torch.zeros(3, dtype=torch.int64, device="cuda"))
    before = env.get_state()
    s, acts = _edge_rows(track, n)
    M = len(acts)
    full = _step(env, s, acts)
    assert full["terminated"].any() and full["truncated"].any() and full["gate"].any() and (full["gate"] & (full["next_gate"] == 0)).any()
    assert set(np.unique(full["terminated"])) | set(np.unique(full["truncated"])) | set(np.unique(full["gate"])) <= {0, 1}
    # M = 1 equals row 5 of the larger call
    one = _step(env, {k: v[5:6] for k, v in s.items()}, acts[5:6])
    _same(one, {k: v[5:6] for k, v in full.items()}, ALL)
    # two identical calls give identical bits, and so does every lane count per row
    _same(_step(env, s, acts), full, ALL)
    for lanes in (1, 4, 16):
        env.set_lanes_per_env(lanes)
        _same(_step(env, s, acts), full, ALL)
    env.set_lanes_per_env(0)
    # inactive rows keep every byte of every array; the active ones are the full call's
    active = (np.arange(M) % 3 != 1).astype(np.uint8)
    part = _step(env, s, acts, active=active)
    on = active != 0
    _same(part, full, ALL, on)
    for k in F64_KEYS + ("turns", "next_gate", "time_step"):
        assert np.array_equal(_bits(part[k])[~on], _bits(np.asarray(s[k], part[k].dtype))[~on]), k
    assert (part["obs"][~on] == np.float32(SENTINEL["obs"])).all() and (part["reward"][~on] == np.float32(SENTINEL["reward"])).all()
    for k in ("terminated", "truncated", "gate"):
        assert (part[k][~on] == 77).all(), k
    # actions outside 0 .. 8 act as 8
    for bad in (-3, 9, 1 << 40):
        _same(_step(env, s, np.full(M, bad, np.int64)), _step(env, s, np.full(M, 8, np.int64)), ALL)
    # next_gate = G and -1: no gate can fire, the value is kept; everything else is the row's with its real gate not firing
    near = R.near_gate_states(track)
    near = {k: near[k] for k in s}
    hit = _step(env, near, np.zeros(240, np.int64))
    assert hit["gate"].sum() == R.NEAR_GATE_COUNTS[(track, n)]["gates"]
    for bad in (t.G, -1, 1 << 20, -(1 << 31)):
        off = dict(near, next_gate=np.full(240, bad, np.int64))
        got = _step(env, off, np.zeros(240, np.int64))
        assert not got["gate"].any() and (got["next_gate"] == bad).all()
        _same(got, hit, ("obs", "terminated", "truncated", "px", "py", "vx", "vy", "turns", "time_step"))
        assert (got["reward"] == np.float32(0.01 * R.REWARD_SCALE)).all()
    # the poses (-50, -50) and (2000, 900), at rest, against the reference
    out_s = dict(px=np.array([-50.0, 2000.0]), py=np.array([-50.0, 900.0]), vx=np.zeros(2), vy=np.zeros(2), turns=np.array([3, -7], np.int32),
                 next_gate=np.zeros(2, np.int64), time_step=np.array([5, 999]))
    got = _step(env, out_s, np.array([8, 8]))
    ref = R.step(track, n, dict(out_s, rot=np.array([rot_after(t.start_rot, 3), rot_after(t.start_rot, -7)])), np.array([8, 8]))
    assert not ref["terminated"].any() and list(ref["truncated"]) == [False, True] and (ref["obs"][1, 6:] == 1.0).all()
    for k in ("terminated", "truncated", "gate"):
        assert np.array_equal(got[k] != 0, ref[k]), k
    assert np.array_equal(_bits(got["reward"]), _bits(ref["reward"])) and np.array_equal(got["time_step"], ref["time_step"])
    if dtype == "f64":
        assert np.array_equal(_bits(got["obs"]), _bits(ref["obs"]))
    else:
        assert np.abs(got["obs"][:, 6:] - ref["obs"][:, 6:]).max() <= OBS_TOL_F32
        assert (np.abs(got["obs"][:, :6] - ref["obs"][:, :6]) <= np.spacing(np.maximum(np.abs(ref["obs"][:, :6]), np.float32(1e-6)))).all()
    # the handle's own state is neither read nor written
    after = env.get_state()
    for k in before:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k
    env.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_edges_two_tracks_in_one_wave_and_unknown_track(dtype):
    n = 16
    s, acts = _edge_rows("big_track", n)
    M = len(acts)
    singles = []
    for track in ("track", "big_track"):
        env = pc.VecCarEnv(1, TRACKS[track], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype=dtype)
        singles.append(_step(env, s, acts))
        env.close()
    env = pc.VecCarEnv(2, [TRACKS["track"], TRACKS["big_track"]], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype=dtype,
                       track_id=np.array([0, 1], np.uint8))
    tid = (np.arange(M) & 1).astype(np.uint8)
    both = _step(env, s, acts, track_id=tid)
    for k in (0, 1):
        _same(both, singles[k], ALL, tid == k)
    assert not np.array_equal(_bits(both["obs"][0::2]), _bits(singles[1]["obs"][0::2]))      # (the two tracks do differ)
    # an id the handle does not have: zeros and flags 0, the state untouched; its neighbours are the rows of the call above
    tid2 = tid.copy()
    tid2[[0, 100, 256]] = (2, 255, 7)
    got = _step(env, s, acts, track_id=tid2)
    bad = tid2 >= 2
    assert (_bits(got["obs"][bad]) == 0).all() and (_bits(got["reward"][bad]) == 0).all()
    for k in ("terminated", "truncated", "gate"):
        assert (got[k][bad] == 0).all(), k
    for k in F64_KEYS + ("turns", "next_gate", "time_step"):
        assert np.array_equal(_bits(got[k])[bad], _bits(np.asarray(s[k], got[k].dtype))[bad]), k
    _same(got, both, ALL, ~bad)
    # ... and with inactive rows among them
    active = (np.arange(M) % 4 != 0).astype(np.uint8)
    part = _step(env, s, acts, track_id=tid2, active=active)
    on = active != 0
    _same(part, got, ALL, on)
    assert (part["obs"][~on] == np.float32(SENTINEL["obs"])).all() and (part["terminated"][~on] == 77).all()
    env.close()


# ---- 4. chained in-place calls against pc_env_step_many --------------------------------------------------------------------------
@pytest.mark.parametrize("track,n", [("big_track", 16), ("track", 12)])
def test_f32_chained_calls_equal_step_many(track, n):
    N, T = 257, 30
    env = pc.VecCarEnv(N, TRACKS[track], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype="f32")
    env.reset()
    st = env.get_state()
    rng = np.random.default_rng(17)
    actions = rng.integers(0, 9, size=(T, N))
    actions[rng.random((T, N)) < 0.4] = 0
    acts = torch.from_numpy(actions).cuda()
    px, py, vx, vy = (_dev(st[k], torch.float64) for k in F64_KEYS)
    turns = _dev(R.turns_of(st["rot"], R.track(track).start_rot), torch.int32)
    next_gate, time_step = _dev(st["next_gate"], torch.int32), _dev(st["time_step"], torch.int32)
    rows = []
    for t in range(T):
        r = env.step_poses(px, py, vx, vy, turns, acts[t], next_gate=next_gate, time_step=time_step)
        rows.append([x.clone() for x in (r.obs, r.reward, r.terminated, r.truncated)])
    obs, rew, term, trunc = env.step_many(acts)
    running = torch.ones(N, dtype=torch.bool, device="cuda")
    compared = 0
    for t in range(T):
        done = (term[t] != 0) | (trunc[t] != 0)
        live = running & ~done      # every env up to the step before its first done
        o, r, te, tr = rows[t]
        assert torch.equal(o[live].view(torch.int32), obs[t][live].view(torch.int32)), t
        assert torch.equal(r[live].view(torch.int32), rew[t][live].view(torch.int32)), t
        assert not te[live].any() and not tr[live].any(), t
        first = running & done      # (its first done itself: the flags and the reward agree; the observation is the reset's there)
        assert torch.equal(te[first] != 0, term[t][first] != 0) and torch.equal(r[first].view(torch.int32), rew[t][first].view(torch.int32)), t
        compared += int(live.sum())
        running = live
    assert compared > N * T // 4
    env.close()


# ---- 5. the landscape's consumers against a loop written here --------------------------------------------------------------------
@pytest.fixture(scope="module")
def landscape():
    agent = pc.Agent(23, 9)
    load_trained_policy(agent)
    agent = agent.cuda()
    ls = pc.PolicyLandscape(agent, TRACKS["big_track"], 16, cell_px=80, speed=0.5, dtype="f32", device="cuda")
    yield ls
    ls.close()


def test_survival_and_lookahead_equal_a_plain_loop(landscape):
    ls, H = landscape, 8
    assert ls.poses_per_track == 10368
    with pytest.raises(RuntimeError):
        pc.PolicyLandscape(ls.agent, None, 16, cell_px=80, device="cuda", envs=ls.envs).lookahead()
    ls.compute().survival(H).lookahead()
    env, agent = ls.envs, ls.agent
    # survival
    px, py, vx, vy, turns, tid = (t.clone() for t in ls.poses())
    M = px.numel()
    col = torch.empty(M, dtype=torch.uint8, device="cuda")
    obs = env.observe_poses(px, py, turns, vx=vx, vy=vy, track_id=tid, collides=col)
    alive = col == 0
    ng, ts = torch.zeros(M, dtype=torch.int32, device="cuda"), torch.zeros(M, dtype=torch.int32, device="cuda")
    want = torch.zeros(M, dtype=torch.int16, device="cuda")
    for _ in range(H):
        act, _, _ = agent.act(obs, greedy=True)
        r = env.step_poses(px, py, vx, vy, turns, act, next_gate=ng, time_step=ts, track_id=tid, active=alive.to(torch.uint8))
        obs = torch.where(alive[:, None], r.obs, obs)
        alive = alive & (r.terminated == 0)
        want += alive
    assert ls.survived.dtype == torch.int16 and ls.survived.shape == (1, 72, 9, 16) and ls.survival_horizon == H
    assert torch.equal(ls.survived.view(-1), want)
    drivable = ls.drivable.view(-1)
    assert torch.equal(drivable, col == 0)
    assert not ls.survived.view(-1)[~drivable].any()      # 0 where the pose is not drivable ...
    assert (want == H).any() and (want[drivable] < H).any()      # ... some pose drives all 8 steps, some drivable pose does not
    # look-ahead
    safe = torch.zeros(M, dtype=torch.uint8, device="cuda")
    crash = torch.zeros(M, dtype=torch.bool, device="cuda")
    greedy = ls.action.view(-1).to(torch.int64)
    for a in range(9):
        p = [t.clone() for t in ls.poses()]
        r = env.step_poses(p[0], p[1], p[2], p[3], p[4], torch.full((M,), a, dtype=torch.int64, device="cuda"), track_id=p[5])
        safe += (drivable & (r.terminated == 0)).to(torch.uint8)
        crash |= drivable & (r.terminated != 0) & (greedy == a)
    assert torch.equal(ls.safe_actions.view(-1), safe) and ls.safe_actions.dtype == torch.uint8
    assert torch.equal(ls.greedy_crashes.view(-1), crash) and torch.equal(ls.avoidable.view(-1), crash & (safe > 0))
    assert not ls.safe_actions.view(-1)[~drivable].any() and (safe == 9).any()
    # the landscape's grid poses are where they were: its calls stepped clones
    for a, b in zip(ls.poses()[:5], grid_poses(ls.tracks[0].start_angle, ls.cell_px, ls.speed)):
        assert torch.equal(a.cpu(), torch.from_numpy(b))


# ---- 6. evaluate.py in a fresh child process ---------------------------------------------------------------------------------------
def test_evaluate_landscape_options(tmp_path):
    agent = pc.Agent(23, 9)
    load_trained_policy(agent)
    torch.save(agent.state_dict(), tmp_path / "model.dat")
    base = [sys.executable, os.path.join(ROOT, "evaluate.py"), "--checkpoint", str(tmp_path / "model.dat"), "--track", TRACKS["big_track"],
            "--num-rays", "16", "--landscape-cell", "80"]
    outs = {}
    for name, extra in (("plain", []), ("more", ["--landscape-horizon", "8", "--landscape-lookahead"])):
        r = subprocess.run(base + ["--landscape", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[name] = json.loads(r.stdout.strip().splitlines()[-1])
    old_keys = {"value", "action", "drivable", "best_value", "best_heading", "action_at_best", "cell_px", "speed", "tracks"}
    plain = np.load(str(tmp_path / "plain_landscape.npz"))
    assert set(plain.files) == old_keys      # with the options off: the keys and the files of before
    assert set(outs["plain"]) == {"landscape", "cells", "drivable_cells", "poses", "drivable_poses"}
    assert sorted(os.listdir(tmp_path)) == sorted(["model.dat", "plain_landscape.npz", "plain_landscape_big_track.png", "more_landscape.npz",
                                                   "more_landscape_big_track.png", "more_survival_big_track.png"])
    more = np.load(str(tmp_path / "more_landscape.npz"))
    assert set(more.files) == old_keys | {"survived", "safe_actions", "greedy_crashes", "avoidable", "survival_horizon"}
    for k in old_keys - {"tracks"}:
        assert np.array_equal(more[k], plain[k], equal_nan=True), k
    out = outs["more"]
    assert set(out) == set(outs["plain"]) | {"survival_horizon", "cells_surviving", "avoidable_poses"}
    assert out["survival_horizon"] == 8 and int(more["survival_horizon"]) == 8
    assert out["cells_surviving"] == int((more["survived"].max(1) >= 8).sum()) and 0 < out["cells_surviving"] <= out["drivable_cells"]
    assert out["avoidable_poses"] == int(more["avoidable"].sum())
    assert more["survived"].shape == (1, 72, 9, 16) and more["survived"].dtype == np.int16 and more["safe_actions"].dtype == np.uint8
    assert os.path.getsize(tmp_path / "more_survival_big_track.png") > 0
    assert out["landscape"][-1].endswith("more_survival_big_track.png")
