"""K17 (pc_env_observe_poses / pc_env_observe) and the policy landscape on the GPU.

F64 handles are held to the golden files' observations bit for bit, F32 handles to pc_env_step bit for bit and to the reference
within test_env_gpu.py's float32 bars; then the edges (one pose, poses outside the track, NULL velocities, two tracks in one wave,
an unknown track id), the landscape against act(observe_poses()), and training with and without the landscape.

The poses (-50, -50) and (2000, 900): from (2000, 900) every ray reports 1.0 (nothing within 1000 px), and so says the reference.
From (-50, -50) the reference itself reports rays that reach the track (big_track: the nearest 314 px away), so "every ray 1.0"
cannot hold there; the kernel is held to the reference at both poses, and neither collides."""
import os

import numpy as np
import pytest
import torch

import oracle
import ppo_car_amd as pc
from conftest import TRACKS
from oracle.scenarios import load_trained_policy
from test_env_gpu import MARGIN_PX, OBS_TOL_F32
import observe_reference as R
import ray_counts_reference as rc

pytestmark = pytest.mark.gpu


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _observe(env, px, py, turns, vx=None, vy=None, track_id=None):
    M = len(px)
    col = torch.full((M,), 7, dtype=torch.uint8, device="cuda")
    obs = env.observe_poses(_dev(px, torch.float64), _dev(py, torch.float64), _dev(turns, torch.int32),
                            vx=None if vx is None else _dev(vx, torch.float64), vy=None if vy is None else _dev(vy, torch.float64),
                            track_id=None if track_id is None else _dev(track_id, torch.uint8), collides=col)
    return obs.cpu().numpy(), col.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_f32(obs, col, ref_obs, ref_col, margin_ok):
    """test_env_gpu.py's bars for an F32 handle: rays within OBS_TOL_F32, header within one float32 ulp, collides where the margin allows"""
    print("f32 max ray error", float(np.abs(obs[:, 6:] - ref_obs[:, 6:]).max()))
    assert np.abs(obs[:, 6:] - ref_obs[:, 6:]).max() <= OBS_TOL_F32
    diff = np.abs(obs[:, :6] - ref_obs[:, :6])
    assert (diff <= np.spacing(np.maximum(np.abs(ref_obs[:, :6]), np.float32(1e-6)))).all(), diff.max()
    assert np.array_equal(col[margin_ok] != 0, ref_col[margin_ok])


# ---- 1. F64 handles, bit for bit against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("track,n", R.CONFIGS)
def test_f64_poses_equal_reference_bits(track, n):
    g = R.golden_rows(track, n)
    env = pc.VecCarEnv(1, TRACKS[track], num_rays=n, dtype="f64")
    obs, col = _observe(env, g["px"], g["py"], g["turns"], g["vx"], g["vy"])
    assert obs.shape == g["obs"].shape
    assert np.array_equal(_bits(obs), _bits(g["obs"]))
    assert np.array_equal(col != 0, g["terminated"]) and set(np.unique(col)) <= {0, 1}
    assert g["terminated"].any() and not g["terminated"].all()
    env.close()


# ---- 2. pc_env_observe on the current state --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("track,n", R.CONFIGS)
def test_observe_current_state(track, n, dtype):
    g = R.golden_rows(track, n)
    M = len(g["px"])
    env = pc.VecCarEnv(M, TRACKS[track], num_rays=n, dtype=dtype)
    env.reset()
    env.set_state(px=g["px"], py=g["py"], vx=g["vx"], vy=g["vy"], rot=g["rot"], time_step=np.arange(M) % 900 + 1)
    before = env.get_state()
    col = torch.full((M,), 7, dtype=torch.uint8, device="cuda")
    obs = env.observe(collides=col).cpu().numpy()
    after = env.get_state()
    for k in before:
        assert np.array_equal(before[k].view(np.uint64) if before[k].dtype == np.float64 else before[k],
                              after[k].view(np.uint64) if after[k].dtype == np.float64 else after[k]), k
    obs_p, col_p = _observe(env, g["px"], g["py"], g["turns"], g["vx"], g["vy"])
    assert np.array_equal(_bits(obs), _bits(obs_p)) and np.array_equal(col.cpu().numpy(), col_p)
    if dtype == "f64":
        assert np.array_equal(_bits(obs), _bits(g["obs"]))
    env.close()


# ---- 3. F32 handles, bit for bit against pc_env_step -----------------------------------------------------------------------------
@pytest.mark.parametrize("step_form", [1, 2])
@pytest.mark.parametrize("track,n", [("big_track", 16), ("track", 12)])
def test_f32_observe_equals_step_bits(track, n, step_form):
    N, T = 300, 40
    env = pc.VecCarEnv(N, TRACKS[track], num_rays=n, reward_scaling=0.1, dtype="f32")
    env.set_option("step_form", step_form)
    env.reset()
    rng = np.random.default_rng(11)
    actions = rng.integers(0, 9, size=(T, N))
    actions[rng.random((T, N)) < 0.4] = 0
    resets = 0
    for t in range(T):
        obs, rew, term, trunc, _ = env.step(torch.from_numpy(actions[t]).cuda())
        seen = env.observe()
        assert torch.equal(obs.view(torch.int32), seen.view(torch.int32)), t
        resets += int(term.sum())
    assert resets > 0      # envs that were auto-reset show the reset observation
    assert env.last_step_kernel() == ("K1" if step_form == 1 else "K1f")
    env.close()


# ---- 4. F32 handles against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("track,n", R.CONFIGS)
def test_f32_poses_against_reference(track, n):
    g = R.golden_rows(track, n)
    env = pc.VecCarEnv(1, TRACKS[track], num_rays=n, dtype="f32")
    obs, col = _observe(env, g["px"], g["py"], g["turns"], g["vx"], g["vy"])
    _check_f32(obs, col, g["obs"], g["terminated"], g["wall_margin"] > MARGIN_PX)
    env.close()


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------
def _edge_poses(track, n):
    g = R.golden_rows(track, n)
    return g["px"][:257].copy(), g["py"][:257].copy(), g["vx"][:257].copy(), g["vy"][:257].copy(), g["turns"][:257].copy()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_edges_one_pose_outside_null_velocity_repeat(dtype):
    track, n = "big_track", 16
    g = R.golden_rows(track, n)
    env = pc.VecCarEnv(3, TRACKS[track], num_rays=n, dtype=dtype)
    px, py, vx, vy, turns = _edge_poses(track, n)
    full, full_col = _observe(env, px, py, turns, vx, vy)
    # M = 1
    one, one_col = _observe(env, px[5:6], py[5:6], turns[5:6], vx[5:6], vy[5:6])
    assert np.array_equal(_bits(one[0]), _bits(full[5])) and one_col[0] == full_col[5]
    # outside the track
    ox, oy, ot = np.array([-50.0, 2000.0]), np.array([-50.0, 900.0]), np.array([3, -7], np.int32)
    out, out_col = _observe(env, ox, oy, ot)
    rot = [oracle.scenarios.rot_after(g["start_rot"], int(t)) for t in ot]
    ref, ref_col = R.observe_many(ox, oy, [0.0, 0.0], [0.0, 0.0], rot, n, g["walls"])
    assert not ref_col.any() and not out_col.any()
    assert (ref[1, 6:] == 1.0).all() and (out[1, 6:] == 1.0).all()
    if dtype == "f64":
        assert np.array_equal(_bits(out), _bits(ref))
    else:
        _check_f32(out, out_col, ref, ref_col, np.ones(2, bool))
    # vx / vy NULL = 0
    nov, nov_col = _observe(env, px, py, turns)
    assert (nov[:, 2:4] == 0).all() and np.array_equal(_bits(np.delete(nov, [2, 3], 1)), _bits(np.delete(full, [2, 3], 1)))
    assert np.array_equal(nov_col, full_col)
    # two calls give identical bytes, and so does every lane count per pose
    again, again_col = _observe(env, px, py, turns, vx, vy)
    assert np.array_equal(_bits(again), _bits(full)) and np.array_equal(again_col, full_col)
    for lanes in (1, 4, 16):
        env.set_lanes_per_env(lanes)
        o, c = _observe(env, px, py, turns, vx, vy)
        assert np.array_equal(_bits(o), _bits(full)) and np.array_equal(c, full_col), lanes
    env.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_edges_two_tracks_in_one_wave_and_unknown_track(dtype):
    n, M = 16, 257
    px, py, vx, vy, turns = _edge_poses("big_track", n)
    singles = []
    for track in ("track", "big_track"):
        env = pc.VecCarEnv(1, TRACKS[track], num_rays=n, dtype=dtype)
        singles.append(_observe(env, px, py, turns, vx, vy))
        env.close()
    env = pc.VecCarEnv(2, [TRACKS["track"], TRACKS["big_track"]], num_rays=n, dtype=dtype, track_id=np.array([0, 1], np.uint8))
    tid = (np.arange(M) & 1).astype(np.uint8)
    obs, col = _observe(env, px, py, turns, vx, vy, track_id=tid)
    for k in (0, 1):
        assert np.array_equal(_bits(obs[tid == k]), _bits(singles[k][0][tid == k])), k
        assert np.array_equal(col[tid == k], singles[k][1][tid == k]), k
    assert not np.array_equal(_bits(obs[0::2]), _bits(singles[1][0][0::2]))      # (the two tracks do differ)
    # an id the handle does not have: a zero row, collides 0; its neighbours are untouched
    tid2 = tid.copy()
    tid2[[0, 100, 256]] = (2, 255, 7)
    obs2, col2 = _observe(env, px, py, turns, vx, vy, track_id=tid2)
    bad = tid2 >= 2
    assert (_bits(obs2[bad]) == 0).all() and (col2[bad] == 0).all()
    assert np.array_equal(_bits(obs2[~bad]), _bits(obs[~bad])) and np.array_equal(col2[~bad], col[~bad])
    env.close()


# ---- 6. landscape ----------------------------------------------------------------------------------------------------------------
def test_landscape_equals_act_on_observed_poses():
    n, cell = 16, 80
    agent = pc.Agent(23, 9)
    load_trained_policy(agent)
    agent = agent.cuda()
    ls = pc.PolicyLandscape(agent, TRACKS["big_track"], n, cell_px=cell, speed=0.5, dtype="f32", device="cuda")
    assert ls.grid == (9, 16) and ls.poses_per_track == 10368
    ls.compute()
    px, py, vx, vy, turns, tid = ls.poses()
    col = torch.empty(10368, dtype=torch.uint8, device="cuda")
    obs = ls.envs.observe_poses(px, py, turns, vx=vx, vy=vy, track_id=tid, collides=col)
    act, _, val = agent.act(obs, greedy=True)
    assert torch.equal(ls.value.view(-1).view(torch.int32), val.view(torch.int32))
    assert torch.equal(ls.action.view(-1), act.to(torch.uint8)) and int(act.max()) <= 8
    assert torch.equal(ls.drivable.view(-1), col == 0)
    # one heading against the reference
    g = R.golden_rows("big_track", n)
    t = 17
    sl = slice(t * 144, (t + 1) * 144)
    rot = oracle.scenarios.rot_after(g["start_rot"], t)
    ref, ref_col = R.observe_many(px[sl].cpu().numpy(), py[sl].cpu().numpy(), vx[sl].cpu().numpy(), vy[sl].cpu().numpy(), [rot] * 144, n, g["walls"])
    margin = np.array([R.collision_margin(float(x), float(y), rot, n, g["walls"]) for x, y in zip(px[sl].cpu().numpy(), py[sl].cpu().numpy())])
    ok = margin > MARGIN_PX
    _check_f32(obs[sl].cpu().numpy(), col[sl].cpu().numpy(), ref, ref_col, ok)
    assert ok.all() and ref_col.any() and not ref_col.all()
    assert np.array_equal(ls.drivable[0, t].cpu().numpy().reshape(-1), ~ref_col)
    # the cell holding the start line is drivable at turn 0; and the reductions say something
    tr = ls.tracks[0]
    assert bool(ls.drivable[0, 0, int(tr.start_y // cell), int(tr.start_x // cell)])
    best = ls.best_value().cpu().numpy()
    assert np.array_equal(np.isnan(best), ~ls.drivable[0].any(0).cpu().numpy()) and np.isfinite(best).sum() > 10
    ls.close()


# ---- 7. training computes the same bits with the landscape on or off -------------------------------------------------------------
def test_training_bits_with_and_without_landscape(tmp_path):
    import glob
    import sys
    from conftest import ROOT
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import train
    models = []
    for name, extra in (("off", []), ("on", ["--landscape-every", "1", "--landscape-cell", "80"])):
        out = str(tmp_path / name)
        train.main(["--run-name", name, "--cuda", "--n-envs", "16", "--n-steps", "64", "--n-epochs", "2", "--batch-size", "64", "--train-iters", "4",
                    "--num-rays", "16", "--track", TRACKS["big_track"], "--out-dir", out] + extra)
        (model,) = glob.glob(os.path.join(out, "checkpoints", "*", "model.dat"))
        models.append(torch.load(model, map_location="cpu"))
        written = glob.glob(os.path.join(out, "checkpoints", "*", "landscape_*"))
        assert len(written) == (4 if extra else 0), written      # two epochs x (npz + one PNG)
    assert models[0].keys() == models[1].keys()
    for k in models[0]:
        assert torch.equal(models[0][k].view(torch.int32), models[1][k].view(torch.int32)), k


# ---- 9. the off-menu ray counts (tests/ray_counts_reference.py): the harvested oracle states in the golden rows' place ---------------------
OFF_MENU = [(rc.TRACK_OF[n], n) for n in (5, 7, 11, 90, 181)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("track,n", OFF_MENU)
def test_off_menu_ray_counts_against_the_reference(track, n, dtype):
    """The poses the harvested steps end at, with the oracle's observation of them and whether they crashed: F64 handles give the
    reference's bits, F32 handles stay within test_env_gpu.py's bars.  At 181 nominal rays the first rows are the recorded crashes of a
    reversing car, which only rays 135 / 180 -- past the 64-bit collision mask -- see."""
    g = rc.harvest(track, n)
    turns = np.rint((g["post_rot"] - g["reset_state"][4]) / 5.0).astype(np.int32)
    env = pc.VecCarEnv(1, TRACKS[track], num_rays=n, dtype=dtype)
    obs, col = _observe(env, g["post_px"], g["post_py"], turns, g["post_vx"], g["post_vy"])
    assert obs.shape == g["step_obs"].shape == (len(turns), 6 + rc.geometry(n)[1]) and set(np.unique(col)) <= {0, 1}
    assert g["terminated"].sum() >= 100 and (~g["terminated"]).sum() >= 100
    if dtype == "f64":
        assert np.array_equal(_bits(obs), _bits(g["step_obs"]))
        assert np.array_equal(col != 0, g["terminated"])
    else:
        _check_f32(obs, col, g["step_obs"], g["terminated"], g["wall_margin"] > MARGIN_PX)
        assert (g["wall_margin"] > MARGIN_PX).mean() > 0.99
    if n == 181:
        k = g["n_high_ray_only"]
        assert k >= 5 and rc.high_ray_only_crashes(g, track, n)[:k].all() and (g["wall_margin"][:k] > MARGIN_PX).all()
        assert (col[:k] == 1).all()
    env.close()


@pytest.mark.parametrize("track,n", OFF_MENU)
def test_off_menu_ray_counts_f32_observe_equals_step_bits(track, n):
    N, T = 300, 40
    env = pc.VecCarEnv(N, TRACKS[track], num_rays=n, reward_scaling=0.1, dtype="f32")
    env.reset()
    rng = np.random.default_rng(11)
    actions = rng.integers(0, 9, size=(T, N))
    actions[rng.random((T, N)) < 0.4] = 0
    resets = 0
    for t in range(T):
        obs, rew, term, trunc, _ = env.step(torch.from_numpy(actions[t]).cuda())
        seen = env.observe()
        assert torch.equal(obs.view(torch.int32), seen.view(torch.int32)), t
        resets += int(term.sum())
    assert resets > 0 and env.last_step_kernel() == "K1"
    env.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("track,n", [(rc.TRACK_OF[n], n) for n in (90, 181)])
def test_off_menu_ray_counts_observe_current_state(track, n, dtype):
    """pc_env_observe on the handle's own state, set to the poses the harvested steps end at: F64 handles give the reference's bits,
    F32 handles stay within the float32 bars; both the bits of observe_poses of the same poses, and the state is left alone."""
    g = rc.harvest(track, n)
    M = len(g["action"])
    turns = np.rint((g["post_rot"] - g["reset_state"][4]) / 5.0).astype(np.int32)
    env = pc.VecCarEnv(M, TRACKS[track], num_rays=n, dtype=dtype)
    env.reset()
    env.set_state(px=g["post_px"], py=g["post_py"], vx=g["post_vx"], vy=g["post_vy"], rot=g["post_rot"], time_step=np.arange(M) % 900 + 1)
    before = env.get_state()
    col = torch.full((M,), 7, dtype=torch.uint8, device="cuda")
    obs = env.observe(collides=col).cpu().numpy()
    col = col.cpu().numpy()
    after = env.get_state()
    for k in before:
        assert np.array_equal(before[k].view(np.uint64) if before[k].dtype == np.float64 else before[k],
                              after[k].view(np.uint64) if after[k].dtype == np.float64 else after[k]), k
    obs_p, col_p = _observe(env, g["post_px"], g["post_py"], turns, g["post_vx"], g["post_vy"])
    assert np.array_equal(_bits(obs), _bits(obs_p)) and np.array_equal(col, col_p)
    if dtype == "f64":
        assert np.array_equal(_bits(obs), _bits(g["step_obs"])) and np.array_equal(col != 0, g["terminated"])
    else:
        _check_f32(obs, col, g["step_obs"], g["terminated"], g["wall_margin"] > MARGIN_PX)
    env.close()
