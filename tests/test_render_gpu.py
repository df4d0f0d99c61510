"""Frames on the device (pc_render_background, pc_render_frames, ppo_car_amd.Renderer, VecCarEnv.render, Evaluator(video_envs=K),
Trainer.save_video): every comparison is over every pixel, equality, against the numpy form of the drawing rule
(tests/render_reference.py)."""
import struct

import numpy as np
import pytest
import torch

import ppo_car_amd as pc
from ppo_car_amd import _capi
from ppo_car_amd.evaluation import Evaluator
from ppo_car_amd.env import ray_count
from ppo_car_amd.render import DEFAULT_PALETTE
from ppo_car_amd.renderer import Renderer
from conftest import TRACKS
from junction_track import _junction_track_json
from render_reference import GATE, reference_background, reference_frames

pytestmark = pytest.mark.gpu
INV, UNS = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_UNSUPPORTED
T_RUN = 60


def _mismatch(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, f"{what}: {len(bad)} of {want.size} bytes differ, first at {bad[:3].tolist()}"


_BG = {}


def _ref_bg(track, scale):
    """The reference background of a track file, computed once per (track, scale)."""
    if (track, scale) not in _BG:
        walls, gates = pc.Track(track).geometry()
        _BG[(track, scale)] = (walls, gates, reference_background(walls, gates, scale))
    return _BG[(track, scale)]


def _real_run(env):
    """reset + T_RUN steps under a fixed action pattern (mostly accelerating, random steering, every fourth env in a circle: some envs crash and are auto-reset):
    obs [T_RUN + 1, N, D] (row t = the observation before step t), next_gate [T_RUN + 1, N] from get_state(), the terminated flags."""
    N = env.num_envs
    rng = np.random.default_rng(5)
    actions = rng.integers(0, 9, size=(T_RUN, N)).astype(np.int64)
    actions[rng.random((T_RUN, N)) < 0.5] = 0
    actions[:, 3::4] = 4            # forward + left throughout: a circle of 115 px radius, into a wall
    obs = torch.empty(T_RUN + 1, N, env.obs_dim, device="cuda")
    ng = np.zeros((T_RUN + 1, N), np.int32)
    term = np.zeros((T_RUN, N), bool)
    env.reset(out=obs[0])
    for t in range(T_RUN):
        ng[t] = env.get_state()["next_gate"]
        _, _, te, _, _ = env.step(torch.from_numpy(actions[t]).cuda(), out=(obs[t + 1], env._new(N), env._new(N), env._new(N)))
        term[t] = te.cpu().numpy() != 0
    ng[T_RUN] = env.get_state()["next_gate"]
    return obs, ng, term


# ---- the background -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scales", [("track", (8, 5)), ("big_track", (8, 5, 2)), ("oval64", (8, 5)), ("junction", (8, 5))])
def test_background_equals_the_reference(tmp_path, name, scales):
    track = TRACKS[name] if name in TRACKS else _junction_track_json(str(tmp_path / "junction.json"))
    env = pc.VecCarEnv(4, track, num_rays=12, dtype="f64")
    for scale in scales:
        walls, gates = pc.Track(track).geometry()
        want = reference_background(walls, gates, scale) if name == "junction" else _ref_bg(track, scale)[2]
        _mismatch(Renderer(env, scale).background()[0], want, f"{name} scale {scale}")
    env.close()


# ---- frames from real rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_rays", [12, 16, 32, 360])
def test_frames_from_real_rows(num_rays):
    track = TRACKS["big_track"]
    walls, gates, bg = _ref_bg(track, 8)
    N = 16
    env = pc.VecCarEnv(N, track, num_rays=num_rays, reward_scaling=0.1)
    obs, ng, term = _real_run(env)
    assert term.any(), "the action pattern crashes no env: no auto-reset row is rendered"
    D = env.obs_dim
    assert D == 6 + ray_count(num_rays)
    r = Renderer(env, 8)
    flat, ngf = obs.reshape(-1, D), ng.reshape(-1)
    order = np.random.default_rng(1).permutation(len(flat))
    G = len(gates)
    for M in (1, 2, 65):
        idx = np.sort(order[:M])
        rows = flat[torch.from_numpy(idx).cuda()].contiguous()
        gate = ngf[idx].copy()
        got = r.frames(rows, next_gate=torch.from_numpy(gate).cuda())
        _mismatch(got, reference_frames(walls, gates, rows.cpu().numpy(), gate, num_rays, 8, background=bg), f"M {M} with next_gate")
        if num_rays != 360 or M == 2:       # (722 primitives per frame: the reference takes 50 ms per frame there)
            _mismatch(r.frames(rows), reference_frames(walls, gates, rows.cpu().numpy(), None, num_rays, 8, background=bg), f"M {M}, NULL next_gate")
    # next_gate 0, the last gate, one past a passed gate: on rows late in the run
    rows = obs[T_RUN, :3].contiguous()
    gate = np.array([0, G - 1, 7], np.int32)
    _mismatch(r.frames(rows, next_gate=torch.from_numpy(gate).cuda()),
              reference_frames(walls, gates, rows.cpu().numpy(), gate, num_rays, 8, background=bg), "chosen next_gate")
    # one env's rows read straight out of the [T, N, D] buffer: obs_ld = N * D
    T = T_RUN + 1 if num_rays != 360 else 8
    view = obs[:T, 5]
    assert view.stride(0) == N * D and not view.is_contiguous()
    gate = np.ascontiguousarray(ng[:T, 5])
    _mismatch(r.frames(view, next_gate=torch.from_numpy(gate).cuda()),
              reference_frames(walls, gates, view.cpu().numpy(), gate, num_rays, 8, background=bg), "strided rows")
    assert (ng > 0).any(), "no env passed a gate in the run"
    env.close()


def test_frames_scale_2_many_tiles():
    track = TRACKS["big_track"]
    walls, gates, bg = _ref_bg(track, 2)
    env = pc.VecCarEnv(8, track, num_rays=16, reward_scaling=0.1)
    obs, ng, _ = _real_run(env)
    rows = torch.stack([obs[T_RUN, 3], obs[17, 6]])
    gate = np.array([ng[T_RUN, 3], ng[17, 6]], np.int32)
    got = Renderer(env, 2).frames(rows, next_gate=torch.from_numpy(gate).cuda())
    assert got.shape == (2, 360, 640, 3)
    _mismatch(got, reference_frames(walls, gates, rows.cpu().numpy(), gate, 16, 2, background=bg), "scale 2")
    env.close()


def test_two_tracks_with_track_id_per_row():
    tracks = [TRACKS["big_track"], TRACKS["track"]]
    tid = (np.arange(8) & 1).astype(np.uint8)
    env = pc.VecCarEnv(8, tracks, num_rays=12, reward_scaling=0.1, track_id=tid)
    obs, ng, _ = _real_run(env)
    rows = obs[T_RUN].contiguous()
    gate = np.ascontiguousarray(ng[T_RUN])
    got = Renderer(env, 8).frames(rows, next_gate=torch.from_numpy(gate).cuda(), track_id=torch.from_numpy(tid).cuda()).cpu().numpy()
    for m in range(8):
        walls, gates, bg = _ref_bg(tracks[tid[m]], 8)
        _mismatch(got[m:m + 1], reference_frames(walls, gates, rows[m:m + 1].cpu().numpy(), gate[m:m + 1], 12, 8, background=bg), f"row {m}")
    env.close()


# ---- hand-made rows ----------------------------------------------------------------------------------------------------------------
def test_hand_made_rows_guards_and_palette():
    track = TRACKS["track"]
    walls, gates, bg = _ref_bg(track, 8)
    env = pc.VecCarEnv(4, track, num_rays=12)
    o = np.zeros((10, 18), np.float32)
    o[:, 0], o[:, 1], o[:, 4] = 0.5, 0.5, 1.0
    o[:, 6:] = 0.05
    o[0, :2] = 0.0                                  # the car at (0, 0)
    o[1, :2] = 1.0                                  # ... at (1280, 720)
    o[2, 6:10] = 0.0, 1.0, np.nan, 7.0              # a degenerate ray, 1000 px (leaves the frame), NaN (counts as 0), clamped to 1000 px
    o[2, 10] = -np.inf
    o[3, 4], o[3, 5] = 0.6, -0.8
    static = slice(4, 10)
    o[4, 4] = 1.5                                   # |cos| > 1
    o[5, 0] = np.nan
    o[6, 0] = 3000.0 / 1280.0
    o[7, 5] = -1.0000001
    o[8, 1] = -np.inf
    o[9] = o[3]                                     # its track_id is past the handle's tracks (below)
    gate = np.arange(10, dtype=np.int32)
    tid = np.zeros(10, np.uint8)
    tid[9] = 1
    r = Renderer(env, 8)
    rows = torch.from_numpy(o).cuda()
    got = r.frames(rows, next_gate=torch.from_numpy(gate).cuda(), track_id=torch.from_numpy(tid).cuda()).cpu().numpy()
    want = reference_frames(walls, gates, o, gate, 12, 8, background=bg)
    _mismatch(got[:9], want[:9], "hand-made rows")
    plain = DEFAULT_PALETTE[np.where(bg[1] != 0, GATE, bg[0])]
    for m in range(static.start, static.stop):
        _mismatch(got[m], plain, f"row {m}: the static layers only")
    assert not np.array_equal(got[3], plain)
    palette = np.random.default_rng(3).integers(0, 256, size=(8, 3), dtype=np.uint8)
    got = Renderer(env, 8, palette=palette).frames(rows[:4], next_gate=torch.from_numpy(gate[:4]).cuda())
    _mismatch(got, reference_frames(walls, gates, o[:4], gate[:4], 12, 8, palette=palette, background=bg), "custom palette")
    env.close()


# ---- nothing else is written ---------------------------------------------------------------------------------------------------------
def test_canaries_state_and_repeatability():
    track = TRACKS["big_track"]
    env = pc.VecCarEnv(8, track, num_rays=16, reward_scaling=0.1)
    obs, ng, _ = _real_run(env)
    rows = obs[T_RUN].contiguous()
    before_rows, before_state = rows.clone(), env.get_state()
    lib, st = _capi.lib, torch.cuda.current_stream().cuda_stream
    H, W, pad = 144, 256, 64
    bg = torch.full((pad + 2 * H * W + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.pc_render_background(env._h, 5, bg.data_ptr() + pad, st) == 0
    fr = torch.full((2, pad + 8 * H * W * 3 + pad), 0x5A, dtype=torch.uint8, device="cuda")
    gate = torch.from_numpy(np.ascontiguousarray(ng[T_RUN])).cuda()
    for k in range(2):
        assert lib.pc_render_frames(env._h, rows.data_ptr(), env.obs_dim, gate.data_ptr(), None, 8, 5, bg.data_ptr() + pad, None,
                                    fr[k].data_ptr() + pad, st) == 0
    torch.cuda.synchronize()
    assert (bg[:pad] == 0xA5).all() and (bg[-pad:] == 0xA5).all() and (fr[:, :pad] == 0x5A).all() and (fr[:, -pad:] == 0x5A).all()
    assert torch.equal(fr[0], fr[1])
    walls, gates, ref = _ref_bg(track, 5)
    _mismatch(bg[pad:-pad].reshape(2, H, W), ref, "background between the canaries")
    _mismatch(fr[0, pad:-pad].reshape(8, H, W, 3), reference_frames(walls, gates, rows.cpu().numpy(), ng[T_RUN], 16, 5, background=ref), "frames")
    assert torch.equal(rows, before_rows)
    after = env.get_state()
    for k in before_state:
        assert np.array_equal(before_state[k], after[k]), k
    env.close()


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    env = pc.VecCarEnv(4, TRACKS["track"], num_rays=12)         # no launch has happened on the handle
    lib, h, D, P = _capi.lib, env._h, env.obs_dim, 4096          # P: a non-NULL address that is never dereferenced
    assert lib.pc_render_background(h, 2, None, None) == INV
    for scale in (0, 3, 16, -1):
        assert lib.pc_render_background(h, scale, P, None) == INV
        assert lib.pc_render_frames(h, P, D, None, None, 1, scale, P, None, P, None) == INV
    assert lib.pc_render_background(h, 2, P + 1, None) == INV
    frames = lambda obs=P, ld=D, M=1, bg=P, out=P: lib.pc_render_frames(h, obs, ld, None, None, M, 2, bg, None, out, None)
    assert frames(obs=None) == INV and frames(bg=None) == INV and frames(out=None) == INV
    assert frames(M=0) == INV and frames(M=-2) == INV and frames(ld=D - 1) == INV
    assert frames(out=P + 2) == INV and frames(bg=P + 2) == INV
    env.close()
    # a track with a wall outside the renderer's box: the handle works, the render calls refuse it and say why
    walls = np.array([[500, 100, 2400, 100], [2400, 100, 2400, 600], [2400, 600, 500, 600], [500, 600, 500, 100],
                      [900, 300, 1800, 300], [1800, 300, 1800, 400], [1800, 400, 900, 400], [900, 400, 900, 300]], np.float64)
    gates = np.array([[700, 100, 700, 600], [2000, 300, 2400, 300]], np.float64)
    env = pc.VecCarEnv(4, pc.Track(walls=walls, gates=gates, start=(700.0, 200.0, 0.0)), num_rays=12, dtype="f64")
    env.reset()
    assert lib.pc_render_background(env._h, 2, P, None) == UNS
    assert b"wall 0" in lib.pc_last_hip_error()
    assert lib.pc_render_frames(env._h, P, D, None, None, 1, 2, P, None, P, None) == UNS
    assert lib.pc_render_background(env._h, 3, P, None) == INV           # the argument checks come first
    with pytest.raises(pc.PpoCarError):
        env.render()
    env.close()


# ---- VecCarEnv.render --------------------------------------------------------------------------------------------------------------
def test_env_render_after_set_state():
    track = TRACKS["big_track"]
    walls, gates, bg = _ref_bg(track, 8)
    t = pc.Track(track)
    env = pc.VecCarEnv(4, track, num_rays=16, render_mode="rgb_array")
    env.reset()
    env.set_state(px=t.start_x + np.array([0.0, 30.0, 55.5, -12.25]), py=t.start_y + np.array([0.0, 4.0, -6.5, 3.0]),
                  rot=t.start_angle + np.array([0.0, 5.0, -10.0, 180.0]), next_gate=np.array([0, 1, 5, len(gates) - 1]))
    before = env.get_state()
    got = env.render(scale=8)
    rows = env.observe().cpu().numpy()
    _mismatch(got, reference_frames(walls, gates, rows, before["next_gate"], 16, 8, background=bg), "render()")
    two = env.render(envs=[3, 0], scale=8)
    assert two.shape == (2, 90, 160, 3) and torch.equal(two[0], got[3]) and torch.equal(two[1], got[0])
    assert env.render().shape == (4, 360, 640, 3)
    after = env.get_state()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    env.close()


# ---- the evaluator's video ---------------------------------------------------------------------------------------------------------
def _trained_agent():
    from oracle.scenarios import load_trained_policy
    agent = pc.Agent(23, 9).cuda()
    load_trained_policy(agent)
    return agent


@pytest.mark.parametrize("greedy", [False, True])
def test_evaluator_video(greedy):
    agent = _trained_agent()
    N, K, every = 64, 2, 4
    kw = dict(n_envs=N, num_rays=16, reward_scaling=0.1, device="cuda", seed=11, greedy=greedy, chunk=1000)
    plain = Evaluator(agent, TRACKS["big_track"], rollout_kernel="mega", **kw)
    plain.run(index=2)
    want_state = plain.state.cpu().numpy().copy()
    assert plain.last_path == "mega"
    acts = plain._mega_rows["act"].to(torch.int64)                 # [1000, N]: what an independent replay is forced with
    sheets = {}
    for path in ("mega", "steps"):
        ev = Evaluator(agent, TRACKS["big_track"], rollout_kernel=path, video_envs=K, video_scale=8, video_every_step=every, **kw)
        ev.run(index=2)
        assert ev.last_path == path
        assert np.array_equal(ev.state.cpu().numpy(), want_state), f"{path}: the state with video differs from the state without"
        steps, ng, lengths = ev.video_plan()
        sheets[path] = ev.video_frames(cols=K)
        assert np.array_equal(lengths, want_state[1, :K].astype(np.int64))
        ev.close()
    assert np.array_equal(sheets["mega"], sheets["steps"])
    # the teacher-forced replay: a fresh env stepped with the evaluation's actions, its next gate read from the env itself
    env = pc.VecCarEnv(N, TRACKS["big_track"], num_rays=16, reward_scaling=0.1)
    G = pc.Track(TRACKS["big_track"]).n_gates
    L = int(lengths.max())
    rows = torch.empty(L, N, env.obs_dim, device="cuda")
    gate = torch.empty(L, N, dtype=torch.int32, device="cuda")
    nxt, _ = env.reset()
    for t in range(L):
        rows[t].copy_(nxt)
        gate[t].copy_(env.infos()["gates_passed"] % G)
        nxt = env.step(acts[t])[0]
    F = (L + every - 1) // every
    assert sheets["mega"].shape == (F, 90, K * 160, 3) and steps.shape == (F, K)
    r = Renderer(env, 8)
    for k in range(K):
        last = (int(lengths[k]) - 1) // every * every
        want_steps = np.minimum(np.arange(F) * every, last)            # a finished env holds its last frame
        assert np.array_equal(steps[:, k], want_steps)
        idx = torch.from_numpy(want_steps).cuda()
        want = r.frames(rows[idx, k].contiguous(), next_gate=gate[idx, k].contiguous()).cpu().numpy()
        assert np.array_equal(ng[:, k], gate[idx, k].cpu().numpy())
        _mismatch(sheets["mega"][:, :, k * 160:(k + 1) * 160], want, f"env {k}")
    plain.close(); env.close()


# ---- the trainer's video -----------------------------------------------------------------------------------------------------------
def test_trainer_video_leaves_training_bit_identical(tmp_path):
    from ppo_car_amd.ppo import PPOConfig, Trainer
    out = {}
    for video in (0, 1):
        cfg = PPOConfig(n_envs=64, n_steps=16, batch_size=16, train_iters=2, track=TRACKS["big_track"], num_rays=16, seed=3,
                        video_every=video, video_envs=2, video_scale=8)
        tr = Trainer(cfg, device="cuda:0")
        scal = []
        for epoch in (1, 2):
            scal.append(tr.run_epoch())
            if video:
                path = str(tmp_path / f"video_{epoch}.png")
                n = tr.save_video(path)
                steps, _, _ = tr.video_evaluator.video_plan()
                data = open(path, "rb").read()
                pos = data.index(b"acTL")
                assert struct.unpack(">II", data[pos + 4:pos + 12]) == (n, 0) and n == len(steps) and n >= 1
                assert struct.unpack(">II", data[16:24]) == (2 * 160, 90)
        out[video] = ([p.detach().cpu().numpy().copy() for p in tr.agent.parameters()], scal)
        assert (tr.video_evaluator is None) == (video == 0)
        tr.close()
    for a, b in zip(out[0][0], out[1][0]):
        assert np.array_equal(a, b)
    clock = lambda d: {k: v for k, v in d.items() if "SPS" not in k and k != "elapsed"}       # (the two wall-clock entries)
    for a, b in zip(out[0][1], out[1][1]):
        assert clock(a) == clock(b) and len(clock(a)) >= 5
