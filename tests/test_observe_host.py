"""Observe-without-stepping and the policy landscape, the parts that need no GPU: the C-ABI's symbols and argument checks, the
plain reference against the golden files, and PolicyLandscape's grid, chunking and reductions on a stand-in observe / act pair."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from ppo_car_amd import _capi
from ppo_car_amd import landscape as L
from conftest import ROOT
import observe_reference as R

INV = _capi.PC_ERR_INVALID_ARG
P = 4096      # a non-NULL address: every call below is refused before any device call, so it is never dereferenced


def test_symbols_exported_with_signatures():
    lib = C.CDLL(_capi.lib_path())
    for name, nargs in (("pc_env_observe_poses", 11), ("pc_env_observe", 4)):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.EXPORTS
        f = getattr(_capi.lib, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs
    assert _capi.lib.pc_env_observe_poses.argtypes[7] is C.c_int64      # M
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    assert re.search(r"int pc_env_observe_poses\(const pc_env\* e, const double\* px, const double\* py, const double\* vx, const double\* vy,\s*"
                     r"const int32_t\* turns, const uint8_t\* track_id, int64_t M, float\* obs, uint8_t\* collides, void\* stream\);", hdr)
    assert re.search(r"int pc_env_observe\(pc_env\* e, float\* obs, uint8_t\* collides, void\* stream\);", hdr)


def _poses(e=P, px=P, py=P, vx=P, vy=P, turns=P, tid=P, M=8, obs=P, col=P):
    return _capi.lib.pc_env_observe_poses(e, px, py, vx, vy, turns, tid, M, obs, col, None)


@pytest.mark.parametrize("kw", [dict(e=None), dict(px=None), dict(py=None), dict(turns=None), dict(obs=None), dict(M=0), dict(M=-5)])
def test_observe_poses_argument_errors_before_any_device_call(kw):
    # (the handle is a made-up address too: the refusal comes before the handle is looked at)
    assert _poses(**kw) == INV


def test_observe_argument_errors_before_any_device_call():
    assert _capi.lib.pc_env_observe(None, P, P, None) == INV
    assert _capi.lib.pc_env_observe(P, None, P, None) == INV


@pytest.mark.parametrize("track,n", R.CONFIGS)
def test_reference_reproduces_golden_rows(track, n):
    g = R.golden_rows(track, n)
    assert len(g["px"]) == 2 * R.ROWS
    obs, col = R.observe_many(g["px"], g["py"], g["vx"], g["vy"], g["rot"], n, g["walls"])
    assert np.array_equal(obs.view(np.uint32), g["obs"].view(np.uint32))
    assert np.array_equal(col, g["terminated"])
    assert np.abs(g["rot"] - (g["start_rot"] + 5.0 * g["turns"])).max() < 1e-9      # every rotation lies on the 5-degree grid


# ---- PolicyLandscape on a stand-in observe / act pair (torch CPU) ----------------------------------------------------------------
class FakeTrack:
    path = None

    def __init__(self, angle):
        self.start_angle = angle

    def geometry(self):
        return np.array([[100.0, 100.0, 1180.0, 100.0]]), np.array([[640.0, 0.0, 640.0, 720.0]])


class FakeEnvs:
    """obs row = (px, py, vx, vy, turns, track); collides: the left half of the frame at every heading, and headings below 36 in the
    top right quarter."""
    obs_dim = 6

    def __init__(self, angles):
        self._tracks = [FakeTrack(a) for a in angles]
        self.calls = []

    def observe_poses(self, px, py, turns, vx=None, vy=None, track_id=None, out=None, collides=None):
        self.calls.append(px.numel())
        out[:, 0], out[:, 1], out[:, 2], out[:, 3] = px, py, vx, vy
        out[:, 4], out[:, 5] = turns.to(torch.float32), track_id.to(torch.float32)
        collides.copy_(((px < 640) | ((py < 360) & (turns < 36))).to(torch.uint8))
        return out


class FakeAgent:
    def __init__(self):
        self.calls = []

    def act(self, obs, out_action=None, out_logprob=None, out_value=None, greedy=False, repack=True):
        assert greedy
        self.calls.append((obs.shape[0], repack))
        turns = obs[:, 4]
        out_value.copy_(-(turns - 50.0).abs() + obs[:, 5] * 100.0 + obs[:, 0] / 1280.0)      # peaks at heading 50 (36 .. 71 and 0 .. 71 alike)
        out_action.copy_((turns.to(torch.int64) + obs[:, 5].to(torch.int64)) % 9)
        return out_action, out_logprob, out_value


def test_grid_poses():
    px, py, vx, vy, turns = L.grid_poses(30.0, 80, 0.5)
    GH, GW = 9, 16
    assert px.shape == (72 * GH * GW,) and px.dtype == np.float64 and turns.dtype == np.int32
    sh = (72, GH, GW)
    assert np.array_equal(px.reshape(sh)[5, 3], (np.arange(GW) + 0.5) * 80) and np.array_equal(py.reshape(sh)[7, :, 2], (np.arange(GH) + 0.5) * 80)
    assert np.array_equal(turns.reshape(sh)[:, 4, 4], np.arange(72))
    a = np.radians(30.0 + 5.0 * np.arange(72))
    assert np.array_equal(vx.reshape(sh)[:, 0, 0], 5.0 * np.cos(a)) and np.array_equal(vy.reshape(sh)[:, 8, 15], 5.0 * np.sin(a))


@pytest.mark.parametrize("cell,chunks", [(80, [20736]), (8, [1 << 18] * 7 + [2 * 72 * 90 * 160 - 7 * (1 << 18)])])
def test_landscape_chunks_and_reductions(cell, chunks, tmp_path):
    envs, agent = FakeEnvs([0.0, 90.0]), FakeAgent()
    ls = L.PolicyLandscape(agent, None, 16, cell_px=cell, speed=0.5, device="cpu", envs=envs)
    GH, GW = 720 // cell, 1280 // cell
    assert ls.grid == (GH, GW) and ls.value.shape == (2, 72, GH, GW)
    assert ls.compute() is ls
    assert envs.calls == chunks and max(chunks) <= 1 << 18
    assert agent.calls == [(c, i == 0) for i, c in enumerate(chunks)]      # one greedy act per chunk, the weights packed once
    px, py, vx, vy, turns, tid = (t.reshape(2, 72, GH, GW) for t in ls.poses())
    assert ls.action.dtype == torch.uint8 and ls.drivable.dtype == torch.bool and ls.value.dtype == torch.float32
    assert torch.equal(ls.drivable, ~((px < 640) | ((py < 360) & (turns < 36))))
    assert torch.equal(ls.action, ((turns.long() + tid.long()) % 9).to(torch.uint8))
    want = (-(turns.float() - 50.0).abs() + tid.float() * 100.0 + px.float() / 1280.0)
    assert torch.equal(ls.value, want)
    for k in (0, 1):
        best, head, act = ls.best_value(k), ls.best_heading(k), ls.action_at_best(k)
        none = ~ls.drivable[k].any(0)
        assert torch.equal(none, (px[k, 0] < 640)) and none.any() and (~none).any()
        assert torch.equal(best.isnan(), none) and torch.equal(head.isnan(), none)      # NaN exactly where no heading is drivable
        assert torch.equal(act == L.NO_ACTION, none)
        ok = ~none
        assert torch.equal(best[ok], want[k, 50][ok])
        assert torch.equal(head[ok], torch.full_like(head[ok], (0.0, 90.0)[k] + 250.0))
        assert torch.equal(act[ok], torch.full_like(act[ok], (50 + k) % 9))
    if cell == 80:
        files = ls.save(str(tmp_path / "out" / "run"))
        assert [os.path.basename(f) for f in files] == ["run_landscape.npz", "run_landscape_track0.png", "run_landscape_track1.png"]
        z = np.load(files[0])
        assert np.array_equal(z["value"], ls.value.numpy()) and np.array_equal(z["drivable"], ls.drivable.numpy())
        assert np.array_equal(np.isnan(z["best_value"][0]), (~ls.drivable[0].any(0)).numpy()) and int(z["cell_px"]) == 80
        assert all(os.path.getsize(f) > 0 for f in files)
    ls.close()


def test_landscape_rejects_bad_arguments():
    with pytest.raises(ValueError):
        L.PolicyLandscape(FakeAgent(), None, 16, cell_px=7, device="cpu", envs=FakeEnvs([0.0]))
    with pytest.raises(ValueError):
        L.PolicyLandscape(FakeAgent(), None, 16, speed=1.5, device="cpu", envs=FakeEnvs([0.0]))


def test_best_value_is_nan_exactly_where_nothing_is_drivable():
    g = torch.Generator().manual_seed(3)
    value = torch.randn(72, 5, 7, generator=g)
    drivable = torch.rand(72, 5, 7, generator=g) < 0.02
    drivable[:, 0, 0] = False
    drivable[:, 1, 1] = False
    drivable[10, 1, 1] = True
    best, turn = L.best_value(value, drivable), L.best_turn(value, drivable)
    assert torch.equal(best.isnan(), ~drivable.any(0)) and torch.equal(turn < 0, ~drivable.any(0))
    assert best[1, 1] == value[10, 1, 1] and turn[1, 1] == 10
    v, d = value.numpy(), drivable.numpy()
    for cy in range(5):
        for cx in range(7):
            if d[:, cy, cx].any():
                idx = np.flatnonzero(d[:, cy, cx])
                assert best[cy, cx] == v[idx, cy, cx].max() and turn[cy, cx] == idx[v[idx, cy, cx].argmax()]
