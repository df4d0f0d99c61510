"""Track telemetry maps (pc_track_maps, ppo_car_amd.TrackMaps, render.heatmap): the numpy reference (track_maps_reference.py, which the
GPU tests hold the kernel to) on hand-built rows, the C-ABI surface and its argument checks in their stated order, the heat-map
renderer, the trainer / CLI switches and the state dict.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from ppo_car_amd import _capi
from conftest import ROOT, TRACKS
from first_episode_reference import RUNNING, TERMINATED, TRUNCATED, buffer_flags, new_state
from track_maps_reference import CELLS, CRASHES, PLANES, SPEED, VISITS, cell_of, grid, speed_q, track_maps_ref

INV, NODEV = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_NO_DEVICE
NAN = np.float32(np.nan)


def rows(points, D=6):
    """points [T][N] of (x, y, vx, vy) -> obs [T, N, D] float32 (the other entries are filler the maps must not read)."""
    p = np.array(points, np.float32)
    obs = np.full(p.shape[:2] + (D,), 7.5, np.float32)
    obs[..., :4] = p
    return obs


def zeros(T, N=1):
    return np.zeros((T, N), np.float32)


# ---- the reference on hand-built rows ------------------------------------------------------------------------------------------
def test_grid_and_cell_list():
    assert CELLS == (4, 5, 8, 10, 16, 20, 40, 80) == tuple(c for c in range(4, 81) if 80 % c == 0)
    assert grid(8) == (90, 160) and grid(80) == (9, 16) and grid(4) == (180, 320)


def test_reference_point_on_a_cell_border():
    """x = k / GW exactly (a power-of-two multiple: exact in float32) belongs to cell k; the float32 below it to cell k - 1."""
    GH, GW = grid(80)
    x = np.float32(4 / 16)
    below = np.nextafter(x, np.float32(0))
    cx, cy = cell_of([x, below], [np.float32(3 / 9), np.float32(3 / 9)], 80)
    assert cx.tolist() == [4, 3]
    assert cy.tolist() == [int(np.floor(np.float32(3 / 9) * np.float32(9)))] * 2
    m = track_maps_ref(rows([[(x, 0.5, 0, 0)], [(below, 0.5, 0, 0)]]), zeros(2), zeros(2), 80)
    assert m[0, VISITS, 4, 4] == 1 and m[0, VISITS, 4, 3] == 1 and m[0, VISITS].sum() == 2


def test_reference_edges_are_clamped():
    GH, GW = grid(8)
    pts = [[(1.0, 1.0, 0, 0)], [(-0.01, -3.0, 0, 0)], [(1.2, 0.0, 0, 0)], [(np.float32(3e38), np.float32(-3e38), 0, 0)]]
    m = track_maps_ref(rows(pts), zeros(4), zeros(4), 8)
    assert m[0, VISITS, GH - 1, GW - 1] == 1       # x = y = 1.0: floor gives GW, GH -> the last cells
    assert m[0, VISITS, 0, 0] == 1                  # below 0 on both axes
    assert m[0, VISITS, 0, GW - 1] == 2             # above 1 in x (the product of 3e38 overflows to +inf: still the last cell)
    assert m[0, VISITS].sum() == 4


def test_reference_nan_and_inf_positions_are_skipped_entirely():
    pts = [[(NAN, 0.5, 1, 0)], [(0.5, np.float32(np.inf), 1, 0)], [(0.5, 0.5, 1, 0)]]
    m = track_maps_ref(rows(pts), np.ones((3, 1), np.float32), zeros(3), 8)
    assert m[0, VISITS].sum() == 1 and m[0, CRASHES].sum() == 1 and m[0, SPEED].sum() == 1024


def test_reference_buffer_layout_equals_steps_layout():
    """The same three steps in both layouts: step t's flags in row t + 1 / last_* against flags[t]."""
    obs = rows([[(0.1, 0.1, 0.5, 0)], [(0.2, 0.2, 0.5, 0)], [(0.3, 0.3, 0.5, 0)]])
    term_b = np.array([[1.0], [0.0], [1.0]], np.float32)     # row 0 belongs to the step before the window: never read
    trunc_b = zeros(3)
    te, tr = buffer_flags(term_b, trunc_b, np.array([0.0], np.float32), np.array([1.0], np.float32))
    assert te[:, 0].tolist() == [0, 1, 0] and tr[:, 0].tolist() == [0, 0, 1]
    m = track_maps_ref(obs, te, tr, 80)
    same = track_maps_ref(obs, np.array([[0.0], [1.0], [0.0]], np.float32), np.array([[0.0], [0.0], [1.0]], np.float32), 80)
    assert np.array_equal(m, same)
    assert m[0, CRASHES].sum() == 1 and m[0, CRASHES, int(0.2 * 9), int(0.2 * 16)] == 1


def test_reference_crash_goes_to_the_cell_before_the_step_and_a_truncation_is_no_crash():
    obs = rows([[(0.10, 0.50, 0, 0)], [(0.60, 0.50, 0, 0)], [(0.90, 0.50, 0, 0)]])
    m = track_maps_ref(obs, np.array([[0.0], [1.0], [0.0]], np.float32), np.array([[1.0], [0.0], [1.0]], np.float32), 80)
    assert m[0, CRASHES].sum() == 1 and m[0, CRASHES, 4, int(np.float32(0.60) * np.float32(16))] == 1     # row 1's own cell
    assert m[0, VISITS].sum() == 3                          # without first_state every sample counts


def test_reference_first_state_cut():
    """Env 0 closes at step 1 (counted, rows 2-3 not); env 1 is not RUNNING on entry (ignored); env 2 runs through."""
    T, N = 4, 3
    obs = rows([[(0.1 * (t + 1), 0.5, 1.0, 0)] * N for t in range(T)])
    term, trunc = zeros(T, N), zeros(T, N)
    term[1, 0] = 1
    term[2, 0] = 1          # after the close: neither a visit nor a crash
    st = new_state(N)
    st[4, 1] = TRUNCATED
    m = track_maps_ref(obs, term, trunc, 80, first_state=st)
    assert m[0, VISITS].sum() == 2 + 0 + 4 and m[0, CRASHES].sum() == 1
    assert m[0, CRASHES, 4, int(np.float32(0.2) * np.float32(16))] == 1
    st[4, 1] = TERMINATED
    assert np.array_equal(track_maps_ref(obs, term, trunc, 80, first_state=st), m)
    # a truncation closes too
    trunc[0, 2] = 1
    assert track_maps_ref(obs, term, trunc, 80, first_state=st)[0, VISITS].sum() == 2 + 0 + 1
    # ... and the cut splits into windows: the state after window 1 says who still counts in window 2
    st2 = st.copy()
    st2[4, 0] = RUNNING      # after rows 0-0 env 0 is still running, env 2 was truncated in row 0
    st2[4, 2] = TRUNCATED
    two = track_maps_ref(obs[1:], term[1:], trunc[1:], 80, first_state=st2,
                         maps=track_maps_ref(obs[:1], term[:1], trunc[:1], 80, first_state=st))
    assert np.array_equal(two, track_maps_ref(obs, term, trunc, 80, first_state=st))


def test_reference_two_tracks_and_an_id_out_of_range():
    obs = rows([[(0.5, 0.5, 0, 1.0)] * 4])
    m = track_maps_ref(obs, np.ones((1, 4), np.float32), zeros(1, 4), 80, n_tracks=2, track_id=np.array([0, 1, 1, 2], np.uint8))
    assert m.shape == (2, PLANES, 9, 16)
    assert m[0, VISITS].sum() == 1 and m[1, VISITS].sum() == 2 and m[:, CRASHES].sum() == 3 and m[1, SPEED].sum() == 2048


def test_reference_speed_unit():
    """q for (0.6, 0.8): the float32 inputs squared and summed in float64, one sqrt, times 1024, rint."""
    a, b = np.float64(np.float32(0.6)), np.float64(np.float32(0.8))
    want = int(np.rint(np.sqrt(a * a + b * b) * 1024.0))
    assert speed_q(np.float32(0.6), np.float32(0.8)) == want == 1024
    assert speed_q(np.float32(1.0), np.float32(-1.0)) == int(np.rint(np.sqrt(2.0) * 1024.0)) == 1448
    assert speed_q(np.float32(0.0), np.float32(0.0)) == 0 and speed_q(NAN, np.float32(0.0)) == 0
    m = track_maps_ref(rows([[(0.5, 0.5, 0.6, 0.8)], [(0.5, 0.5, 1.0, -1.0)]]), zeros(2), zeros(2), 8)
    assert m[0, SPEED, 45, 80] == 1024 + 1448 and m[0, VISITS, 45, 80] == 2


def test_reference_accumulates():
    obs = rows([[(0.5, 0.5, 0.5, 0)]])
    m = track_maps_ref(obs, zeros(1), zeros(1), 8)
    m2 = track_maps_ref(obs, zeros(1), zeros(1), 8, maps=m)
    assert np.array_equal(m2, 2 * m) and m[0, VISITS].sum() == 1


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------
def test_symbol_and_constants_in_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    assert re.search(r"\bint pc_track_maps\(", hdr)
    assert "pc_track_maps" in _capi.EXPORTS and _capi.lib.pc_track_maps is not None
    for name, value in (("PC_MAP_VISITS", 0), ("PC_MAP_SPEED", 1), ("PC_MAP_CRASHES", 2), ("PC_MAP_PLANES", 3), ("PC_MAP_SPEED_UNIT", 1024)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
        assert getattr(_capi, name) == value
    assert _capi.PC_MAP_CELLS == CELLS
    assert (VISITS, SPEED, CRASHES, PLANES) == (_capi.PC_MAP_VISITS, _capi.PC_MAP_SPEED, _capi.PC_MAP_CRASHES, _capi.PC_MAP_PLANES)


P = 4096      # a non-NULL address: every call below is refused before any device call, so it is never dereferenced


def _maps(device=0, obs=P, D=18, term=P, trunc=P, lt=P, ltr=P, T=8, N=8, layout=0, tid=P, n_tracks=1, cell=8, first=P, maps=P):
    return _capi.lib.pc_track_maps(device, obs, D, term, trunc, lt, ltr, T, N, layout, tid, n_tracks, cell, first, maps, None)


@pytest.mark.parametrize("bad", [dict(obs=None), dict(term=None), dict(trunc=None), dict(maps=None), dict(T=0), dict(T=-2), dict(N=0),
                                 dict(N=-1), dict(D=3), dict(D=0), dict(layout=2), dict(layout=-1), dict(lt=None), dict(ltr=None),
                                 dict(n_tracks=0), dict(n_tracks=257), dict(n_tracks=-1), dict(cell=0), dict(cell=-8), dict(cell=1),
                                 dict(cell=2), dict(cell=3), dict(cell=6), dict(cell=32), dict(cell=160), dict(cell=720)])
def test_argument_checks_come_before_the_device(bad):
    assert _maps(**bad) == INV
    assert _maps(device=-1, **bad) == INV           # the arguments are looked at before the device
    assert _maps(device=1 << 20, **bad) == INV


@pytest.mark.parametrize("cell", CELLS)
def test_every_listed_cell_size_reaches_the_device_check(cell):
    assert _maps(device=-1, cell=cell) == NODEV
    assert _maps(device=1 << 20, cell=cell) == NODEV


def test_optional_arguments_reach_the_device_check():
    assert _maps(device=-1, tid=None, first=None) == NODEV
    assert _maps(device=-1, lt=None, ltr=None, layout=1) == NODEV        # the steps layout needs no last flags
    assert _maps(device=-1, D=4, n_tracks=256, T=1, N=1) == NODEV
    if not torch.cuda.is_available():      # a box without a GPU: every device index
        assert _maps() == NODEV


# ---- render.heatmap --------------------------------------------------------------------------------------------------------------
def test_heatmap(tmp_path):
    from ppo_car_amd.env import Track
    from ppo_car_amd.render import COLORS, heatmap, write_png
    walls, gates = Track(TRACKS["big_track"]).geometry()
    GH, GW = grid(8)
    v = np.zeros((GH, GW))
    v[10:20, 30:40] = 1.0
    v[50:60, 100:110] = 1000.0
    img = heatmap(v, walls, gates)
    assert img.shape == (720, 1280, 3) and img.dtype == np.uint8
    bg, wall = np.array(COLORS["background"], np.uint8), np.array(COLORS["wall"], np.uint8)
    is_wall = (img == wall).all(-1)
    is_gate = (img == np.array(COLORS["gate"], np.uint8)).all(-1)
    assert is_wall.sum() > 500
    free = ~(is_wall | is_gate)
    seen = np.kron(v > 0, np.ones((8, 8), bool))
    assert (img[free & ~seen] == bg).all()                   # no visits: the background
    lo, hi = img[10 * 8:20 * 8, 30 * 8:40 * 8][free[10 * 8:20 * 8, 30 * 8:40 * 8]], img[50 * 8:60 * 8, 100 * 8:110 * 8][free[50 * 8:60 * 8, 100 * 8:110 * 8]]
    assert len(lo) and len(hi) and (lo == lo[0]).all() and (hi == hi[0]).all()
    assert not (lo[0] == hi[0]).all() and not (lo[0] == bg).all() and not (hi[0] == bg).all()
    # linear scale: NaN is "no data", 0 is data
    lin = heatmap(np.where(v > 0, v, np.nan), walls, gates, log=False)
    assert (lin[free & ~seen] == bg).all() and not (lin[free & seen] == bg).all(-1).any()
    z = heatmap(np.zeros((GH, GW)), walls[:0], gates[:0], log=False)
    assert not (z == bg).all(-1).any()
    small = heatmap(v, walls, gates, size=(640, 360))
    assert small.shape == (360, 640, 3)
    path = tmp_path / "m.png"
    write_png(str(path), img)
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"


# ---- the switches ----------------------------------------------------------------------------------------------------------------
def test_config_and_cli_default_off():
    import evaluate
    import train
    from ppo_car_amd.ppo import PPOConfig
    cfg = PPOConfig()
    assert cfg.track_maps is False and cfg.track_maps_cell == 8 and cfg.track_maps_every == 0 and cfg.eval_track_maps is False
    a = train.parse_args(["--run-name", "x"])
    assert a.track_maps is False and a.track_maps_cell == 8 and a.track_maps_every == 0 and a.eval_track_maps is False
    a = train.parse_args(["--run-name", "x", "--track-maps", "--track-maps-cell", "16", "--track-maps-every", "10", "--eval-track-maps"])
    assert a.track_maps is True and a.track_maps_cell == 16 and a.track_maps_every == 10 and a.eval_track_maps is True
    with pytest.raises(SystemExit):
        train.parse_args(["--run-name", "x", "--track-maps-cell", "7"])
    e = evaluate.parse_args(["--checkpoint", "c"])
    assert e.maps is None
    e = evaluate.parse_args(["--checkpoint", "c", "--envs", "64", "--maps", "out/m"])
    assert e.maps == "out/m" and e.envs == 64
    with pytest.raises(ValueError):
        PPOConfig(track_maps_cell=7)
    with pytest.raises(ValueError):
        PPOConfig(track_maps_every=-1)
    PPOConfig(track_maps=True, track_maps_cell=80, track_maps_every=3, eval_track_maps=True)


def test_track_maps_on_cpu_storage(tmp_path):
    """The class keeps its counts wherever it is told to; only update() needs the GPU."""
    import ppo_car_amd as pc
    from ppo_car_amd.evaluation import Evaluator        # noqa: F401  (the import chain of the switches)
    m = pc.TrackMaps(n_tracks=2, cell_px=80, device="cpu")
    assert m.counts.shape == (2, 3, 9, 16) and m.counts.dtype == torch.int64 and not m.counts.any()
    with pytest.raises(RuntimeError):
        m.update(torch.zeros(1, 1, 6), torch.zeros(1, 1), torch.zeros(1, 1), torch.zeros(1), torch.zeros(1))
    for bad in (dict(n_tracks=0), dict(n_tracks=257), dict(cell_px=7)):
        with pytest.raises(ValueError):
            pc.TrackMaps(device="cpu", **bad)
    m.counts[1, VISITS, 4, 5] = 4
    m.counts[1, SPEED, 4, 5] = 4 * 512
    m.counts[1, CRASHES, 4, 5] = 1
    assert m.visits(1)[4, 5] == 4 and m.visits(0).sum() == 0
    assert m.mean_speed(1)[4, 5] == 5.0 and torch.isnan(m.mean_speed(1)[0, 0])         # 512 / 1024 of max_speed = 10 px per step
    assert m.crash_rate(1)[4, 5] == 0.25 and torch.isnan(m.crash_rate(0)).all()
    sd = m.state_dict()
    assert set(sd) == {"counts", "cell_px"} and sd["cell_px"] == 80 and sd["counts"].data_ptr() != m.counts.data_ptr()
    m2 = pc.TrackMaps(n_tracks=2, cell_px=80, device="cpu")
    m2.load_state_dict(sd)
    assert torch.equal(m2.counts, m.counts)
    with pytest.raises(ValueError):
        pc.TrackMaps(n_tracks=2, cell_px=40, device="cpu").load_state_dict(sd)
    with pytest.raises(ValueError):
        pc.TrackMaps(n_tracks=1, cell_px=80, device="cpu").load_state_dict(sd)
    files = m.save(str(tmp_path / "maps" / "m"), [TRACKS["big_track"], TRACKS["track"]])
    assert len(files) == 1 + 2 * 3 and all(os.path.exists(f) for f in files)
    z = np.load(files[0])
    assert np.array_equal(z["counts"], m.counts.numpy()) and int(z["cell_px"]) == 80 and z["tracks"].tolist() == ["big_track", "track"]
    assert all(open(f, "rb").read(8) == b"\x89PNG\r\n\x1a\n" for f in files[1:])
    m.clear()
    assert not m.counts.any()
