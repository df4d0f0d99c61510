"""Frames on the device, the host side (no GPU): the numpy reference of the drawing rule (render_reference.py, which the GPU tests hold
the kernels to) against hand-derived pixels, render.py's animated PNG and contact sheets, the switches and their ValueErrors, the C-ABI
surface."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

import ppo_car_amd as pc
from ppo_car_amd import _capi
from ppo_car_amd.render import DEFAULT_PALETTE, contact_sheet, write_apng
from conftest import ROOT, TRACKS
from render_reference import (CAR, GRASS, HIT, RAY, ROAD, SCALES, WALL, Q, covers, grid, half_width, reference_background,
                              reference_frames)
import render_reference

INV, UNS = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def geometry():
    return {k: pc.Track(TRACKS[k]).geometry() + (pc.Track(TRACKS[k]),) for k in ("track", "big_track")}


@pytest.fixture(scope="module")
def backgrounds(geometry):
    return {(k, s): reference_background(geometry[k][0], geometry[k][1], s) for k in geometry for s in (2, 8)}


# ---- the reference against hand-derived pixels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["track", "big_track"])
@pytest.mark.parametrize("scale", [2, 8])
def test_start_is_road_corner_is_grass_wall_midpoint_is_wall(geometry, backgrounds, name, scale):
    walls, gates, t = geometry[name]
    bg = backgrounds[(name, scale)]
    assert bg.shape == (2, 720 // scale, 1280 // scale) and bg.dtype == np.uint8
    assert bg[0, int(t.start_y) // scale, int(t.start_x) // scale] == ROAD
    assert bg[0, 0, 0] == GRASS and bg[1, 0, 0] == 0
    mx, my = (walls[0, 0] + walls[0, 2]) / 2, (walls[0, 1] + walls[0, 3]) / 2
    assert bg[0, int(my) // scale, int(mx) // scale] == WALL
    assert set(np.unique(bg[0])) == {GRASS, ROAD, WALL}
    assert bg[1].max() == len(gates)                    # the last gate is nowhere hidden behind a later one


def test_horizontal_ray_covers_exactly_the_expected_run():
    """A ray from (200, 300) px to (300, 300) px: in quarter pixels (800, 1200) - (1200, 1200).
    scale 1: centres at 4 i + 2, half-width max(2, 3) = 3 q.  Rows 299 and 300 (|dy| = 2); between the ends columns 200 .. 299, and one
    more at either end: (798, 1198) is sqrt(8) < 3 from A.  scale 8: centres at 32 i + 16, half-width 24 q: row 37 only (1200; the next
    rows are 32 q away), columns 25 (816) .. 37 (1200 = B itself) and 24 (784: 16 q before A); column 38 is 32 q past B."""
    for scale, rows, cols in ((1, (299, 300), (199, 300)), (8, (37, 37), (24, 37))):
        Px, Py = grid(scale)
        got = covers(Px, Py, (800, 1200), (1200, 1200), half_width(2, scale))
        want = np.zeros_like(got)
        want[rows[0]:rows[1] + 1, cols[0]:cols[1] + 1] = True
        assert np.array_equal(got, want), scale


def test_frame_layers_on_a_hand_made_row(geometry, backgrounds):
    """One row on big_track at scale 8: the car at the start, heading +x, ray 0 of 100 px and every other ray of length 0."""
    walls, gates, t = geometry["big_track"]
    o = np.zeros((1, 18), np.float32)
    o[0, :2] = t.start_x / 1280.0, t.start_y / 720.0
    o[0, 4] = 1.0
    o[0, 6] = 0.1
    f = reference_frames(walls, gates, o, [3], 12, 8, background=backgrounds[("big_track", 8)])
    assert f.shape == (1, 90, 160, 3)
    x, y = float(np.float64(o[0, 0]) * 1280.0), float(np.float64(o[0, 1]) * 720.0)
    at = lambda px, py: tuple(f[0, int(py) // 8, int(px) // 8])
    pal = [tuple(c) for c in DEFAULT_PALETTE]
    assert at(x, y) == pal[CAR] and at(x + 14, y) == pal[CAR]
    assert at(x + 60, y) == pal[RAY] and at(x + 100, y) == pal[HIT]
    assert at(0, 0) == pal[GRASS]
    assert np.array_equal(DEFAULT_PALETTE, render_reference.DEFAULT_PALETTE)
    # next_gate = 20: gates 0 .. 19 are hidden, gate 20 is highlighted; None: every gate plain (gates away from the car and its ray)
    f = reference_frames(walls, gates, o, [20], 12, 8, background=backgrounds[("big_track", 8)])
    plain = reference_frames(walls, gates, o, None, 12, 8, background=backgrounds[("big_track", 8)])
    gq = Q(gates)
    for g, shown in ((10, False), (20, True), (30, True)):
        mx, my = (gq[g, 0] + gq[g, 2]) / 8.0, (gq[g, 1] + gq[g, 3]) / 8.0
        assert np.hypot(mx - x, my - y) > 150.0
        j, i = int(my) // 8, int(mx) // 8
        assert tuple(plain[0, j, i]) == pal[render_reference.GATE]
        assert tuple(f[0, j, i]) == (pal[render_reference.NEXT_GATE] if g == 20 else pal[render_reference.GATE] if shown else pal[ROAD]), g


def test_guards_draw_the_static_layers_only(geometry, backgrounds):
    walls, gates, _ = geometry["track"]
    bg = backgrounds[("track", 8)]
    static = DEFAULT_PALETTE[np.where(bg[1] != 0, render_reference.GATE, bg[0])]
    o = np.zeros((5, 18), np.float32)
    o[:, :2], o[:, 4] = 0.5, 1.0
    o[0, 4] = 1.5                   # |cos| > 1
    o[1, 0] = np.nan
    o[2, 0] = 3000.0 / 1280.0       # outside the box
    o[3, 5] = np.inf
    f = reference_frames(walls, gates, o, [2] * 5, 12, 8, background=bg)
    for m in range(4):
        assert np.array_equal(f[m], static), m
    assert not np.array_equal(f[4], static)


@pytest.mark.parametrize("scale", SCALES)
def test_lines_are_gap_free_at_every_scale(geometry, scale):
    """Every 1-px sample along every (quantised) wall, and along a 45-degree ray, lies in a covered pixel: the half-width is at least
    3 * scale q = 0.75 * scale px, the half-diagonal of a pixel is 0.71 * scale px."""
    Px, Py = grid(scale)
    H, W = Py.shape[0], Px.shape[1]
    segs = [(tuple(w[:2]), tuple(w[2:]), half_width(10, scale)) for w in Q(geometry["track"][0]).tolist()]
    segs.append(((403, 290), (403 + 1111, 290 + 1111), half_width(2, scale)))
    for A, B, h in segs:
        got = covers(Px, Py, A, B, h)
        n = int(np.hypot(B[0] - A[0], B[1] - A[1]) / 4.0) + 1
        t = np.linspace(0.0, 1.0, n + 1)
        sx, sy = (A[0] + t * (B[0] - A[0])) / 4.0, (A[1] + t * (B[1] - A[1])) / 4.0        # px
        i, j = np.floor(sx / scale).astype(int), np.floor(sy / scale).astype(int)
        ok = (i >= 0) & (i < W) & (j >= 0) & (j < H)
        assert ok.any() and got[j[ok], i[ok]].all(), (A, B)


# ---- write_apng, contact_sheet ----------------------------------------------------------------------------------------------------
def _chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff, tag
        out.append((tag, body))
        pos += 12 + n
    return out


def test_write_apng_chunks_and_pixels(tmp_path):
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, size=(3, 5, 7, 3), dtype=np.uint8)
    path = tmp_path / "a.png"
    write_apng(str(path), frames, fps=25)
    ch = _chunks(path.read_bytes())
    assert [t for t, _ in ch] == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fcTL", b"fdAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", ch[0][1]) == (7, 5, 8, 2, 0, 0, 0)
    assert struct.unpack(">II", ch[1][1]) == (3, 0)
    seq = []
    images = []
    for tag, body in ch:
        if tag == b"fcTL":
            s, w, h, x, y, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", body)
            assert (w, h, x, y, num, den, dispose, blend) == (7, 5, 0, 0, 1, 25, 0, 0)
            seq.append(s)
        elif tag == b"fdAT":
            seq.append(struct.unpack(">I", body[:4])[0])
            images.append(body[4:])
        elif tag == b"IDAT":
            images.append(body)
    assert seq == list(range(5))
    for k, z in enumerate(images):
        raw = np.frombuffer(zlib.decompress(z), np.uint8).reshape(5, 1 + 21)
        assert not raw[:, 0].any() and np.array_equal(raw[:, 1:].reshape(5, 7, 3), frames[k])
    with pytest.raises(ValueError):
        write_apng(str(path), frames[0])
    with pytest.raises(ValueError):
        write_apng(str(path), frames, fps=0)


def test_write_apng_decodes_with_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    frames = np.random.default_rng(1).integers(0, 256, size=(4, 6, 8, 3), dtype=np.uint8)
    path = tmp_path / "b.png"
    write_apng(str(path), frames)
    im = Image.open(str(path))
    assert getattr(im, "n_frames", 1) == 4
    for k in range(4):
        im.seek(k)
        assert np.array_equal(np.asarray(im.convert("RGB")), frames[k])


def test_contact_sheet_layout():
    frames = np.arange(5 * 2 * 3 * 3, dtype=np.uint8).reshape(5, 2, 3, 3)
    sheet = contact_sheet(frames, 2)
    assert sheet.shape == (3 * 2, 2 * 3, 3)
    for k in range(5):
        r, c = divmod(k, 2)
        assert np.array_equal(sheet[r * 2:(r + 1) * 2, c * 3:(c + 1) * 3], frames[k])
    assert not sheet[4:, 3:].any()
    assert np.array_equal(contact_sheet(frames[:1], 1), frames[0])
    with pytest.raises(ValueError):
        contact_sheet(frames, 0)
    with pytest.raises(ValueError):
        contact_sheet(frames[0], 2)


# ---- the switches -----------------------------------------------------------------------------------------------------------------
def test_cli_flags_default_off():
    import evaluate
    import train
    from ppo_car_amd.ppo import PPOConfig
    a = evaluate.parse_args(["--checkpoint", "m.dat"])
    assert a.video is None and a.video_envs == 4 and a.video_scale == 4 and a.video_fps == 30
    a = evaluate.parse_args(["--checkpoint", "m.dat", "--envs", "64", "--video", "o.png", "--video-envs", "2", "--video-scale", "8", "--video-fps", "15"])
    assert (a.video, a.video_envs, a.video_scale, a.video_fps) == ("o.png", 2, 8, 15)
    t = train.parse_args(["--run-name", "x"])
    assert t.video_every == 0 and t.video_envs == 4 and t.video_scale == 4
    t = train.parse_args(["--run-name", "x", "--video-every", "10", "--video-envs", "2"])
    assert t.video_every == 10 and t.video_envs == 2
    cfg = PPOConfig()
    assert cfg.video_every == 0 and cfg.video_envs == 4 and cfg.video_scale == 4


def test_value_errors():
    import evaluate
    from ppo_car_amd.evaluation import Evaluator
    from ppo_car_amd.ppo import PPOConfig
    from ppo_car_amd.renderer import frame_size
    with pytest.raises(ValueError, match="--envs"):
        evaluate.parse_args(["--checkpoint", "m.dat", "--video", "o.png"])
    with pytest.raises(ValueError, match="video-envs"):
        evaluate.parse_args(["--checkpoint", "m.dat", "--envs", "2", "--video", "o.png"])
    with pytest.raises(ValueError, match="video-scale"):
        evaluate.parse_args(["--checkpoint", "m.dat", "--envs", "8", "--video", "o.png", "--video-scale", "3"])
    # the Evaluator refuses before it creates anything (no GPU is touched)
    with pytest.raises(ValueError, match="video_envs"):
        Evaluator(None, TRACKS["track"], n_envs=4, video_envs=5)
    with pytest.raises(ValueError, match="scale"):
        Evaluator(None, TRACKS["track"], n_envs=4, video_envs=2, video_scale=3)
    with pytest.raises(ValueError):
        Evaluator(None, TRACKS["track"], n_envs=4, video_envs=2, video_every_step=0)
    with pytest.raises(ValueError):
        PPOConfig(video_every=-1)
    with pytest.raises(ValueError):
        PPOConfig(video_every=1, video_scale=3)
    with pytest.raises(ValueError):
        PPOConfig(video_every=1, eval_every=1, eval_envs=2, video_envs=4)
    with pytest.raises(ValueError):
        frame_size(3)
    assert frame_size(5) == (144, 256) and frame_size(8) == (90, 160)
    with pytest.raises(ValueError, match="render_mode"):
        pc.VecCarEnv(4, TRACKS["track"], render_mode="human")


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_exports_and_library():
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    for name in ("pc_render_background", "pc_render_frames"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _capi.EXPORTS
        assert getattr(_capi.lib, name) is not None
    for k, name in enumerate(("GRASS", "ROAD", "WALL", "GATE", "NEXT_GATE", "RAY", "HIT", "CAR", "COLORS")):
        assert re.search(rf"#define PC_RENDER_{name} {k}\b", hdr), name
        assert getattr(_capi, "PC_RENDER_" + name) == k
    assert _capi.PC_RENDER_SCALES == SCALES and DEFAULT_PALETTE.shape == (_capi.PC_RENDER_COLORS, 3)


def test_null_arguments_are_refused_without_a_handle():
    P = 4096      # a non-NULL address: the calls are refused before anything is dereferenced
    lib = _capi.lib
    assert lib.pc_render_background(None, 2, P, None) == INV
    assert lib.pc_render_frames(None, P, 18, None, None, 1, 2, P, None, P, None) == INV
