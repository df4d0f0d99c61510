"""Software rasteriser for one env's state (the role of CarEnv.__render_frame, car_env.py:766-807, and
of log_video's frames, train.py:23-50, without pygame / cv2): walls, reward gates (the next one highlighted), the car as
a heading arrow and its rays out to the distances the observation reports.  numpy only; PNG written with zlib."""
import struct
import zlib

import numpy as np

WIDTH, HEIGHT = 1280, 720
COLORS = {"background": (24, 24, 28), "wall": (235, 235, 235), "gate": (60, 110, 60), "next_gate": (90, 230, 90),
          "ray": (70, 110, 200), "car": (240, 80, 60)}
# heatmap's fixed ramp, low to high (equally spaced stops, linear in between)
RAMP = ((40, 40, 110), (40, 130, 200), (60, 190, 120), (240, 220, 70), (230, 60, 40))


def _line(img, x0, y0, x1, y1, color):
    h, w, _ = img.shape
    n = int(max(abs(x1 - x0), abs(y1 - y0))) + 1
    xs = np.rint(np.linspace(x0, x1, n)).astype(np.int64)
    ys = np.rint(np.linspace(y0, y1, n)).astype(np.int64)
    ok = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    img[ys[ok], xs[ok]] = color


def rasterise(walls, gates, px, py, rot_deg, ray_obs, next_gate=0, num_rays_nominal=None, size=(640, 360)):
    """walls / gates: [n, 4] segments in the 1280 x 720 frame (Track.geometry()); ray_obs: the observation's ray part
    (distance / 1000, car_env.py:593); rot_deg: heading in degrees.  Returns uint8 [H, W, 3]."""
    w, h = size
    sx, sy = w / WIDTH, h / HEIGHT
    img = np.empty((h, w, 3), np.uint8)
    img[:] = COLORS["background"]
    for i, g in enumerate(np.asarray(gates)):
        _line(img, g[0] * sx, g[1] * sy, g[2] * sx, g[3] * sy, COLORS["next_gate" if i == next_gate else "gate"])
    R = len(ray_obs)
    n = num_rays_nominal or R
    step = 360 // n                                            # car_env.py:269
    for i, d in enumerate(np.asarray(ray_obs, np.float64) * 1000.0):
        a = np.radians(rot_deg + i * step)
        _line(img, px * sx, py * sy, (px + d * np.cos(a)) * sx, (py + d * np.sin(a)) * sy, COLORS["ray"])
    for s in np.asarray(walls):
        _line(img, s[0] * sx, s[1] * sy, s[2] * sx, s[3] * sy, COLORS["wall"])
    a = np.radians(rot_deg)
    c, s_ = np.cos(a), np.sin(a)
    nose = (px + 14 * c, py + 14 * s_)
    for lx, ly in ((-8, -6), (-8, 6)):                         # a small arrow: two tail points to the nose, and the base
        _line(img, (px + lx * c - ly * s_) * sx, (py + lx * s_ + ly * c) * sy, nose[0] * sx, nose[1] * sy, COLORS["car"])
    _line(img, (px - 8 * c + 6 * s_) * sx, (py - 8 * s_ - 6 * c) * sy, (px - 8 * c - 6 * s_) * sx, (py - 8 * s_ + 6 * c) * sy,
          COLORS["car"])
    return img


def heatmap(values, walls, gates, size=(1280, 720), log=True):
    """values [GH, GW]: one number per cell of a grid over the 1280 x 720 frame (TrackMaps: visits, mean speed, crashes), coloured on
    the fixed ramp RAMP from the smallest to the largest value present (log: on a logarithmic scale, values <= 0 are no data); cells
    without data (NaN) keep the background colour.  Walls and gates ([n, 4] segments, Track.geometry()) are drawn over the cells.
    Returns uint8 [H, W, 3]."""
    w, h = size
    sx, sy = w / WIDTH, h / HEIGHT
    v = np.asarray(values, np.float64)
    gh, gw = v.shape
    has = np.isfinite(v) & ((v > 0) if log else True)
    cells = np.empty((gh, gw, 3), np.uint8)
    cells[:] = COLORS["background"]
    if has.any():
        x = np.log(v[has]) if log else v[has]
        lo, hi = x.min(), x.max()
        u = (x - lo) / (hi - lo) if hi > lo else np.full(x.shape, 0.5)
        ramp = np.asarray(RAMP, np.float64)
        pos = u * (len(ramp) - 1)
        i = np.minimum(pos.astype(np.int64), len(ramp) - 2)
        f = (pos - i)[:, None]
        cells[has] = np.rint(ramp[i] * (1.0 - f) + ramp[i + 1] * f).astype(np.uint8)
    ys = np.minimum(np.arange(h) * gh // h, gh - 1)
    xs = np.minimum(np.arange(w) * gw // w, gw - 1)
    img = cells[ys[:, None], xs[None, :]]
    for g in np.asarray(gates):
        _line(img, g[0] * sx, g[1] * sy, g[2] * sx, g[3] * sy, COLORS["gate"])
    for s in np.asarray(walls):
        _line(img, s[0] * sx, s[1] * sy, s[2] * sx, s[3] * sy, COLORS["wall"])
    return img


def write_png(path, img):
    """Minimal PNG encoder (8-bit RGB, one IDAT)."""
    h, w, _ = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


# ---- frames rendered on the device (renderer.py, pc_render_frames): the default palette, contact sheets, animated PNG ----------------
# [PC_RENDER_COLORS][3] in the order of include/ppocar.h's PC_RENDER_* indices: grass, road, wall, gate, next gate, ray, hit disc, car
# (COLORS plus a road fill and a hit-disc colour; the library's default when no palette is passed)
DEFAULT_PALETTE = np.array([COLORS["background"], (58, 58, 66), COLORS["wall"], COLORS["gate"], COLORS["next_gate"], COLORS["ray"],
                            (250, 210, 70), COLORS["car"]], np.uint8)


def contact_sheet(frames, cols):
    """frames uint8 [K, H, W, 3] -> one image of ceil(K / cols) rows x cols columns, frame k at row k // cols, column k % cols; cells
    past K are black."""
    frames = np.asarray(frames, np.uint8)
    if frames.ndim != 4 or frames.shape[3] != 3 or len(frames) < 1:
        raise ValueError(f"contact_sheet: frames must be [K >= 1, H, W, 3], got {frames.shape}")
    cols = int(cols)
    if cols < 1:
        raise ValueError(f"contact_sheet: cols must be >= 1, not {cols}")
    k, h, w, _ = frames.shape
    rows = (k + cols - 1) // cols
    sheet = np.zeros((rows * cols, h, w, 3), np.uint8)
    sheet[:k] = frames
    return sheet.reshape(rows, cols, h, w, 3).transpose(0, 2, 1, 3, 4).reshape(rows * h, cols * w, 3)


def write_apng(path, frames, fps=30):
    """Animated PNG (8-bit RGB, zlib only), frames uint8 [K, H, W, 3] played in a loop at `fps`: IHDR, acTL, then per frame an fcTL and
    its image -- the first in IDAT (a viewer without APNG support shows it), the others in fdAT -- with one running sequence number over
    the fcTL and fdAT chunks, then IEND."""
    frames = np.asarray(frames, np.uint8)
    if frames.ndim != 4 or frames.shape[3] != 3 or len(frames) < 1:
        raise ValueError(f"write_apng: frames must be [K >= 1, H, W, 3], got {frames.shape}")
    fps = int(fps)
    if not 1 <= fps <= 65535:
        raise ValueError(f"write_apng: fps must be 1 .. 65535, not {fps}")
    k, h, w, _ = frames.shape

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    out = [b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)), chunk(b"acTL", struct.pack(">II", k, 0))]
    seq = 0
    for i in range(k):
        # fcTL: sequence, width, height, x / y offset, delay = 1 / fps s, dispose none, blend source
        out.append(chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, 1, fps, 0, 0)))
        seq += 1
        rows = np.empty((h, 1 + 3 * w), np.uint8)
        rows[:, 0] = 0                                          # filter type none
        rows[:, 1:] = frames[i].reshape(h, 3 * w)
        data = zlib.compress(rows.tobytes(), 6)
        if i == 0:
            out.append(chunk(b"IDAT", data))
        else:
            out.append(chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(b"".join(out))
