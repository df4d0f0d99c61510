"""The drawing rule of pc_render_background / pc_render_frames (include/ppocar.h) in numpy int64 / float64: the
yardstick of tests/test_render_host.py and tests/test_render_gpu.py.  Vectorised per primitive over the frame's pixels; nothing here
is shared with the kernels."""
import math

import numpy as np

SCALES = (1, 2, 4, 5, 8, 10)
GRASS, ROAD, WALL, GATE, NEXT_GATE, RAY, HIT, CAR = range(8)
# grass, road, wall, gate, next gate, ray, hit disc, car
DEFAULT_PALETTE = np.array([(24, 24, 28), (58, 58, 66), (235, 235, 235), (60, 110, 60), (90, 230, 90), (70, 110, 200),
                            (250, 210, 70), (240, 80, 60)], np.uint8)


def Q(v):
    """float64 pixels -> quarter pixels: rint(v * 4.0), ties to even."""
    return np.rint(np.asarray(v, np.float64) * 4.0).astype(np.int64)


def half_width(nominal, scale):
    return max(nominal, 3 * scale)


def grid(scale):
    """The pixel centres in quarter pixels: (Px [1, W], Py [H, 1]) int64."""
    assert scale in SCALES
    W, H = 1280 // scale, 720 // scale
    return (4 * scale * np.arange(W, dtype=np.int64) + 2 * scale)[None, :], (4 * scale * np.arange(H, dtype=np.int64) + 2 * scale)[:, None]


def covers(Px, Py, A, B, h):
    """bool [H, W]: the segment (A, B) of half-width h (quarter pixels, ints) covers the pixel centre."""
    ax, ay, bx, by = int(A[0]), int(A[1]), int(B[0]), int(B[1])
    ex, ey = bx - ax, by - ay
    wx, wy = Px - ax, Py - ay
    L = ex * ex + ey * ey
    h2 = h * h
    near_a = wx * wx + wy * wy <= h2
    if L == 0:
        return near_a | np.zeros_like(Py, bool)
    u = wx * ex + wy * ey
    vx, vy = Px - bx, Py - by
    near_b = vx * vx + vy * vy <= h2
    cr = wx * ey - wy * ex
    return np.where(u <= 0, near_a, np.where(u >= L, near_b, cr * cr <= h2 * L))


def reference_background(walls, gates, scale):
    """walls [S, 4], gates [G, 4] float64 pixels (Track.geometry()) -> uint8 [2, H, W]: plane 0 GRASS / ROAD / WALL, plane 1 = 1 + the
    highest gate that covers the pixel (0: none)."""
    Px, Py = grid(scale)
    wq, gq = Q(walls).reshape(-1, 4), Q(gates).reshape(-1, 4)
    crossings = np.zeros((Py.shape[0], Px.shape[1]), np.int64)
    wall = np.zeros(crossings.shape, bool)
    hw, hg = half_width(10, scale), half_width(10, scale)
    for ax, ay, bx, by in wq.tolist():
        ex, ey = bx - ax, by - ay
        cr = (Px - ax) * ey - (Py - ay) * ex
        straddles = (ay > Py) != (by > Py)
        right = (cr < 0) if ey > 0 else (cr > 0)
        crossings += straddles & right
        wall |= covers(Px, Py, (ax, ay), (bx, by), hw)
    layer = np.where(wall, WALL, np.where(crossings & 1 == 1, ROAD, GRASS)).astype(np.uint8)
    plane = np.zeros(crossings.shape, np.uint8)
    for g, (ax, ay, bx, by) in enumerate(gq.tolist()):
        plane[covers(Px, Py, (ax, ay), (bx, by), hg)] = g + 1
    return np.stack([layer, plane])


def ray_directions(num_rays_nominal):
    """[(cos, sin)] of radians(i * step), step = 360 // n (car_env.py:269), through math (libm)."""
    step = 360 // num_rays_nominal
    return [(math.cos(math.radians(a)), math.sin(math.radians(a))) for a in range(0, 360, step)]


def frame_is_dynamic(o):
    """The guards: does the row draw its rays and its car?"""
    o = np.asarray(o, np.float32)
    if not all(np.isfinite(o[k]) for k in (0, 1, 4, 5)):
        return False
    x, y = np.float64(o[0]) * 1280.0, np.float64(o[1]) * 720.0
    return bool(abs(np.float64(o[4])) <= 1.0 and abs(np.float64(o[5])) <= 1.0 and -1024.0 <= x <= 2304.0 and -1024.0 <= y <= 1744.0)


def reference_frames(walls, gates, obs, next_gate, num_rays_nominal, scale, palette=None, background=None):
    """obs [M, 6 + R] float32 rows on ONE track; next_gate [M] ints or None -> uint8 [M, H, W, 3].  background: a
    reference_background(walls, gates, scale) computed before (shared between calls), or None."""
    pal = DEFAULT_PALETTE if palette is None else np.asarray(palette, np.uint8)
    bg = reference_background(walls, gates, scale) if background is None else background
    gq = Q(gates).reshape(-1, 4)
    Px, Py = grid(scale)
    dirs = ray_directions(num_rays_nominal)
    obs = np.asarray(obs, np.float32)
    out = np.empty((len(obs),) + bg.shape[1:] + (3,), np.uint8)
    h_ray, h_car, h_gate = half_width(2, scale), half_width(24, scale), half_width(10, scale)
    for m, o in enumerate(obs):
        dyn = frame_is_dynamic(o)
        ng = int(next_gate[m]) if (next_gate is not None and dyn) else None
        col = bg[0].copy()
        col[(bg[1] != 0) & ((bg[1].astype(np.int64) - 1 >= ng) if ng is not None else True)] = GATE
        if dyn:
            if ng is not None and 0 <= ng < len(gq):
                col[covers(Px, Py, gq[ng, :2], gq[ng, 2:], h_gate)] = NEXT_GATE
            x, y = np.float64(o[0]) * 1280.0, np.float64(o[1]) * 720.0
            c, s = np.float64(o[4]), np.float64(o[5])
            A = (int(Q(x)), int(Q(y)))
            ends = []
            for i, (ci, si) in enumerate(dirs):
                dx, dy = c * ci - s * si, s * ci + c * si
                e = np.float64(o[6 + i])
                d = 1000.0 * e if np.isfinite(e) else np.float64(0.0)
                d = min(max(d, 0.0), 1000.0)
                ends.append((int(Q(x + d * dx)), int(Q(y + d * dy))))
            for B in ends:
                col[covers(Px, Py, A, B, h_ray)] = RAY
            for B in ends:
                col[covers(Px, Py, B, B, 20)] = HIT
            col[covers(Px, Py, (int(Q(x - 8.0 * c)), int(Q(y - 8.0 * s))), (int(Q(x + 14.0 * c)), int(Q(y + 14.0 * s))), h_car)] = CAR
        out[m] = pal[col]
    return out
