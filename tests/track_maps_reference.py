"""Plain numpy reference of pc_track_maps (include/ppocar.h): float32 cell arithmetic, float64 speed, int64 counters.  A helper of the
track-map tests, like first_episode_reference.py; no GPU, no library.

maps [n_tracks, 3, GH, GW] int64 (GW = 1280 // cell_px, GH = 720 // cell_px): plane 0 visits, 1 the sum of q = rint(speed * 1024),
2 crashes.  Row t of obs is the observation BEFORE step t; flags are taken in the STEP layout (flags[t] belong to step t):
buffer_flags() of first_episode_reference.py converts the Buffer layout."""
import numpy as np

VISITS, SPEED, CRASHES, PLANES = 0, 1, 2, 3
SPEED_UNIT = 1024
CELLS = (4, 5, 8, 10, 16, 20, 40, 80)
RUNNING = 0


def grid(cell_px):
    return 720 // cell_px, 1280 // cell_px          # (GH, GW)


def cell_of(o0, o1, cell_px):
    """(cx, cy) of float32 positions: ONE float32 multiply each, floor, clamp to the edge cells."""
    GH, GW = grid(cell_px)
    with np.errstate(over="ignore", invalid="ignore"):
        fx = np.floor(np.asarray(o0, np.float32) * np.float32(GW))
        fy = np.floor(np.asarray(o1, np.float32) * np.float32(GH))
    fx, fy = np.where(np.isnan(fx), np.float32(0), fx), np.where(np.isnan(fy), np.float32(0), fy)      # (such samples are skipped)
    return np.clip(fx, 0, GW - 1).astype(np.int64), np.clip(fy, 0, GH - 1).astype(np.int64)


def speed_q(o2, o3):
    """q = rint(sqrt(o2^2 + o3^2) * 1024) with the float32 inputs widened to float64 first (not finite, or above 9e18: 0)."""
    a, b = np.asarray(o2, np.float32).astype(np.float64), np.asarray(o3, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.sqrt(a * a + b * b) * float(SPEED_UNIT)
        ok = s < 9.0e18
        return np.where(ok, np.rint(np.where(ok, s, 0.0)), 0.0).astype(np.int64)


def track_maps_ref(obs, term, trunc, cell_px, n_tracks=1, track_id=None, first_state=None, maps=None):
    """obs [T, N, D], term / trunc [T, N] in the STEP layout -> maps (accumulated into a copy of `maps`, or from zero).
    first_state [8, N]: pc_first_episodes' state BEFORE the window (only row 4 is read)."""
    obs = np.asarray(obs, np.float32)
    T, N, _ = obs.shape
    GH, GW = grid(cell_px)
    out = np.zeros((n_tracks, PLANES, GH, GW), np.int64) if maps is None else np.array(maps, np.int64)
    tid = np.zeros(N, np.int64) if track_id is None else np.asarray(track_id).astype(np.int64)
    counted = np.ones(N, bool) if first_state is None else np.asarray(first_state)[4] == RUNNING
    counted = counted & (tid < n_tracks)
    cx, cy = cell_of(obs[..., 0], obs[..., 1], cell_px)
    q = speed_q(obs[..., 2], obs[..., 3])
    finite = np.isfinite(obs[..., 0]) & np.isfinite(obs[..., 1])
    for t in range(T):
        use = counted & finite[t]
        k, y, x = tid[use], cy[t][use], cx[t][use]
        np.add.at(out, (k, VISITS, y, x), 1)
        np.add.at(out, (k, SPEED, y, x), q[t][use])
        crash = use & (np.asarray(term[t]) != 0)
        np.add.at(out, (tid[crash], CRASHES, cy[t][crash], cx[t][crash]), 1)
        if first_state is not None:         # the closing step itself counted; everything after it does not
            counted = counted & (np.asarray(term[t]) == 0) & (np.asarray(trunc[t]) == 0)
    return out
