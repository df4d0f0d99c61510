"""Plain reference of pc_env_observe_poses: CarEnv._get_obs (car_env.py:569-597) and Car.check_collision (car_env.py:376-392)
of a bare pose, with numpy, math and the oracle's single-ray distance.  Slow and literal on purpose."""
import math

import numpy as np

from conftest import GOLDEN      # (first: it puts the repository root on sys.path)

import oracle  # noqa: E402

# the golden files the kernel is held to: (track, nominal rays) -- the ray menu (12, 17, 33) and a chain of more than 64 vertices
CONFIGS = (("track", 32), ("big_track", 12), ("big_track", 16), ("oval64", 16))
ROWS = 600      # rows per group: not a multiple of any group or wave size


def observe(px, py, vx, vy, rot, n, walls):
    """One pose -> (obs [6 + R] float32, collides bool).  rot: heading in degrees; n: Car's nominal num_rays."""
    step = 360 // n
    R = len(range(0, 360, step))                                                  # car_env.py:269
    o = np.zeros(6 + R, np.float32)
    o[0:4] = np.float32(px / 1280), np.float32(py / 720), np.float32(vx / 10.0), np.float32(vy / 10.0)      # :578-581
    o[4] = np.float32(math.cos(math.radians(rot)))                                # :584-588
    o[5] = np.float32(math.sin(math.radians(rot)))
    d = [oracle.ray_distance(px, py, rot + i * step, walls) for i in range(R)]    # Ray.get_distance, :186-213
    o[6:] = [np.float32(x / 1000.0) for x in d]                                   # :593-595
    collides = any(d[r] < 10.0 for r in range(0, n, n // 4))                      # :389-390
    return o, collides


def collision_margin(px, py, rot, n, walls):
    """How far, in pixels, the nearest of check_collision's rays is from its 10 px threshold: below MARGIN_PX (test_env_gpu.py) a
    float32-selector handle may decide the other way."""
    return min(abs(oracle.ray_distance(px, py, rot + r * (360 // n), walls) - 10.0) for r in range(0, n, n // 4))


def observe_many(px, py, vx, vy, rot, n, walls):
    rows = [observe(float(a), float(b), float(c), float(d), float(r), n, walls) for a, b, c, d, r in zip(px, py, vx, vy, rot)]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], bool)


_cache = {}


def golden_rows(track, n):
    """The first ROWS rows of the golden file's `long` and `short` groups, concatenated: the post-step poses, the turn counts they
    mean, the step's own observation and termination flag, and the wall margin.  Loaded once per file."""
    key = (track, n)
    if key not in _cache:
        g = np.load(f"{GOLDEN}/env_{track}_n{n}.npz")
        start_rot = float(g["reset_state"][4])
        out = {k: [] for k in ("px", "py", "vx", "vy", "rot", "obs", "terminated", "wall_margin")}
        for grp in ("long", "short"):
            for k in ("px", "py", "vx", "vy", "rot"):
                out[k].append(g[f"{grp}_post_{k}"].reshape(-1)[:ROWS])
            out["obs"].append(g[f"{grp}_step_obs"].reshape(-1, g[f"{grp}_step_obs"].shape[-1])[:ROWS])
            out["terminated"].append(g[f"{grp}_terminated"].reshape(-1)[:ROWS])
            out["wall_margin"].append(g[f"{grp}_wall_margin"].reshape(-1)[:ROWS])
        out = {k: np.concatenate(v) for k, v in out.items()}
        out["turns"] = np.rint((out["rot"] - start_rot) / 5.0).astype(np.int32)
        out["start_rot"] = start_rot
        out["walls"] = g["walls"]
        _cache[key] = out
    return _cache[key]
