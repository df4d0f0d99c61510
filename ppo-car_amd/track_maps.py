"""Track telemetry maps: where on the track the cars drive, how fast, and where they crash -- per cell of cell_px x cell_px pixels
and per track, accumulated on the device by K16 (include/ppocar.h pc_track_maps) from observation rows that are already there.

counts [n_tracks, 3, GH, GW] int64 (GW = 1280 // cell_px, GH = 720 // cell_px): plane 0 VISITS (samples whose car was in the cell),
1 SPEED (the sum of their speeds in units of max_speed / 1024), 2 CRASHES (samples whose step terminated; the cell is the one of the
last observation BEFORE the hit).  update() only enqueues and only reads its arguments: a run computes the same bits with or without
it.  Every add is an integer add, so the counts do not depend on the launch geometry or on the order of arrival."""
import os

import numpy as np
import torch

from ._capi import (PC_EPISODE_BUFFER, PC_EPISODE_STEPS, PC_FIRST_ROWS, PC_MAP_CELLS, PC_MAP_CRASHES, PC_MAP_PLANES, PC_MAP_SPEED,
                    PC_MAP_SPEED_UNIT, PC_MAP_VISITS, check, lib)

WIDTH, HEIGHT, MAX_SPEED = 1280, 720, 10.0       # the frame (car_env.py:578-579) and the speed limit per axis in px per step (:580-581)
PLANE_NAMES = ("visits", "mean_speed", "crashes")


class TrackMaps:
    def __init__(self, n_tracks=1, cell_px=8, device="cuda"):
        if not 1 <= int(n_tracks) <= 256:
            raise ValueError(f"TrackMaps: n_tracks must be 1 .. 256, not {n_tracks!r}")
        if cell_px not in PC_MAP_CELLS:
            raise ValueError(f"TrackMaps: cell_px must be one of {PC_MAP_CELLS}, not {cell_px!r}")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_tracks, self.cell_px = int(n_tracks), int(cell_px)
        self.grid = (HEIGHT // self.cell_px, WIDTH // self.cell_px)         # (GH, GW)
        self.counts = torch.zeros(self.n_tracks, PC_MAP_PLANES, *self.grid, dtype=torch.int64, device=self.device)

    def clear(self):
        self.counts.zero_()

    def _rows(self, t, n, what, dtype=torch.float32):
        if not (t.is_cuda and t.device == self.device and t.dtype == dtype and t.is_contiguous() and t.numel() == n):
            raise ValueError(f"TrackMaps.update: {what} must be a contiguous {dtype} tensor of {n} elements on {self.device}, got "
                             f"{tuple(t.shape)} {t.dtype} {t.device}")
        return t.data_ptr()

    def update(self, obs, term, trunc, last_term=None, last_trunc=None, layout=PC_EPISODE_BUFFER, track_id=None, first_state=None):
        """obs [T, N, D], term / trunc [T, N] float32 in pc_first_episodes' two layouts (PC_EPISODE_BUFFER: step t's flags in row t + 1,
        step T - 1's in last_term / last_trunc [N]; PC_EPISODE_STEPS: flags[t] belong to step t); row t of obs is the observation the
        policy acted on at step t.  track_id [N] uint8 on the device (None: track 0).  first_state: pc_first_episodes' [8, N] float64
        state BEFORE this window's scan -- only the first episodes are counted.  Enqueues one launch on the current stream."""
        if self.device.type != "cuda":
            raise RuntimeError("TrackMaps.update runs the HIP kernel: the maps must live on a GPU")
        if layout not in (PC_EPISODE_BUFFER, PC_EPISODE_STEPS):
            raise ValueError(f"TrackMaps.update: layout must be PC_EPISODE_BUFFER or PC_EPISODE_STEPS, not {layout!r}")
        if obs.dim() != 3:
            raise ValueError(f"TrackMaps.update: obs must be [T, N, D], got {tuple(obs.shape)}")
        T, N, D = obs.shape
        buffer = layout == PC_EPISODE_BUFFER
        if buffer and (last_term is None or last_trunc is None):
            raise ValueError("TrackMaps.update: the Buffer layout needs last_term and last_trunc")
        check(lib.pc_track_maps(self.device.index, self._rows(obs, T * N * D, "obs"), D, self._rows(term, T * N, "term"),
                                self._rows(trunc, T * N, "trunc"), self._rows(last_term, N, "last_term") if buffer else None,
                                self._rows(last_trunc, N, "last_trunc") if buffer else None, T, N, layout,
                                None if track_id is None else self._rows(track_id, N, "track_id", torch.uint8), self.n_tracks,
                                self.cell_px,
                                None if first_state is None else self._rows(first_state, PC_FIRST_ROWS * N, "first_state", torch.float64),
                                self.counts.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream), "pc_track_maps")

    # ---- views (device tensors; no host synchronisation) -------------------------------------------------------------------------
    def visits(self, track=0):
        return self.counts[track, PC_MAP_VISITS]

    def mean_speed(self, track=0):
        """px per step; NaN where there are no visits."""
        c = self.counts[track]
        return c[PC_MAP_SPEED].to(torch.float64) / PC_MAP_SPEED_UNIT * MAX_SPEED / c[PC_MAP_VISITS].to(torch.float64)

    def crash_rate(self, track=0):
        """Crashes per visit; NaN where there are no visits."""
        c = self.counts[track]
        return c[PC_MAP_CRASHES].to(torch.float64) / c[PC_MAP_VISITS].to(torch.float64)

    # ---- checkpoints and files ------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"counts": self.counts.clone(), "cell_px": self.cell_px}

    def load_state_dict(self, sd):
        if int(sd["cell_px"]) != self.cell_px or tuple(sd["counts"].shape) != tuple(self.counts.shape):
            raise ValueError(f"TrackMaps.load_state_dict: maps of cell_px {int(sd['cell_px'])}, shape {tuple(sd['counts'].shape)} do not "
                             f"fit cell_px {self.cell_px}, shape {tuple(self.counts.shape)}")
        self.counts.copy_(sd["counts"])

    def save(self, path_prefix, tracks):
        """<path_prefix>.npz (counts, cell_px, the track names) and one PNG per track and plane, <path_prefix>_<track>_<plane>.png:
        visits and crashes on a logarithmic ramp, the mean speed on a linear one, walls and gates drawn over them.  tracks: the
        paths / Track objects of the planes, in order.  Synchronises (it fetches the counts).  Returns the files written."""
        from .env import Track
        from .render import heatmap, write_png
        if isinstance(tracks, (str, os.PathLike, Track)):
            tracks = [tracks]
        if len(tracks) != self.n_tracks:
            raise ValueError(f"TrackMaps.save: {len(tracks)} tracks for {self.n_tracks} plane sets")
        tr = [t if isinstance(t, Track) else Track(t) for t in tracks]
        names = [os.path.splitext(os.path.basename(os.fspath(t.path)))[0] if t.path is not None else f"track{k}" for k, t in enumerate(tr)]
        if len(set(names)) != len(names):
            names = [f"{k}_{n}" for k, n in enumerate(names)]
        counts = self.counts.cpu().numpy()
        os.makedirs(os.path.dirname(os.path.abspath(path_prefix)), exist_ok=True)
        files = [f"{path_prefix}.npz"]
        np.savez_compressed(files[0], counts=counts, cell_px=np.int64(self.cell_px), tracks=np.array(names))
        for k, t in enumerate(tr):
            walls, gates = t.geometry()
            v = counts[k, PC_MAP_VISITS].astype(np.float64)
            seen = v > 0
            with np.errstate(invalid="ignore", divide="ignore"):
                speed = np.where(seen, counts[k, PC_MAP_SPEED] / PC_MAP_SPEED_UNIT * MAX_SPEED / v, np.nan)
            planes = ((np.where(seen, v, np.nan), True), (speed, False),
                      (np.where(counts[k, PC_MAP_CRASHES] > 0, counts[k, PC_MAP_CRASHES], np.nan).astype(np.float64), True))
            for name, (values, log) in zip(PLANE_NAMES, planes):
                files.append(f"{path_prefix}_{names[k]}_{name}.png")
                write_png(files[-1], heatmap(values, walls, gates, log=log))
        return files
