"""Frames on the device: observation rows -> RGB frames through the hand-written rasteriser (pc_render_background / pc_render_frames,
include/ppocar.h; the role of CarEnv.render(), car_env.py:762-807, and of log_video's frames, train.py:23-50).  A frame is a pure
function of (observation row, track, next-gate index): any rollout or evaluation buffer can be rendered after the fact."""
import numpy as np
import torch

from ._capi import PC_RENDER_COLORS, PC_RENDER_SCALES, check, lib


def frame_size(scale):
    """(H, W) of a frame at `scale`; ValueError for a scale off PC_RENDER_SCALES."""
    if scale not in PC_RENDER_SCALES:
        raise ValueError(f"render scale must be one of {PC_RENDER_SCALES}, not {scale!r}")
    return 720 // scale, 1280 // scale


class Renderer:
    """Renders rows of `envs`' observation layout on `envs`' tracks.  Owns the static background image of the handle's tracks at
    `scale` (built by the first frames() call) and nothing else: the env state is neither read nor written.
    palette: uint8 [PC_RENDER_COLORS, 3] (render.DEFAULT_PALETTE's order) or None = the library's default."""

    def __init__(self, envs, scale=2, palette=None):
        self.H, self.W = frame_size(scale)
        self.envs, self.scale, self.device = envs, int(scale), envs.device
        self.palette = None
        if palette is not None:
            p = np.ascontiguousarray(palette, np.uint8)
            if p.shape != (PC_RENDER_COLORS, 3):
                raise ValueError(f"palette must be uint8 [{PC_RENDER_COLORS}, 3], got {p.shape}")
            self.palette = p
        self._background = None

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def background(self):
        """uint8 [n_tracks, 2, H, W] (device): plane 0 grass / road / wall, plane 1 = 1 + the gate that covers the pixel."""
        if self._background is None:
            bg = torch.empty(len(self.envs._tracks), 2, self.H, self.W, dtype=torch.uint8, device=self.device)
            check(lib.pc_render_background(self.envs._h, self.scale, bg.data_ptr(), self._stream()), "pc_render_background")
            self._background = bg
        return self._background

    def frames(self, obs, next_gate=None, track_id=None, out=None):
        """obs float32 [M, D] on the device, rows contiguous, any row stride >= D (e.g. buffer[:, n] of a [T, N, D] buffer);
        next_gate int32 [M] or None (all gates drawn plain); track_id uint8 [M] or None (track 0) -> uint8 [M, H, W, 3]."""
        D = self.envs.obs_dim
        if not (obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] == D and obs.shape[0] >= 1
                and obs.stride(1) == 1 and (obs.shape[0] == 1 or obs.stride(0) >= D)):
            raise ValueError(f"frames: obs must be a float32 CUDA tensor [M >= 1, {D}] with contiguous rows, got {tuple(obs.shape)} "
                             f"{obs.dtype} {obs.device} strides {tuple(obs.stride())}")
        M = obs.shape[0]
        ld = obs.stride(0) if M > 1 else D
        ptr = self.envs._ptr
        if out is None:
            out = torch.empty(M, self.H, self.W, 3, dtype=torch.uint8, device=self.device)
        check(lib.pc_render_frames(self.envs._h, obs.data_ptr(), ld, ptr(next_gate, torch.int32, M, "next_gate"),
                                   ptr(track_id, torch.uint8, M, "track_id"), M, self.scale, self.background().data_ptr(),
                                   self.palette.ctypes.data if self.palette is not None else None,
                                   ptr(out, torch.uint8, M * self.H * self.W * 3, "out"), self._stream()), "pc_render_frames")
        return out
