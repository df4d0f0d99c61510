"""Policy landscape: what the policy would do, and what the critic expects, at every spot of the track -- the spots the cars never
reach included.  Per track, the centre of every cell of the track maps' grid (TrackMaps: GW = 1280 // cell_px, GH = 720 // cell_px)
is observed at all 72 headings by K17 (include/ppocar.h pc_env_observe_poses) with the car driving where it points, and the greedy
policy step (pc_policy_act_greedy) runs on those observations.

value [n_tracks, 72, GH, GW] float32 (the critic), action [.., 72, GH, GW] uint8 (the first argmax of the logits), drivable
[.., 72, GH, GW] bool (Car.check_collision is false at the pose).  Heading index t means the track's start angle + 5 t degrees.
compute() only enqueues (observe, act, two copies per chunk of at most 2^18 poses), draws no random number and writes nothing
but its own tensors: a training run computes the same bits with or without it.

survival(horizon) and lookahead() ask what happens from each pose, by stepping CLONES of the grid poses with K20 (pc_env_step_poses;
nothing is committed to any env): survived [n_tracks, 72, GH, GW] int16, the steps the greedy policy completes without hitting a wall;
safe_actions uint8, greedy_crashes and avoidable bool, the one-step look-ahead of all 9 actions.  They exist once their call has run.

viability(depth) asks the same of all 9 actions `depth` steps deep with ONE K21 launch per chunk (pc_env_safe_actions: the exhaustive
search on the device, no observation computed): viable [n_tracks, 72, GH, GW] uint16, bit a set iff action a can still avoid a crash
within `depth` steps; doomed and avoidable_late bool."""
import os

import numpy as np
import torch

from ._capi import PC_MAP_CELLS

WIDTH, HEIGHT, MAX_SPEED = 1280, 720, 10.0       # the frame (car_env.py:578-579) and the speed limit per axis in px per step (:580-581)
HEADINGS, TURN_DEG = 72, 5.0                     # Car.move_car turns by 5 degrees (car_env.py:440-442): 72 headings
CHUNK = 1 << 18                                  # poses per observe / act launch pair
NO_ACTION = 255                                  # action_at_best() where no heading is drivable


def grid_poses(start_angle, cell_px, speed):
    """The poses of one track, as float64 / int32 numpy arrays of 72 * GH * GW entries in [heading][cy][cx] order: the cell centres
    ((cx + 0.5) * cell_px, (cy + 0.5) * cell_px), turns 0 .. 71, and the velocity speed * max_speed along the heading start_angle +
    5 * turns degrees (cosine and sine in float64 on the host).  Returns px, py, vx, vy, turns."""
    GH, GW = HEIGHT // cell_px, WIDTH // cell_px
    turns = np.arange(HEADINGS, dtype=np.int32)
    a = np.radians(np.float64(start_angle) + TURN_DEG * turns.astype(np.float64))
    shape = (HEADINGS, GH, GW)
    px = np.broadcast_to(((np.arange(GW, dtype=np.float64) + 0.5) * cell_px)[None, None, :], shape)
    py = np.broadcast_to(((np.arange(GH, dtype=np.float64) + 0.5) * cell_px)[None, :, None], shape)
    vx = np.broadcast_to((np.float64(speed) * MAX_SPEED * np.cos(a))[:, None, None], shape)
    vy = np.broadcast_to((np.float64(speed) * MAX_SPEED * np.sin(a))[:, None, None], shape)
    tn = np.broadcast_to(turns[:, None, None], shape)
    return tuple(np.ascontiguousarray(x).reshape(-1) for x in (px, py, vx, vy, tn))


def best_value(value, drivable):
    """[72, GH, GW] -> [GH, GW]: the largest value over the drivable headings, NaN where no heading is drivable."""
    v = torch.where(drivable, value, torch.full_like(value, float("-inf"))).amax(0)
    return torch.where(drivable.any(0), v, torch.full_like(v, float("nan")))


def best_turn(value, drivable):
    """[72, GH, GW] -> [GH, GW] int64: the first heading index at that maximum; -1 where no heading is drivable."""
    t = torch.where(drivable, value, torch.full_like(value, float("-inf"))).argmax(0)
    return torch.where(drivable.any(0), t, torch.full_like(t, -1))


class PolicyLandscape:
    def __init__(self, agent, tracks, num_rays, cell_px=8, speed=0.5, dtype="f32", device="cuda", envs=None):
        """agent: ppo_car_amd.Agent (its act(obs, greedy=True)); tracks: one path / Track or a list; num_rays: Car's nominal ray
        count, which fixes the agent's input width.  The landscape owns a one-env handle, used for its track tables only.  (envs: an
        object with observe_poses(), step_poses(), obs_dim and _tracks to use in its place -- the host tests' stand-in.)"""
        if cell_px not in PC_MAP_CELLS:
            raise ValueError(f"PolicyLandscape: cell_px must be one of {PC_MAP_CELLS}, not {cell_px!r}")
        if not 0.0 <= float(speed) <= 1.0:
            raise ValueError(f"PolicyLandscape: speed is a fraction of max_speed, 0 .. 1, not {speed!r}")
        self.agent, self.cell_px, self.speed = agent, int(cell_px), float(speed)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._own_envs = envs is None
        if envs is None:
            from .env import VecCarEnv
            envs = VecCarEnv(1, tracks, num_rays=num_rays, device=self.device, dtype=dtype)
        self.envs = envs
        self.tracks = list(envs._tracks)
        self.n_tracks = len(self.tracks)
        self.grid = (HEIGHT // self.cell_px, WIDTH // self.cell_px)         # (GH, GW)
        self.poses_per_track = HEADINGS * self.grid[0] * self.grid[1]
        # the poses of every track, [n_tracks * poses_per_track] each: constant, uploaded once
        cols = [grid_poses(t.start_angle, self.cell_px, self.speed) for t in self.tracks]
        self._px, self._py, self._vx, self._vy, self._turns = (
            torch.from_numpy(np.concatenate([c[i] for c in cols])).to(self.device) for i in range(5))
        self._track_id = torch.arange(self.n_tracks, dtype=torch.uint8).repeat_interleave(self.poses_per_track).to(self.device)
        shape = (self.n_tracks, HEADINGS, *self.grid)
        self.value = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.action = torch.zeros(shape, dtype=torch.uint8, device=self.device)
        self.drivable = torch.zeros(shape, dtype=torch.bool, device=self.device)
        n = min(CHUNK, self.n_tracks * self.poses_per_track)
        self._obs = torch.empty(n, envs.obs_dim, dtype=torch.float32, device=self.device)
        self._act = torch.empty(n, dtype=torch.int64, device=self.device)
        self._logprob = torch.empty(n, dtype=torch.float32, device=self.device)
        self._collides = torch.empty(n, dtype=torch.uint8, device=self.device)
        # survival() / lookahead(): created by the call that fills them
        self.survived = self.survival_horizon = self.safe_actions = self.greedy_crashes = self.avoidable = None
        self.viable = self.viability_depth = self.doomed = self.avoidable_late = None      # viability()
        self._computed = False
        self._step_bufs = None

    def poses(self):
        """(px, py, vx, vy, turns, track_id): the device tensors compute() evaluates, [n_tracks * 72 * GH * GW] each."""
        return self._px, self._py, self._vx, self._vy, self._turns, self._track_id

    def compute(self):
        """Fill value / action / drivable from the agent's current weights.  Per chunk of at most 2^18 poses: one
        pc_env_observe_poses launch and one pc_policy_act_greedy launch (the weights are packed once, ahead of the first).
        Enqueues on the current stream; no synchronisation, no random draw.  Returns self."""
        total = self.n_tracks * self.poses_per_track
        value, action, drivable = self.value.view(-1), self.action.view(-1), self.drivable.view(-1)
        for lo in range(0, total, CHUNK):
            hi = min(lo + CHUNK, total)
            n = hi - lo
            obs, collides = self._obs[:n], self._collides[:n]
            self.envs.observe_poses(self._px[lo:hi], self._py[lo:hi], self._turns[lo:hi], vx=self._vx[lo:hi], vy=self._vy[lo:hi],
                                    track_id=self._track_id[lo:hi], out=obs, collides=collides)
            self.agent.act(obs, out_action=self._act[:n], out_logprob=self._logprob[:n], out_value=value[lo:hi], greedy=True,
                           repack=lo == 0)
            action[lo:hi].copy_(self._act[:n])
            torch.eq(collides, 0, out=drivable[lo:hi])
        self._computed = True
        return self

    # ---- what happens from each pose (K20, pc_env_step_poses: steps of clones of the grid poses; nothing is committed anywhere) -----
    def _chunk_state(self, lo, hi):
        """Fresh clones of the chunk's grid poses plus zero next_gate / time_step: the tensors step_poses() updates in place."""
        z = torch.zeros(hi - lo, dtype=torch.int32, device=self.device)
        return [t[lo:hi].clone() for t in (self._px, self._py, self._vx, self._vy, self._turns)] + [z, z.clone()]

    def _step_out(self, n):
        if self._step_bufs is None:
            m = self._obs.shape[0]
            u8 = lambda: torch.zeros(m, dtype=torch.uint8, device=self.device)
            self._step_bufs = (torch.zeros(m, dtype=torch.float32, device=self.device), u8(), u8(), u8(),
                               torch.zeros(m, dtype=torch.float32, device=self.device))
        rew, term, trunc, gate, val = self._step_bufs
        return (self._obs[:n], rew[:n], term[:n], trunc[:n], gate[:n]), val[:n]

    def survival(self, horizon=64):
        """Fill survived [n_tracks, 72, GH, GW] int16: how many steps the greedy policy completes from the pose without hitting a wall --
        0 at a pose that is not drivable, `horizon` if it never crashes.  Per chunk of at most 2^18 poses: one pc_env_observe_poses, then
        `horizon` times one pc_policy_act_greedy and one pc_env_step_poses on clones of the grid poses, active = still alive.  1 <= horizon
        <= 999: the time limit cannot fire.  No random draw, no synchronisation; writes nothing but its own tensors.  Returns self."""
        horizon = int(horizon)
        if not 1 <= horizon <= 999:
            raise ValueError(f"PolicyLandscape.survival: horizon must be in 1 .. 999, not {horizon!r}")
        total = self.n_tracks * self.poses_per_track
        if self.survived is None:
            self.survived = torch.zeros((self.n_tracks, HEADINGS, *self.grid), dtype=torch.int16, device=self.device)
        self.survived.zero_()
        self.survival_horizon = horizon
        survived = self.survived.view(-1)
        for lo in range(0, total, CHUNK):
            hi = min(lo + CHUNK, total)
            n = hi - lo
            px, py, vx, vy, turns, next_gate, time_step = self._chunk_state(lo, hi)
            out, val = self._step_out(n)
            obs, collides, tid = out[0], self._collides[:n], self._track_id[lo:hi]
            self.envs.observe_poses(px, py, turns, vx=vx, vy=vy, track_id=tid, out=obs, collides=collides)
            torch.eq(collides, 0, out=self.drivable.view(-1)[lo:hi])      # (what compute() writes there)
            alive = (collides == 0).to(torch.uint8)
            out[2].zero_()
            for s in range(horizon):
                self.agent.act(obs, out_action=self._act[:n], out_logprob=self._logprob[:n], out_value=val, greedy=True,
                               repack=lo == 0 and s == 0)
                self.envs.step_poses(px, py, vx, vy, turns, self._act[:n], next_gate=next_gate, time_step=time_step, track_id=tid,
                                     active=alive, out=out)
                alive &= out[2] == 0
                survived[lo:hi] += alive
        return self

    def lookahead(self):
        """One-step look-ahead from every grid pose, after compute() (RuntimeError otherwise): per chunk and for each of the 9 actions one
        pc_env_step_poses on a clone of the chunk.  safe_actions uint8: how many actions' step does not terminate (0 where the pose is not
        drivable); greedy_crashes bool: the pose is drivable and the step under compute()'s greedy action terminates; avoidable =
        greedy_crashes & (safe_actions > 0).  No random draw, no synchronisation.  Returns self."""
        if not self._computed:
            raise RuntimeError("PolicyLandscape.lookahead() reads the action and drivable maps: call compute() first")
        total = self.n_tracks * self.poses_per_track
        shape = (self.n_tracks, HEADINGS, *self.grid)
        self.safe_actions = torch.zeros(shape, dtype=torch.uint8, device=self.device)
        self.greedy_crashes = torch.zeros(shape, dtype=torch.bool, device=self.device)
        safe, crashes = self.safe_actions.view(-1), self.greedy_crashes.view(-1)
        action, drivable = self.action.view(-1), self.drivable.view(-1)
        for lo in range(0, total, CHUNK):
            hi = min(lo + CHUNK, total)
            n = hi - lo
            out, _ = self._step_out(n)
            ok = drivable[lo:hi]
            active = ok.to(torch.uint8)
            for a in range(9):
                px, py, vx, vy, turns, next_gate, time_step = self._chunk_state(lo, hi)
                self._act[:n].fill_(a)
                self.envs.step_poses(px, py, vx, vy, turns, self._act[:n], next_gate=next_gate, time_step=time_step,
                                     track_id=self._track_id[lo:hi], active=active, out=out)
                term = out[2] != 0
                safe[lo:hi] += (ok & ~term).to(torch.uint8)
                crashes[lo:hi] |= ok & term & (action[lo:hi] == a)
        self.avoidable = self.greedy_crashes & (self.safe_actions > 0)
        return self

    def viability(self, depth=3):
        """Which actions can still avoid a crash within `depth` steps (1 .. 4) from every grid pose, after compute() (RuntimeError
        otherwise): per chunk one pc_env_safe_actions with active = drivable.  viable uint16: bit a is set iff action a is safe at `depth`
        (VecCarEnv.safe_actions), 0 where the pose is not drivable; doomed bool: drivable and no bit set; avoidable_late bool: compute()'s
        greedy action has its bit clear and some other bit is set.  At depth 1 the bit count is lookahead()'s safe_actions and
        avoidable_late its avoidable.  No random draw, no synchronisation; writes nothing but its own tensors.  Returns self."""
        if not self._computed:
            raise RuntimeError("PolicyLandscape.viability() reads the action and drivable maps: call compute() first")
        total = self.n_tracks * self.poses_per_track
        shape = (self.n_tracks, HEADINGS, *self.grid)
        self.viable = torch.zeros(shape, dtype=torch.uint16, device=self.device)
        self.viability_depth = int(depth)
        viable, drivable = self.viable.view(-1), self.drivable.view(-1)
        bit = torch.arange(9, dtype=torch.int32, device=self.device)
        safe = torch.zeros(min(CHUNK, total), 9, dtype=torch.uint8, device=self.device)
        for lo in range(0, total, CHUNK):
            hi = min(lo + CHUNK, total)
            ok = drivable[lo:hi]
            self.envs.safe_actions(self._px[lo:hi], self._py[lo:hi], self._vx[lo:hi], self._vy[lo:hi], self._turns[lo:hi], depth=int(depth),
                                   track_id=self._track_id[lo:hi], active=ok.to(torch.uint8), out=safe[:hi - lo])
            bits = (safe[:hi - lo].to(torch.int32) << bit).sum(1, dtype=torch.int32)
            viable[lo:hi].copy_(torch.where(ok, bits, torch.zeros_like(bits)))      # (an inactive row's bytes were not written)
        v = self.viable.to(torch.int32)
        self.doomed = self.drivable & (v == 0)
        self.avoidable_late = (((v >> self.action.to(torch.int32)) & 1) == 0) & (v != 0)
        return self

    def viable_count(self, track=0):
        """[GH, GW] float32: the most safe actions over the drivable headings; NaN where no heading is drivable."""
        v = self.viable[track].to(torch.int32)
        count = ((v.unsqueeze(-1) >> torch.arange(9, dtype=torch.int32, device=self.device)) & 1).sum(-1)
        return best_value(count.to(torch.float32), self.drivable[track])

    def best_survival(self, track=0):
        """[GH, GW] float32: the most steps survived over the drivable headings; NaN where no heading is drivable."""
        return best_value(self.survived[track].to(torch.float32), self.drivable[track])

    # ---- reductions over the headings (device tensors; no host synchronisation) -------------------------------------------------
    def best_value(self, track=0):
        """[GH, GW] float32: the critic's value at the best drivable heading; NaN where no heading is drivable."""
        return best_value(self.value[track], self.drivable[track])

    def best_heading(self, track=0):
        """[GH, GW] float64: that heading in degrees, the track's start angle + 5 * its index; NaN where no heading is drivable."""
        t = best_turn(self.value[track], self.drivable[track])
        deg = self.tracks[track].start_angle + TURN_DEG * t.to(torch.float64)
        return torch.where(t >= 0, deg, torch.full_like(deg, float("nan")))

    def action_at_best(self, track=0):
        """[GH, GW] uint8: the greedy action at that heading; NO_ACTION (255) where no heading is drivable."""
        t = best_turn(self.value[track], self.drivable[track])
        a = self.action[track].gather(0, t.clamp(min=0).unsqueeze(0)).squeeze(0)
        return torch.where(t >= 0, a, torch.full_like(a, NO_ACTION))

    # ---- files -------------------------------------------------------------------------------------------------------------------
    def save(self, path_prefix):
        """<path_prefix>_landscape.npz (value, action, drivable, best_value, best_heading, action_at_best, cell_px, speed, the track
        names) and one PNG per track, <path_prefix>_landscape_<track>.png: best_value on a linear ramp, walls and gates drawn over
        it.  Whichever of survived (with survival_horizon), safe_actions, greedy_crashes, avoidable exist are added to the .npz, and
        with survived one <path_prefix>_survival_<track>.png per track: the most steps survived over the drivable headings, linear
        ramp.  Synchronises (it fetches the tensors).  Returns the files written."""
        from .render import heatmap, write_png
        names = [os.path.splitext(os.path.basename(os.fspath(t.path)))[0] if getattr(t, "path", None) is not None else f"track{k}"
                 for k, t in enumerate(self.tracks)]
        if len(set(names)) != len(names):
            names = [f"{k}_{n}" for k, n in enumerate(names)]
        os.makedirs(os.path.dirname(os.path.abspath(path_prefix)), exist_ok=True)
        best = np.stack([self.best_value(k).cpu().numpy() for k in range(self.n_tracks)])
        files = [f"{path_prefix}_landscape.npz"]
        extra = {k: getattr(self, k).cpu().numpy() for k in ("survived", "safe_actions", "greedy_crashes", "avoidable", "viable", "doomed",
                                                             "avoidable_late")
                 if getattr(self, k) is not None}      # (survival() / lookahead() / viability(): only what was computed)
        if self.survived is not None:
            extra["survival_horizon"] = np.int64(self.survival_horizon)
        if self.viable is not None:
            extra["viability_depth"] = np.int64(self.viability_depth)
        np.savez_compressed(files[0], value=self.value.cpu().numpy(), action=self.action.cpu().numpy(), drivable=self.drivable.cpu().numpy(),
                            best_value=best, best_heading=np.stack([self.best_heading(k).cpu().numpy() for k in range(self.n_tracks)]),
                            action_at_best=np.stack([self.action_at_best(k).cpu().numpy() for k in range(self.n_tracks)]),
                            cell_px=np.int64(self.cell_px), speed=np.float64(self.speed), tracks=np.array(names), **extra)
        for k, t in enumerate(self.tracks):
            walls, gates = t.geometry()
            files.append(f"{path_prefix}_landscape_{names[k]}.png")
            write_png(files[-1], heatmap(best[k].astype(np.float64), walls, gates, log=False))
        if self.survived is not None:      # the most steps survived over the drivable headings, on a linear ramp
            for k, t in enumerate(self.tracks):
                walls, gates = t.geometry()
                files.append(f"{path_prefix}_survival_{names[k]}.png")
                write_png(files[-1], heatmap(self.best_survival(k).cpu().numpy().astype(np.float64), walls, gates, log=False))
        if self.viable is not None:        # how many actions are still safe, the most over the drivable headings, on a linear ramp
            for k, t in enumerate(self.tracks):
                walls, gates = t.geometry()
                files.append(f"{path_prefix}_viability_{names[k]}.png")
                write_png(files[-1], heatmap(self.viable_count(k).cpu().numpy().astype(np.float64), walls, gates, log=False))
        return files

    def close(self):
        if self._own_envs and self.envs is not None:
            self.envs.close()
        self.envs = None
