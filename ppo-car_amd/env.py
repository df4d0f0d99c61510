"""VecCarEnv -- the gymnasium vector-env surface train.py drives (reference train.py:138-142,
159-164,185,296), backed by the HIP env-step kernel through the C-ABI.  Tensors in, tensors out,
everything stays on the GPU; no host synchronisation in step()."""
import collections
import ctypes as C
import os

import numpy as np
import torch

from . import _capi
from ._capi import check, lib

# what VecCarEnv.step_poses returns (the stepped px, py, vx, vy, turns are the caller's own tensors, updated in place)
StepPoses = collections.namedtuple("StepPoses", "obs reward terminated truncated gate next_gate time_step")


class Track:
    """A loaded track (CarEnv.load_track, car_env.py:535-567).  Host-side only."""

    def __init__(self, path=None, *, walls=None, gates=None, start=None):
        h = C.c_void_p()
        if path is not None:
            # the reference prints "Track file not found" and returns None (car_env.py:624-628);
            # here a missing / malformed track is a hard error
            check(lib.pc_track_load_json(os.fsencode(path), C.byref(h)), f"pc_track_load_json({path!r})")
        else:
            w = np.ascontiguousarray(walls, np.float64).reshape(-1, 4)
            g = np.ascontiguousarray(gates, np.float64).reshape(-1, 4)
            check(lib.pc_track_from_arrays(w.ctypes.data, len(w), g.ctypes.data, len(g), float(start[0]), float(start[1]),
                                           float(start[2]), C.byref(h)), "pc_track_from_arrays")
        self._h = h
        self.path = path
        s, g_, st = C.c_int(), C.c_int(), (C.c_double * 3)()
        check(lib.pc_track_info(h, C.byref(s), C.byref(g_), st), "pc_track_info")
        self.n_walls, self.n_gates = s.value, g_.value
        self.start_x, self.start_y, self.start_angle = st[0], st[1], st[2]

    def geometry(self):
        walls = np.zeros((self.n_walls, 4), np.float64)
        gates = np.zeros((self.n_gates, 4), np.float64)
        check(lib.pc_track_geometry(self._h, walls.ctypes.data, gates.ctypes.data), "pc_track_geometry")
        return walls, gates

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.pc_track_destroy(h)


def ray_count(num_rays):
    """len(range(0, 360, 360 // n)) -- car_env.py:269: 12 -> 12, 16 -> 17, 32 -> 33."""
    r = lib.pc_ray_count(int(num_rays))
    check(min(r, 0), f"pc_ray_count({num_rays})")
    return r


class _Space:
    """gymnasium's two spaces as the reference declares and train.py reads them (train.py:141-142): the Box observation space
    with its bound vectors (car_env.py:513-524: low = [0, 0, -1, -1, -1, -1, 0 ...], high = 1, float32) and Discrete(9)
    (car_env.py:525).  `.shape` is the width CarEnv.step actually PRODUCES, 6 + R (R = 12 / 17 / 33 rays for num_rays 12 / 16 /
    32, car_env.py:269); the reference declares 6 + num_rays (its Box for num_rays = 16 says (22,) while _get_obs returns 23
    entries -- SURVEY quirk Q1): that declared shape is kept as `.declared_shape`."""

    def __init__(self, shape=None, n=None, dtype=np.float32, low=None, high=None, declared_shape=None):
        self.shape, self.n, self.dtype = shape, n, dtype
        self.low, self.high = low, high
        self.declared_shape = declared_shape if declared_shape is not None else shape

    @classmethod
    def car_obs(cls, obs_dim, num_rays_nominal, batch=None):
        """Box(low, high) of CarEnv.__init__ (car_env.py:514-524) for an observation of obs_dim entries; batch = n_envs gives the
        vector env's batched space (gymnasium tiles the single space's bounds)."""
        low = np.concatenate([np.array([0.0, 0.0, -1.0, -1.0, -1.0, -1.0], np.float32), np.zeros(obs_dim - 6, np.float32)])
        high = np.ones(obs_dim, np.float32)
        shape, decl = (obs_dim,), (6 + num_rays_nominal,)
        if batch is not None:
            low, high = np.broadcast_to(low, (batch, obs_dim)), np.broadcast_to(high, (batch, obs_dim))
            shape, decl = (batch, obs_dim), (batch, 6 + num_rays_nominal)
        return cls(shape=shape, low=low, high=high, declared_shape=decl)

    def contains(self, x):
        """gymnasium.spaces.Box.contains / Discrete.contains.  (The reference never clips the position to the track's frame, so a
        car that leaves the 1280 x 720 window produces an observation outside its own declared Box: car_env.py:578-581.)"""
        x = np.asarray(x)
        if self.n is not None:
            return bool(np.issubdtype(x.dtype, np.integer) and np.all((x >= 0) & (x < self.n)))
        if self.low is None:
            return tuple(x.shape) == tuple(self.shape)
        return bool(tuple(x.shape) == tuple(self.shape) and np.all(x >= self.low) and np.all(x <= self.high))

    def __repr__(self):
        if self.n is not None:
            return f"Discrete({self.n})"
        if self.low is None:
            return f"Box(-inf, inf, {self.shape}, float32)"
        return f"Box({float(np.min(self.low))}, {float(np.max(self.high))}, {self.shape}, float32)"


def _device_index(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"VecCarEnv runs on an AMD GPU only (got device {device}); there is no CPU path")
    if not torch.cuda.is_available():
        raise RuntimeError("VecCarEnv needs a GPU: torch.cuda.is_available() is False and there is no CPU fallback")
    return device.index if device.index is not None else torch.cuda.current_device()


class VecCarEnv:
    """n_envs CarEnv instances stepped by one kernel launch.

    Mirrors `gym.vector.AsyncVectorEnv([make_env(...)] * n)` as the reference uses it:
      reset(options={"track_path": p}) -> (obs[N, D] float32, infos)          train.py:159-164
      step(actions[N] int64) -> (obs, rewards, terminateds, truncateds, infos)  train.py:185
        with TransformReward's `r * reward_scaling` (train.py:65,68) and same-step auto-reset
      close()                                                                   train.py:296
    `num_rays` is Car's nominal ray count (car_env.py:227); the observation has 6 + R entries with
    R = len(range(0, 360, 360 // num_rays)) exactly as the reference produces them.
    tracks: one path / Track, or a list of them with `track_id` [N] picking each env's track.
    record_episode_statistics=True (gymnasium's RecordEpisodeStatistics, on the device): step() adds infos["episode"] = {"r" float64,
    "l", "gates", "laps" int32} [N], valid where infos["_episode"]; step() and step_many() accumulate what episode_statistics() returns.
    """

    def __init__(self, n_envs, tracks, num_rays=12, reward_scaling=1.0, device="cuda", dtype="f32", track_id=None,
                 record_episode_statistics=False, render_mode=None):
        if render_mode not in (None, "rgb_array"):
            raise ValueError(f"VecCarEnv: render_mode must be None or 'rgb_array', not {render_mode!r}")
        self.render_mode = render_mode
        self._renderers = {}
        self.device = torch.device("cuda", _device_index(device))
        self.num_envs = int(n_envs)
        self.num_rays = int(num_rays)
        self.reward_scaling = float(reward_scaling)
        self.dtype = dtype
        self._h = None
        self._tracks = None
        self._track_id = None if track_id is None else np.ascontiguousarray(track_id, np.uint8)
        self._opts = {}
        self._seq_ws = None      # the policy step's side outputs in rollout_sequences(agent=...), grown on demand
        self._build(tracks)
        self._episodes = None
        if record_episode_statistics:
            from .episodes import EpisodeStats
            self._episodes = EpisodeStats(self.num_envs, self.reward_scaling, self.device)
            self._episode_step_out = self._episodes.new_out()

    # ---- construction ---------------------------------------------------------------------
    def _build(self, tracks):
        if isinstance(tracks, (str, os.PathLike, Track)):
            tracks = [tracks]
        tr = [t if isinstance(t, Track) else Track(t) for t in tracks]
        arr = (C.c_void_p * len(tr))(*[t._h for t in tr])
        h = C.c_void_p()
        tid = self._track_id
        if tid is not None and len(tid) != self.num_envs:
            raise ValueError("track_id must have one entry per env")
        check(lib.pc_env_create(self.device.index, self.num_envs, self.num_rays, arr, len(tr),
                                tid.ctypes.data if tid is not None else None, _capi.DTYPES[self.dtype], C.byref(h)),
              "pc_env_create")
        self.close()
        self._h, self._tracks = h, tr
        self._renderers = {}             # (their backgrounds are the old handle's tracks)
        self.obs_dim = lib.pc_env_obs_dim(h)
        self.act_dim = lib.pc_env_num_actions(h)
        # dtype f32: walls that float32 cannot order (crossing / touching non-neighbours, spikes, very short walls) are resolved by a
        # float64 scan of the whole chain -- exact, and an O(n_walls) cost on every ray that selects one: say so when it is a large share
        self.track_info = []
        for k in range(len(tr)):
            w, nv, ns = C.c_int(), C.c_int(), C.c_int()
            check(lib.pc_env_track_info(h, k, C.byref(w), C.byref(nv), C.byref(ns)), "pc_env_track_info")
            self.track_info.append({"n_walls": w.value, "n_chain_vertices": nv.value, "n_scan_segments": ns.value})
            if self.dtype in ("f32", "float32") and ns.value * 4 > w.value:
                import warnings
                warnings.warn(f"track {k} ({getattr(tr[k], 'path', None)}): {ns.value} of {w.value} walls cross, touch or fold back on another wall; "
                              "dtype='f32' resolves every ray that selects one of them by a float64 scan of all walls (exact, slow) -- "
                              "consider dtype='f64' or cleaning the track (python -m ppo_car_amd.track_tool check)", RuntimeWarning, stacklevel=3)
        # what train.py:141-142 reads: envs.single_observation_space.shape, envs.single_action_space.n
        self.single_observation_space = _Space.car_obs(self.obs_dim, self.num_rays)
        self.single_action_space = _Space(n=self.act_dim, dtype=np.int64)
        self.observation_space = _Space.car_obs(self.obs_dim, self.num_rays, batch=self.num_envs)
        self.action_space = _Space(shape=(self.num_envs,), dtype=np.int64)
        self.single_observation_space_shape = (self.obs_dim,)     # (round-1 spellings, kept)
        self.single_action_space_n = self.act_dim
        for name, value in self._opts.items():       # (a rebuilt handle -- reset(options={"track_path": ...}) -- keeps its options)
            check(lib.pc_env_set_option(self._h, self.OPTIONS[name], value), f"pc_env_set_option({name})")

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _new(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    @staticmethod
    def _ptr(t, dtype, numel, what):
        if t is None:
            return None
        if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() == numel):
            raise ValueError(f"{what}: need a contiguous {dtype} CUDA tensor with {numel} elements, got "
                             f"{tuple(t.shape)} {t.dtype} {t.device}")
        return t.data_ptr()

    _ROW_DTYPES = {"track_id": torch.uint8, "active": torch.uint8, "actions": torch.int64}

    def _pose_args(self, what, px, py, vx, vy, turns, noun="states", **rows):
        """M and the pointers of a call's state rows: px, py, vx, vy float64 and turns int32, then `rows` in the order given (track_id,
        active uint8; actions int64; anything else int32), each of M entries or None."""
        if px.dim() != 1 or px.numel() < 1:
            raise ValueError(f"{what}: px must be a 1-d tensor of M >= 1 {noun}, got {tuple(px.shape)}")
        M = px.numel()
        ptrs = [self._ptr(t, torch.float64, M, name) for name, t in (("px", px), ("py", py), ("vx", vx), ("vy", vy))]
        ptrs.append(self._ptr(turns, torch.int32, M, "turns"))
        ptrs += [self._ptr(t, self._ROW_DTYPES.get(name, torch.int32), M, name) for name, t in rows.items()]
        return M, ptrs

    # ---- gymnasium-style surface ----------------------------------------------------------------
    def reset(self, seed=None, options=None, out=None):
        """seed is accepted and ignored, as in the reference (the env is deterministic, car_env.py:617)."""
        if options and "track_path" in options:
            if len(self._tracks) != 1 or self._tracks[0].path != options["track_path"]:
                self._build(options["track_path"])
        obs = out if out is not None else self._new(self.num_envs, self.obs_dim)
        check(lib.pc_env_reset(self._h, self._ptr(obs, torch.float32, self.num_envs * self.obs_dim, "obs"), self._stream()),
              "pc_env_reset")
        if self._episodes is not None:
            self._episodes.reset()
        return obs, {}

    def infos(self):
        """CarEnv._get_info() (car_env.py:599-603) of every env's current state, as device tensors."""
        gp, tp = self._new(self.num_envs, dtype=torch.int32), self._new(self.num_envs, dtype=torch.int32)
        check(lib.pc_env_info(self._h, gp.data_ptr(), tp.data_ptr(), self._stream()), "pc_env_info")
        return {"gates_passed": gp, "time_passed": tp}

    def step(self, actions, out=None, gates_passed=None, final_obs=None, info=False):
        """out = (obs, rewards, terminateds, truncateds) preallocated tensors (e.g. rows of the rollout
        buffer) or None to allocate.  Flags are float32 0/1, what train.py:191-192 builds.
        info=True fills `infos` with CarEnv._get_info()'s keys (car_env.py:599-603) as device tensors:
        "gates_passed" / "time_passed" of every env's current state (0 / 0 for an env auto-reset in this step, whose
        finished episode's count is "final_gates_passed" -- gymnasium's final_info["gates_passed"])."""
        N, D = self.num_envs, self.obs_dim
        if actions.dtype != torch.int64 or not actions.is_cuda:
            actions = actions.to(device=self.device, dtype=torch.int64)
        actions = actions.contiguous()
        if out is None:
            out = (self._new(N, D), self._new(N), self._new(N), self._new(N))
        obs, rew, term, trunc = out
        if info and gates_passed is None:
            gates_passed = self._new(N, dtype=torch.int32)
        check(lib.pc_env_step(self._h, self._ptr(actions, torch.int64, N, "actions"), self.reward_scaling,
                              self._ptr(obs, torch.float32, N * D, "obs"), self._ptr(rew, torch.float32, N, "rewards"),
                              self._ptr(term, torch.float32, N, "terminateds"), self._ptr(trunc, torch.float32, N, "truncateds"),
                              self._ptr(gates_passed, torch.int32, N, "gates_passed"),
                              self._ptr(final_obs, torch.float32, N * D, "final_obs"), self._stream()), "pc_env_step")
        infos = {}
        if info:
            gp, tp = self._new(N, dtype=torch.int32), self._new(N, dtype=torch.int32)
            check(lib.pc_env_info(self._h, gp.data_ptr(), tp.data_ptr(), self._stream()), "pc_env_info")
            infos["gates_passed"], infos["time_passed"] = gp, tp
            infos["final_gates_passed"] = gates_passed
        elif gates_passed is not None:
            infos["gates_passed"] = gates_passed
        if final_obs is not None:
            infos["final_observation"] = final_obs
        if self._episodes is not None:
            self._record_step(rew, term, trunc, infos)
        return obs, rew, term, trunc, infos

    def _record_step(self, rew, term, trunc, infos):
        """infos["episode"] / ["_episode"] of the episodes this step finished (gymnasium's vector format), and their totals into the
        running statistics."""
        ep, so = self._episodes, self._episode_step_out
        ep.clear(so)
        ep.update(rew, term, trunc, layout="steps", out=so)
        acc = ep.out
        acc[:5] += so[:5]
        torch.minimum(acc[5], so[5], out=acc[5])
        torch.maximum(acc[6], so[6], out=acc[6])
        infos["episode"] = {"r": so[1] / self.reward_scaling, "l": so[2].to(torch.int32), "gates": so[3].to(torch.int32),
                            "laps": so[4].to(torch.int32)}
        infos["_episode"] = so[0] > 0

    def episode_statistics(self):
        """The statistics of the episodes finished since the last call (record_episode_statistics=True), as 0-d device tensors
        (episodes; mean return (unscaled), return_min / _max, mean length, gates and laps per episode; NaN means when none finished),
        then clears them.  No host synchronisation; episodes.to_host() turns them into floats / None."""
        if self._episodes is None:
            raise RuntimeError("VecCarEnv(record_episode_statistics=True) keeps episode statistics; this env does not")
        s = self._episodes.summary()
        self._episodes.clear()
        return s

    def step_many(self, actions, out=None):
        """`for t in range(T): envs.step(actions[t])` as ONE call (pc_env_step_many): actions [T, N] int64 -> (obs [T, N, D], rewards,
        terminateds, truncateds [T, N]), row t = what the t-th step() returns, bit for bit; the env state afterwards is the state after
        those T steps.  Where the handle has the table-driven kernel (last_step_kernel() == "K1f" / "K1f-table") the T steps are one launch."""
        N, D = self.num_envs, self.obs_dim
        if actions.dtype != torch.int64 or not actions.is_cuda:
            actions = actions.to(device=self.device, dtype=torch.int64)
        actions = actions.contiguous()
        if actions.dim() != 2 or actions.shape[1] != N:
            raise ValueError(f"step_many: actions must be [T, {N}], got {tuple(actions.shape)}")
        T = actions.shape[0]
        if out is None:
            out = (self._new(T, N, D), self._new(T, N), self._new(T, N), self._new(T, N))
        obs, rew, term, trunc = out
        check(lib.pc_env_step_many(self._h, self._ptr(actions, torch.int64, T * N, "actions"), T, self.reward_scaling,
                                   self._ptr(obs, torch.float32, T * N * D, "obs"), self._ptr(rew, torch.float32, T * N, "rewards"),
                                   self._ptr(term, torch.float32, T * N, "terminateds"), self._ptr(trunc, torch.float32, T * N, "truncateds"),
                                   self._stream()), "pc_env_step_many")
        if self._episodes is not None:
            self._episodes.update(rew, term, trunc, layout="steps")
        return obs, rew, term, trunc

    # ---- observing without stepping (pc_env_observe, pc_env_observe_poses) ---------------------------------------------------
    def observe(self, out=None, collides=None):
        """CarEnv._get_obs() (car_env.py:569-597) of every env's CURRENT state: obs [N, D] float32, e.g. after set_state().  Right
        after step() it is that step's observation, bit for bit.  collides: an optional [N] uint8 tensor that receives
        Car.check_collision (car_env.py:376-392).  The state is not modified; one launch, no synchronisation."""
        N, D = self.num_envs, self.obs_dim
        obs = out if out is not None else self._new(N, D)
        check(lib.pc_env_observe(self._h, self._ptr(obs, torch.float32, N * D, "obs"), self._ptr(collides, torch.uint8, N, "collides"),
                                 self._stream()), "pc_env_observe")
        return obs

    def observe_poses(self, px, py, turns, vx=None, vy=None, track_id=None, out=None, collides=None):
        """What a car at each of M poses sees on this env's tracks: obs [M, D] float32.  px, py (and vx, vy, default 0) float64,
        turns int32 (heading = the track's start angle + 5 degrees * turns), track_id uint8 (default track 0): device tensors of M
        entries, M independent of num_envs.  collides: an optional [M] uint8 tensor for Car.check_collision.  A pose whose track_id
        this env does not have gets a row of zeros.  The env state is neither read nor written; one launch, no synchronisation."""
        M, rows = self._pose_args("observe_poses", px, py, vx, vy, turns, noun="poses", track_id=track_id)
        D = self.obs_dim
        obs = out if out is not None else self._new(M, D)
        check(lib.pc_env_observe_poses(self._h, *rows, M, self._ptr(obs, torch.float32, M * D, "obs"),
                                       self._ptr(collides, torch.uint8, M, "collides"), self._stream()), "pc_env_observe_poses")
        return obs

    # ---- stepping without committing (pc_env_step_poses) ----------------------------------------------------------------------
    def step_poses(self, px, py, vx, vy, turns, actions, next_gate=None, time_step=None, track_id=None, active=None, out=None):
        """One CarEnv.step of M states the caller names, IN PLACE: px, py, vx, vy float64, turns int32 (observe_poses' heading rule),
        next_gate / time_step int32 (None: a fresh zero tensor) are device tensors of M entries and hold the stepped state afterwards --
        also where the step terminated or truncated: nothing is reset.  actions int64 (anything outside 0 .. 8 acts as 8), track_id
        uint8 (default track 0), active uint8 (default every row; a row with 0 is not touched in any tensor).  out = (obs [M, D]
        float32, reward [M] float32, terminated, truncated, gate [M] uint8) or None to allocate.  Returns StepPoses(obs, reward,
        terminated, truncated, gate, next_gate, time_step).  A row whose track_id this env does not have gets zeros and keeps its
        state.  The env's own state is neither read nor written; one launch, no synchronisation."""
        if next_gate is None:
            next_gate = torch.zeros_like(px, dtype=torch.int32, device=self.device)
        if time_step is None:
            time_step = torch.zeros_like(px, dtype=torch.int32, device=self.device)
        M, rows = self._pose_args("step_poses", px, py, vx, vy, turns, next_gate=next_gate, time_step=time_step, track_id=track_id,
                                  actions=actions, active=active)
        D = self.obs_dim
        if out is None:
            out = (self._new(M, D), self._new(M), self._new(M, dtype=torch.uint8), self._new(M, dtype=torch.uint8),
                   self._new(M, dtype=torch.uint8))
        obs, rew, term, trunc, gate = out
        check(lib.pc_env_step_poses(self._h, *rows, M, self.reward_scaling, self._ptr(obs, torch.float32, M * D, "obs"),
                                    self._ptr(rew, torch.float32, M, "reward"), self._ptr(term, torch.uint8, M, "terminated"),
                                    self._ptr(trunc, torch.uint8, M, "truncated"), self._ptr(gate, torch.uint8, M, "gate"),
                                    self._stream()), "pc_env_step_poses")
        return StepPoses(obs, rew, term, trunc, gate, next_gate, time_step)

    # ---- safe-action masks (pc_env_safe_actions, pc_env_safe_actions_state) ----------------------------------------------------
    def safe_actions(self, px, py, vx, vy, turns, depth=1, time_step=None, track_id=None, active=None, out=None):
        """Which of the 9 actions can still avoid a crash within `depth` steps (1 .. 4) from each of M states: bool [M, 9].  safe[m, a] is
        true iff the step under a does not terminate and -- for depth > 1 -- it truncates or some action is safe at depth - 1 from where
        it leads (a branch that reaches the time limit alive is safe).  px, py, vx, vy float64, turns int32 (observe_poses' heading rule),
        time_step int32 (default 0), track_id uint8 (default track 0), active uint8 (default every row; a row with 0 keeps its 9 bytes):
        device tensors of M entries, all read only.  out: a [M, 9] uint8 tensor to fill (the returned bool tensor is a view of it).  A row
        whose track_id this env does not have is all false.  The env state is neither read nor written; one launch, no synchronisation."""
        M, rows = self._pose_args("safe_actions", px, py, vx, vy, turns, time_step=time_step, track_id=track_id, active=active)
        safe = out if out is not None else self._new(M, 9, dtype=torch.uint8)
        check(lib.pc_env_safe_actions(self._h, *rows, M, int(depth), self._ptr(safe, torch.uint8, M * 9, "out"), self._stream()),
              "pc_env_safe_actions")
        return safe.view(torch.bool)

    def action_masks(self, depth=1, out=None):
        """The admissible actions of every env's CURRENT state (sb3-contrib's name for it): bool [n_envs, 9], safe_actions() of the state
        as step() holds it.  out: a [n_envs, 9] uint8 tensor to fill.  The state is not modified; one launch, no synchronisation."""
        N = self.num_envs
        safe = out if out is not None else self._new(N, 9, dtype=torch.uint8)
        check(lib.pc_env_safe_actions_state(self._h, int(depth), self._ptr(safe, torch.uint8, N * 9, "out"), self._stream()),
              "pc_env_safe_actions_state")
        return safe.view(torch.bool)

    # ---- scoring action sequences (pc_env_rollout_sequences, pc_env_rollout_sequences_state) -----------------------------------------
    _SEQ_OUT = (("ret", torch.float64, True), ("steps", torch.int32, True), ("status", torch.uint8, True), ("gates", torch.int32, True),
                ("laps", torch.int32, True), ("best_k", torch.int32, False), ("best_action", torch.int64, False),
                ("best_ret", torch.float64, False))

    _SEQ_VALUE_OUT = (("end_obs", torch.float32), ("end_value", torch.float32), ("end_discount", torch.float64), ("ret_env", torch.float64))

    def _sequence_args(self, what, M, actions, reward_scale, out, value=None):
        """(the call's trailing arguments from `actions` on, the dict to return).  value: None, or (gamma, bootstrap, agent, repack) for
        the entry points that discount and bootstrap (pc_env_rollout_sequences_value[_state])."""
        if actions.dtype != torch.uint8 or actions.dim() not in (2, 3) or (actions.dim() == 3 and actions.shape[0] != M):
            raise ValueError(f"{what}: actions must be a uint8 tensor [H, K] (shared) or [{M}, H, K] (per state), got "
                             f"{tuple(actions.shape)} {actions.dtype}")
        H, K = actions.shape[-2:]
        stride = H * K if actions.dim() == 3 else 0
        res = {}
        for name, dtype, per_lane in self._SEQ_OUT:
            if out is None or (name not in out and name in ("ret", "steps", "status")):
                res[name] = self._new(M, K, dtype=dtype) if per_lane else self._new(M, dtype=dtype)
            else:
                res[name] = out.get(name)      # an `out` without an optional key: that array is not asked for
        ptrs = [self._ptr(res[name], dtype, M * K if per_lane else M, name) for name, dtype, per_lane in self._SEQ_OUT]
        scale = self.reward_scaling if reward_scale is None else float(reward_scale)
        args = [self._ptr(actions, torch.uint8, actions.numel(), "actions"), stride, K, H, scale]
        if value is not None:
            gamma, bootstrap, agent, repack = value
            gamma = 1.0 if gamma is None else float(gamma)
            mode = _capi.SEQ_BOOTSTRAP.get("none" if bootstrap is None else bootstrap, bootstrap)
            if not isinstance(mode, int):
                raise ValueError(f"{what}: bootstrap must be one of {sorted(_capi.SEQ_BOOTSTRAP)}, not {bootstrap!r}")
            handle = image = ws = None
            if agent is not None:
                handle = agent._policy_handle() if agent._std_mlp() else None
                stale = not getattr(agent, "_image_ok", False) or getattr(agent, "_image_handle", None) is not handle
                if handle is None or ((repack or stale) and not agent.pack_policy()):
                    raise ValueError(f"{what}: the agent's shape is outside the fused policy step's menu (two 1-hidden-layer MLPs of 256 "
                                     "units, obs dim <= 40, <= 15 actions); there is no torch fallback for the critic here")
                image = agent._image.data_ptr()
                nbytes = lib.pc_env_rollout_sequences_value_workspace(M, K)
                if self._seq_ws is None or self._seq_ws.numel() < nbytes:
                    self._seq_ws = self._new(max(nbytes, 16), dtype=torch.uint8)
                ws = self._seq_ws.data_ptr()
            D = self.obs_dim
            for name, dtype in self._SEQ_VALUE_OUT:
                need = agent is not None and name in ("end_obs", "end_value")
                if name == "end_value" and agent is None:
                    res[name] = None      # (no policy: nothing would be written)
                elif (out is None) or (need and name not in out):
                    res[name] = self._new(M, K, D, dtype=dtype) if name == "end_obs" else self._new(M, K, dtype=dtype)
                else:
                    res[name] = out.get(name)
            args += [gamma, mode, handle, image, ws] + ptrs
            args += [self._ptr(res[name], dtype, M * K * (D if name == "end_obs" else 1), name) for name, dtype in self._SEQ_VALUE_OUT]
        else:
            args += ptrs
        args.append(self._stream())
        return args, {k: v for k, v in res.items() if v is not None}

    def rollout_sequences(self, px, py, vx, vy, turns, actions, next_gate=None, time_step=None, track_id=None, active=None,
                          reward_scale=None, out=None, gamma=None, bootstrap=None, agent=None, repack=True):
        """What each of K action sequences of H steps earns from each of M states (step = step_poses' step; a sequence that terminated
        or truncated takes no further step).  px, py, vx, vy float64, turns int32 (observe_poses' heading rule), next_gate / time_step
        int32 (default 0), track_id uint8 (default track 0), active uint8 (default every row; a row with 0 is not written in any
        output): device tensors of M entries, all read only.  actions: uint8, time-major [H, K] shared by all states or [M, H, K], one
        table per state; anything outside 0 .. 8 acts as 8.  reward_scale: default the env's reward_scaling.  Returns a dict of device
        tensors: ret float64, steps int32, status uint8 (_capi.PC_FIRST_*), gates, laps int32, each [M, K]; best_k int32 (the lowest k
        of the row's maximum), best_action int64 (its first action), best_ret float64, each [M].  out: a dict of tensors to fill; with
        `out` given, an optional key it lacks (gates, laps, best_*) is not computed.  A row whose track_id this env does not have gets
        zeros (best_action 8).  The env state is neither read nor written; no synchronisation.
        gamma, bootstrap, agent: all None (the default) is the call above.  Otherwise pc_env_rollout_sequences_value: ret is the
        discounted sum (gamma, default 1.0) plus, where `bootstrap` ("none", "running" or "running_truncated") covers the lane's status,
        end_discount * the value `agent`'s critic gives the observation the lane ends at -- one fused policy step over all M * K end
        observations.  agent: a ppo_car_amd.Agent on the fused menu (a ValueError otherwise: there is no torch fallback); its weights
        are packed once per call unless repack=False.  The dict gains end_obs float32 [M, K, D], end_value float32 (with an agent),
        end_discount and ret_env float64 [M, K]; with `out` given, end_discount / ret_env (and, without an agent, end_obs) are computed
        only where `out` has the key."""
        M, rows = self._pose_args("rollout_sequences", px, py, vx, vy, turns, next_gate=next_gate, time_step=time_step, track_id=track_id,
                                  active=active)
        if gamma is None and bootstrap is None and agent is None:
            args, res = self._sequence_args("rollout_sequences", M, actions, reward_scale, out)
            check(lib.pc_env_rollout_sequences(self._h, *rows, M, *args), "pc_env_rollout_sequences")
            return res
        args, res = self._sequence_args("rollout_sequences", M, actions, reward_scale, out, (gamma, bootstrap, agent, repack))
        check(lib.pc_env_rollout_sequences_value(self._h, *rows, M, *args), "pc_env_rollout_sequences_value")
        return res

    def score_sequences(self, actions, reward_scale=None, out=None, gamma=None, bootstrap=None, agent=None, repack=True):
        """rollout_sequences() of every env's CURRENT state, as step() holds it (M = n_envs).  The state is not modified."""
        if gamma is None and bootstrap is None and agent is None:
            args, res = self._sequence_args("score_sequences", self.num_envs, actions, reward_scale, out)
            check(lib.pc_env_rollout_sequences_state(self._h, *args), "pc_env_rollout_sequences_state")
            return res
        args, res = self._sequence_args("score_sequences", self.num_envs, actions, reward_scale, out, (gamma, bootstrap, agent, repack))
        check(lib.pc_env_rollout_sequences_value_state(self._h, *args), "pc_env_rollout_sequences_value_state")
        return res

    def render(self, envs=None, scale=2):
        """gymnasium's rgb_array: frames of the CURRENT state of all envs, or of the listed ones in the listed order, uint8
        [K, 720 / scale, 1280 / scale, 3] on the device (renderer.Renderer; one frame is frames[k]).  observe() into a scratch tensor, then
        the rasteriser; the next gate of every env comes from the handle's own state.  The state is not modified."""
        from .renderer import Renderer
        r = self._renderers.get(scale)
        if r is None:
            r = self._renderers[scale] = Renderer(self, scale)
        obs = self.observe()
        ng = np.zeros(self.num_envs, np.int64)
        check(lib.pc_env_get_state(self._h, None, None, None, None, None, None, ng.ctypes.data, None), "pc_env_get_state")
        ng = torch.from_numpy(ng.astype(np.int32)).to(self.device)
        tid = None if self._track_id is None else torch.from_numpy(self._track_id).to(self.device)
        if envs is not None:
            idx = torch.as_tensor(np.asarray(envs, np.int64).reshape(-1), device=self.device)
            obs, ng = obs[idx].contiguous(), ng[idx].contiguous()
            tid = None if tid is None else tid[idx].contiguous()
        return r.frames(obs, next_gate=ng, track_id=tid)

    def last_step_kernel(self):
        """which kernel the last step() / step_many() launched: "K1" (generic per-step kernel), "K1f" (table-driven), "K1f-table" or "none"."""
        code = lib.pc_env_last_step_kernel(self._h)
        if code < 0:
            check(code, "pc_env_last_step_kernel")
        return _capi.PC_STEP_NAMES[code]

    def close(self):
        h, self._h = self._h, None
        if h:
            lib.pc_env_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- teacher forcing / introspection (parity tests, bench) -----------------------------------
    _FIELDS = (("px", np.float64), ("py", np.float64), ("vx", np.float64), ("vy", np.float64), ("rot", np.float64),
               ("time_step", np.int64), ("next_gate", np.int64), ("passed", np.int64))

    def get_state(self):
        out = {k: np.zeros(self.num_envs, dt) for k, dt in self._FIELDS}
        check(lib.pc_env_get_state(self._h, *[out[k].ctypes.data for k, _ in self._FIELDS]), "pc_env_get_state")
        return out

    def set_state(self, **kw):
        args = []
        for k, dt in self._FIELDS:
            v = kw.pop(k, None)
            if v is None:
                args.append(None)
            else:
                a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (self.num_envs,)))
                args.append(a)
        if kw:
            raise TypeError(f"unknown state fields {sorted(kw)}")
        check(lib.pc_env_set_state(self._h, *[a.ctypes.data if a is not None else None for a in args]), "pc_env_set_state")
        if self._episodes is not None:
            self._episodes.forget()      # the injected episodes' history is unknown

    def launch_info(self):
        v = [C.c_int() for _ in range(4)]
        check(lib.pc_env_launch_info(self._h, *[C.byref(x) for x in v]), "pc_env_launch_info")
        return dict(lanes_per_env=v[0].value, rays_per_lane=v[1].value, blocks=v[2].value, threads=v[3].value)

    def last_rollout_kernel(self):
        """which persistent kernel the last pc_rollout on this handle launched: "K9", "K9s", "K9-literal", "K9d-filter" or "none" (every one fills the same buffers bit for bit)"""
        from ._capi import PC_KERNEL_NAMES
        code = lib.pc_env_last_rollout_kernel(self._h)
        if code < 0:
            check(code, "pc_env_last_rollout_kernel")
        return PC_KERNEL_NAMES[code]

    def set_lanes_per_env(self, lanes):
        check(lib.pc_env_set_lanes_per_env(self._h, int(lanes)), "pc_env_set_lanes_per_env")

    OPTIONS = {"rollout_form": 1, "rollout_epw": 2, "rollout_fast": 3, "step_form": 4}     # PC_OPT_* (include/ppocar.h)

    def set_option(self, name, value):
        """Per-handle launch option of pc_rollout / pc_env_step on THIS vector env (other handles keep theirs).  step_form: 0 automatic,
        1 always the generic per-step kernel K1, 2 the table-driven K1f wherever the handle has it."""
        check(lib.pc_env_set_option(self._h, self.OPTIONS[name], int(value)), f"pc_env_set_option({name})")
        self._opts[name] = int(value)

    def get_option(self, name):
        v = C.c_int()
        check(lib.pc_env_get_option(self._h, self.OPTIONS[name], C.byref(v)), f"pc_env_get_option({name})")
        return v.value
