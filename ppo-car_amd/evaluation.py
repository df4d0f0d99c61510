"""Batched evaluation: the FIRST episode of N fresh envs, one per env, with lap times -- the batched form of the reference's log_video
episode (train.py:23-50) and of the PPO libraries' evaluate_policy / EvalCallback.

An Evaluator owns everything it runs on: its own VecCarEnv handle, its own row buffers of `chunk` steps, its own [8, N] float64 state
(include/ppocar.h pc_first_episodes) and its own weight image, packed through the agent's current policy handle into its own buffer
with its own range-status word.  It reads the agent's parameters and nothing else of it: not Agent.act / pack_policy, not the agent's
call counter, image or range-check event, not torch's global RNG, nothing of a Trainer.  A training run with an evaluator computes,
bit for bit, what it computes without one.

run(index) resets the envs and steps exactly PC_TIME_LIMIT = 1000 steps in ceil(1000 / chunk) windows, each followed by
pc_first_episodes.  CarEnv truncates at time >= 1000 (car_env.py:745-750), so after 1000 steps from reset EVERY env has closed its
first episode: no early stop, no host synchronisation.  The draw of step t comes from the stream (seed, offset = index * 1000 + t,
idx = env), so run(index) is reproducible and two indices never share a draw.
  sampled, a shape pc_rollout takes : one pc_rollout per window (Buffer layout)                             last_path == "mega"
  greedy=True, rollout_kernel="mega", a shape pc_rollout_greedy takes: one pc_rollout_greedy per window     last_path == "mega"
  rollout_kernel="steps", greedy=True with "auto", or a shape the persistent kernel refuses: per step pc_policy_act (greedy:
                                      pc_policy_act_greedy), then pc_env_step into step-layout rows         last_path == "steps"
  an agent outside the fused kernel's menu: agent.actor(obs) + pc_sample / pc_greedy                        last_path == "steps"
pc_rollout == T x (pc_policy_act; pc_env_step) and pc_rollout_greedy == T x (pc_policy_act_greedy; pc_env_step) bit for bit, so the two
paths of either kind leave the same state bits.  (Making "mega" what "auto" means for greedy evaluations too is a one-line change in
__init__ below, once pc_rollout_greedy has run in anger.)

track_maps=True: the evaluator owns a TrackMaps (track_maps.py), one plane set per track of its handle, cleared by run() and updated
in front of every window's pc_first_episodes with the state as it stands there -- the maps cover exactly the first episodes.  The
persistent path has the observation rows already; the per-step path then keeps the window's rows (step t reads row t and writes row
t + 1, the window's last step writes _next_obs) instead of stepping one row in place: the same launches on other addresses, the same
state bits.  Off: not one launch or buffer is added.

video_envs=K > 0: the evaluator keeps the observation rows, rewards and flags of envs 0 .. K - 1 for all 1000 steps ([1000, K, D]: a few
hundred KB), copied out of each window's rows on both paths (the per-step path: one K x D copy in front of every step).  After run(),
video_frames() renders every video_every_step-th step of each of those envs' FIRST episodes on the device (renderer.Renderer: a frame is
a pure function of the observation row, the track and the next-gate index, which is the running count of the episode's gate steps --
decoded from the rewards as pc_first_episodes decodes them -- modulo the track's gate count) and returns one contact sheet per frame
time.  The copies read rows the windows have written and write the evaluator's own buffers: self.state holds the same bits with video
on or off.  Off: not one launch or buffer is added.

shield_depth=d > 0 (per-step path only; with rollout_kernel="mega" a ValueError): a shielded evaluation.  Every step takes the policy's
own action as without a shield (the draw or the argmax: the random stream is the same), asks pc_env_safe_actions_state which actions
can still avoid a crash within d steps, and where the chosen action cannot while another can, replaces it by the safe action with the
highest logit (pc_greedy of the logits with the unsafe entries at -FLT_MAX: the lowest index on ties).  A row with no safe action keeps
its action.  Over the steps of the first episodes (an env counts until the step that closes its first episode, that step included:
pc_first_episodes' rule) it counts the steps, the replaced steps and the steps with no safe action: shield_totals(), and
eval/shield_interventions and eval/shield_doomed in evaluate()'s dict.  A crash of an unshielded policy that the shield prevents was
tactical; what is left with the shield on was decided more than d steps ahead.  Off (0, the default): not one launch, tensor or key
is added."""
import math
import sys

import numpy as np
import torch

from . import _capi
from ._capi import PC_EPISODE_BUFFER, PC_EPISODE_STEPS, PC_FIRST_ROWS, PC_TIME_LIMIT, check, lib
from .env import VecCarEnv
from .model import PolicyRangeError
from .renderer import Renderer, frame_size
from .track_maps import TrackMaps

EVAL_MEAN_KEYS = ("eval/episodic_return", "eval/episodic_return_min", "eval/episodic_return_max", "eval/episodic_length",
                  "eval/gates_per_episode", "eval/laps_per_episode", "eval/crash_rate", "eval/best_lap_steps", "eval/mean_lap_steps",
                  "eval/first_lap_steps")
EVAL_KEYS = ("eval/episodes",) + EVAL_MEAN_KEYS
# Evaluator.totals(): float64 [EVAL_TOTALS]
#   0 envs   1 sum of scaled returns   2 min   3 max   4 sum of lengths   5 of gates   6 of laps   7 envs that terminated
#   8 sum of row 5 (the lap times' sum)   9 min of row 6 (best lap)   10 envs that lapped   11 sum of their first laps
#   12 the range status of the evaluator's weight image (include/ppocar.h PC_POLICY_RANGE_*; 0 = inside the arithmetic's domain)
EVAL_TOTALS = 13
SHIELD_KEYS = ("eval/shield_interventions", "eval/shield_doomed")
# Evaluator.shield_totals(): float64 [3] = steps of the first episodes, those whose action the shield replaced, those with no safe action
_warned_range = False


def new_state(n_envs, device):
    """The state pc_first_episodes starts from: rows 0-5 zero, rows 6-7 +inf."""
    s = torch.zeros(PC_FIRST_ROWS, n_envs, dtype=torch.float64, device=device)
    s[6:].fill_(math.inf)
    return s


def state_totals(s, range_status):
    """A pc_first_episodes state [8, N] reduced over envs in a fixed order, with the range-status word (int32 [1]) as entry 12: float64
    [EVAL_TOTALS] on the state's device, no host synchronisation."""
    lapped = torch.isfinite(s[7])
    one = lambda x: x.reshape(1).to(torch.float64)
    return torch.cat([torch.full((1,), float(s.shape[1]), dtype=torch.float64, device=s.device), one(s[0].sum()),
                      one(s[0].min()), one(s[0].max()), one(s[1].sum()), one(s[2].sum()), one(s[3].sum()),
                      one((s[4] == float(_capi.PC_FIRST_TERMINATED)).sum()), one(s[5].sum()), one(s[6].min()), one(lapped.sum()),
                      one(torch.where(lapped, s[7], torch.zeros_like(s[7])).sum()), one(range_status)])


def evaluation_scalars(tot, reward_scaling, policy_range="fallback"):
    """Host totals (Evaluator.totals(), tolist()) -> the eval/* keys.  Returns are unscaled.  The lap keys are None where no env lapped.
    A non-zero range status (the weights left the fp16 x 2 policy arithmetic's domain: the episodes were not this policy's) makes every
    mean None, with one warning on stderr -- or PolicyRangeError with policy_range = "raise", as Agent.policy_range decides elsewhere."""
    global _warned_range
    n, s = tot[0], float(reward_scaling)
    if tot[12] != 0:
        if policy_range == "raise":
            raise PolicyRangeError("the policy weights left the fp16x2 form's numeric domain during an evaluation "
                                   f"(range status {int(tot[12])}): use policy_precision = 0")
        if not _warned_range:
            _warned_range = True
            print(f"[ppo_car_amd] evaluation: the policy weights left the fp16x2 form's numeric domain (range status {int(tot[12])}); "
                  "its episodes are not the policy's and are not reported", file=sys.stderr, flush=True)
        return {"eval/episodes": int(n), **{k: None for k in EVAL_MEAN_KEYS}}
    lapped = tot[10] > 0
    return {"eval/episodes": int(n), "eval/episodic_return": tot[1] / n / s, "eval/episodic_return_min": tot[2] / s,
            "eval/episodic_return_max": tot[3] / s, "eval/episodic_length": tot[4] / n, "eval/gates_per_episode": tot[5] / n,
            "eval/laps_per_episode": tot[6] / n, "eval/crash_rate": tot[7] / n,
            "eval/best_lap_steps": tot[9] if lapped else None,
            "eval/mean_lap_steps": tot[8] / tot[6] if tot[6] > 0 else None,
            "eval/first_lap_steps": tot[11] / tot[10] if lapped else None}


class Evaluator:
    def __init__(self, agent, tracks, n_envs=1024, num_rays=12, reward_scaling=0.1, device="cuda", dtype="f32", track_id=None,
                 greedy=False, seed=0, chunk=250, rollout_kernel="auto", track_maps=False, track_maps_cell=8, video_envs=0, video_scale=4,
                 video_every_step=2, shield_depth=0):
        if not 0 <= int(shield_depth) <= _capi.PC_SAFE_MAX_DEPTH:
            raise ValueError(f"Evaluator: shield_depth must be 0 (off) .. {_capi.PC_SAFE_MAX_DEPTH}, not {shield_depth!r}")
        if int(shield_depth) > 0 and rollout_kernel == "mega":
            raise ValueError("Evaluator: shield_depth > 0 masks the action between the policy step and the env step, which only the "
                             "per-step path has: rollout_kernel must be 'auto' or 'steps', not 'mega'")
        if int(n_envs) < 1:
            raise ValueError(f"Evaluator: n_envs must be >= 1, not {n_envs!r}")
        if int(chunk) < 1:
            raise ValueError(f"Evaluator: chunk must be >= 1, not {chunk!r}")
        if rollout_kernel not in ("auto", "mega", "steps"):
            raise ValueError(f"Evaluator: rollout_kernel must be 'auto', 'mega' or 'steps', not {rollout_kernel!r}")
        if not 0 <= int(video_envs) <= int(n_envs):
            raise ValueError(f"Evaluator: video_envs must be 0 .. n_envs = {int(n_envs)}, not {video_envs!r}")
        if int(video_every_step) < 1:
            raise ValueError(f"Evaluator: video_every_step must be >= 1, not {video_every_step!r}")
        if int(video_envs) > 0:
            frame_size(video_scale)         # (ValueError for a scale off the list, before anything is created)
        self.agent = agent
        self.envs = VecCarEnv(int(n_envs), tracks, num_rays=num_rays, reward_scaling=reward_scaling, device=device, dtype=dtype,
                              track_id=track_id)
        self.device = self.envs.device
        self.num_envs, self.reward_scaling = self.envs.num_envs, float(reward_scaling)
        self.greedy, self.seed = bool(greedy), int(seed)
        self.chunk = min(int(chunk), PC_TIME_LIMIT)
        self.last_path = None
        N, D, A, C = self.num_envs, self.envs.obs_dim, self.envs.act_dim, self.chunk
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=self.device)
        self.state = new_state(N, self.device)
        self._state0 = self.state.clone()
        self._fused = bool(agent._std_mlp()) and agent.policy_form() is not None
        self._mega = self._fused and (rollout_kernel == "mega" if self.greedy else rollout_kernel != "steps")
        self.shield_depth = int(shield_depth)
        self._shield = None
        if self.shield_depth > 0:       # the per-step path, whatever "auto" would take
            self._mega = False
            self._shield = dict(logits=new(N, A), masked=new(N, A), mask=new(N, 9, dtype=torch.uint8), act=new(N, dtype=torch.int64),
                                running=torch.ones(N, dtype=torch.bool, device=self.device),
                                counts=torch.zeros(3, dtype=torch.float64, device=self.device))
        self._image = self._image_handle = None
        self._range = torch.zeros(1, dtype=torch.int32, device=self.device)
        # rows of one window (both layouts), the observation / flags the next step starts from, and the per-step outputs
        self._rew, self._term, self._trunc = new(C, N), new(C, N), new(C, N)
        self._next_obs, self._next_term, self._next_trunc = new(N, D), new(N), new(N)
        self._act, self._logprob, self._val = new(N, dtype=torch.int64), new(N), new(N)
        self._mega_rows = None
        if self._mega:
            self._alloc_mega()
        self.maps = self._map_track_id = self._obs_rows = None
        if track_maps:
            self.maps = TrackMaps(len(self.envs._tracks), track_maps_cell, self.device)
            if self.envs._track_id is not None:
                self._map_track_id = torch.from_numpy(self.envs._track_id).to(self.device)
        self.video_envs, self.video_scale, self.video_every_step = int(video_envs), video_scale, int(video_every_step)
        self._vid = self._renderer = None
        self._t0 = 0                    # the running window's first step (run() sets it)
        if self.video_envs > 0:         # rows of envs 0 .. K - 1 in the step layout: row t = what the policy saw at step t, and step t's reward / flags
            K = self.video_envs
            self._vid = dict(obs=new(PC_TIME_LIMIT, K, D), rew=new(PC_TIME_LIMIT, K), term=new(PC_TIME_LIMIT, K), trunc=new(PC_TIME_LIMIT, K))
            self._renderer = Renderer(self.envs, video_scale)

    def _alloc_mega(self):
        N, D, C = self.num_envs, self.envs.obs_dim, self.chunk
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        self._mega_rows = dict(obs=new(C, N, D), act=new(C, N), val=new(C, N), logprob=new(C, N))

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- the weight image: this evaluator's own, packed through the agent's current handle ------------------------------------
    def _pack(self):
        agent = self.agent
        h = agent._policy_handle()
        n = agent.policy_form()[2]
        if self._image is None or self._image.numel() != n:
            self._image = torch.empty(n, dtype=torch.float32, device=self.device)
        a1, a2, c1, c2 = agent.actor[0], agent.actor[2], agent.critic[0], agent.critic[2]
        check(lib.pc_policy_pack_checked(h, a1.weight.data_ptr(), a1.bias.data_ptr(), a2.weight.data_ptr(), a2.bias.data_ptr(),
                                         c1.weight.data_ptr(), c1.bias.data_ptr(), c2.weight.data_ptr(), c2.bias.data_ptr(),
                                         self._image.data_ptr(), self._range.data_ptr(), self._stream()), "pc_policy_pack_checked")
        self._image_handle = h          # the image belongs to the handle that packed it
        return h

    # ---- one window ----------------------------------------------------------------------------------------------------------
    def _scan(self, T, layout):
        buffer = layout == PC_EPISODE_BUFFER
        check(lib.pc_first_episodes(self.device.index, self._rew.data_ptr(), self._term.data_ptr(), self._trunc.data_ptr(),
                                    self._next_term.data_ptr() if buffer else None, self._next_trunc.data_ptr() if buffer else None,
                                    T, self.num_envs, layout, self.reward_scaling, self.state.data_ptr(), self._stream()),
              "pc_first_episodes")

    def _map(self, obs, T, layout):
        """This window's rows into the maps, BEFORE its scan: the state says which envs are still in their first episode."""
        buffer = layout == PC_EPISODE_BUFFER
        self.maps.update(obs[:T], self._term[:T], self._trunc[:T], self._next_term if buffer else None,
                         self._next_trunc if buffer else None, layout, self._map_track_id, first_state=self.state)

    def _window_mega(self, h, T, offset):
        """pc_rollout (greedy: pc_rollout_greedy) over T steps: rows in the Buffer layout.  False = the shape is outside the persistent
        kernel's menu."""
        m = self._mega_rows
        m["obs"][0].copy_(self._next_obs)
        self._term[0].copy_(self._next_term)
        self._trunc[0].copy_(self._next_trunc)
        rows = (m["obs"].data_ptr(), m["act"].data_ptr(), self._rew.data_ptr(), m["val"].data_ptr(), self._term.data_ptr(),
                self._trunc.data_ptr(), m["logprob"].data_ptr(), self._next_obs.data_ptr(), self._next_term.data_ptr(),
                self._next_trunc.data_ptr(), None, None)
        if self.greedy:
            rc = lib.pc_rollout_greedy(self.envs._h, h, self._image.data_ptr(), T, self.reward_scaling, *rows, None, 0, self._stream())
        else:
            rc = lib.pc_rollout(self.envs._h, h, self._image.data_ptr(), T, self.reward_scaling, self.seed, offset, None, *rows, self._stream())
        if rc == _capi.PC_ERR_UNSUPPORTED:
            return False
        check(rc, "pc_rollout_greedy" if self.greedy else "pc_rollout")
        if self.maps is not None:
            self._map(m["obs"], T, PC_EPISODE_BUFFER)
        if self._vid is not None:       # Buffer layout -> step layout: step t's flags sit in row t + 1, the last step's in _next_*
            v, K, t0 = self._vid, self.video_envs, self._t0
            v["obs"][t0:t0 + T].copy_(m["obs"][:T, :K])
            v["rew"][t0:t0 + T].copy_(self._rew[:T, :K])
            for name, rows, last in (("term", self._term, self._next_term), ("trunc", self._trunc, self._next_trunc)):
                v[name][t0:t0 + T - 1].copy_(rows[1:T, :K])
                v[name][t0 + T - 1].copy_(last[:K])
        self._scan(T, PC_EPISODE_BUFFER)
        return True

    def _window_steps(self, h, T, offset):
        """T x (policy step; env step): rows in the step layout, the observation stepped in place (with maps: through the window's rows)."""
        N, di, st = self.num_envs, self.device.index, self._stream()
        obs, act = self._next_obs, self._act
        rows = None
        if self.maps is not None:
            if self._obs_rows is None:
                self._obs_rows = torch.empty(self.chunk, N, self.envs.obs_dim, dtype=torch.float32, device=self.device)
            rows = self._obs_rows
            rows[0].copy_(self._next_obs)
        for t in range(T):
            if rows is not None:
                obs = rows[t]
            if self._vid is not None:
                self._vid["obs"][self._t0 + t].copy_(obs[:self.video_envs])
            lg_out = self._shield["logits"].data_ptr() if self._shield is not None else None
            if h is not None and self.greedy:       # the argmax inside the policy step: two launches per step, no logits buffer
                check(lib.pc_policy_act_greedy(h, obs.data_ptr(), N, self._image.data_ptr(), act.data_ptr(), None, self._logprob.data_ptr(),
                                               self._val.data_ptr(), lg_out, st), "pc_policy_act_greedy")
            elif h is not None:
                check(lib.pc_policy_act(h, obs.data_ptr(), N, self._image.data_ptr(), self.seed, offset + t, None, act.data_ptr(), None,
                                        self._logprob.data_ptr(), self._val.data_ptr(), lg_out, st), "pc_policy_act")
            else:           # outside the fused kernel's menu: torch's GEMMs in front of the draw
                lg = self.agent.actor(obs).contiguous()
                if self._shield is not None:
                    self._shield["logits"].copy_(lg)
                if self.greedy:
                    check(lib.pc_greedy(di, lg.data_ptr(), N, self.envs.act_dim, act.data_ptr(), None, None, st), "pc_greedy")
                else:
                    check(lib.pc_sample(di, lg.data_ptr(), N, lg.shape[1], self.seed, offset + t, act.data_ptr(), self._logprob.data_ptr(),
                                        None, st), "pc_sample")
            if self._shield is not None:
                self._shield_step(act)
            nxt = obs if rows is None else (rows[t + 1] if t + 1 < T else self._next_obs)
            self.envs.step(act, out=(nxt, self._rew[t], self._term[t], self._trunc[t]))
            if self._shield is not None:    # an env counts up to and including the step that closes its first episode
                self._shield["running"] &= (self._term[t] == 0) & (self._trunc[t] == 0)
        if rows is not None:
            self._map(rows, T, PC_EPISODE_STEPS)
        if self._vid is not None:
            v, K, t0 = self._vid, self.video_envs, self._t0
            for name, src in (("rew", self._rew), ("term", self._term), ("trunc", self._trunc)):
                v[name][t0:t0 + T].copy_(src[:T, :K])
        self._scan(T, PC_EPISODE_STEPS)

    def _shield_step(self, act):
        """The shield between the policy step and the env step: `act` (the policy's own choice) is replaced, in place, where its byte of
        the state's safe-action mask is 0 and the row has a safe action, by the first maximum of the logits over the safe actions."""
        sh, N, A = self._shield, self.num_envs, self.envs.act_dim
        mask = self.envs.action_masks(self.shield_depth, out=sh["mask"])              # bool [N, 9]
        torch.where(mask[:, :A], sh["logits"], torch.full_like(sh["logits"], torch.finfo(torch.float32).min), out=sh["masked"])
        check(lib.pc_greedy(self.device.index, sh["masked"].data_ptr(), N, A, sh["act"].data_ptr(), None, None, self._stream()), "pc_greedy")
        doomed = ~mask.any(1)
        replace = ~mask.gather(1, act.unsqueeze(1)).squeeze(1) & ~doomed
        torch.where(replace, sh["act"], act, out=act)
        run = sh["running"]
        sh["counts"] += torch.stack([run.sum(), (run & replace).sum(), (run & doomed).sum()]).to(torch.float64)

    @torch.no_grad()
    def run(self, index=0):
        """The first episodes of all envs under the agent's current weights -> self.state ([8, N] float64, device).  Enqueues only."""
        h = self._pack() if self._fused else None
        self.envs.reset(out=self._next_obs)
        self._next_term.zero_()
        self._next_trunc.zero_()
        self.state.copy_(self._state0)
        if self._shield is not None:
            self._shield["running"].fill_(True)
            self._shield["counts"].zero_()
        if self.maps is not None:
            self.maps.clear()
        base = int(index) * PC_TIME_LIMIT
        mega = self._mega
        for t0 in range(0, PC_TIME_LIMIT, self.chunk):
            T = min(self.chunk, PC_TIME_LIMIT - t0)
            self._t0 = t0
            if mega and not self._window_mega(h, T, base + t0):
                if t0 != 0:
                    raise RuntimeError("Evaluator: pc_rollout refused a window after it took the first one")
                mega = self._mega = False       # nothing was launched: the per-step kernels run the whole evaluation
            if not mega:
                self._window_steps(h, T, base + t0)
        self.last_path = "mega" if mega else "steps"
        return self.state

    # ---- results -----------------------------------------------------------------------------------------------------------------
    def totals(self):
        """The state reduced over envs in a fixed order, and the weight image's range status: float64 [EVAL_TOTALS] on the device, no
        host synchronisation."""
        return state_totals(self.state, self._range)

    def shield_totals(self):
        """Evaluator(shield_depth=d): float64 [3] on the device, no host synchronisation -- the steps of the first episodes of the last
        run(), those whose action the shield replaced, those with no safe action."""
        if self._shield is None:
            raise RuntimeError("Evaluator(shield_depth=d) counts the shield's interventions; this evaluator has no shield")
        return self._shield["counts"]

    def scalars(self, host_totals, reward_scaling=None, host_shield_totals=None):
        """Host totals (totals() fetched: tolist()) -> the eval/* dict; see evaluation_scalars.  host_shield_totals (shield_totals()
        fetched) adds eval/shield_interventions and eval/shield_doomed: the shares of the first episodes' steps."""
        out = evaluation_scalars(host_totals, self.reward_scaling if reward_scaling is None else reward_scaling,
                                 getattr(self.agent, "policy_range", "fallback"))
        if host_shield_totals is not None:
            steps, replaced, doomed = host_shield_totals
            out["eval/shield_interventions"], out["eval/shield_doomed"] = replaced / steps, doomed / steps
        return out

    def evaluate(self, index=0):
        """run + fetch: the eval/* dict of one evaluation (synchronises)."""
        self.run(index)
        if self._shield is None:
            return self.scalars(self.totals().tolist())
        return self.scalars(self.totals().tolist(), host_shield_totals=self.shield_totals().tolist())

    # ---- the video ---------------------------------------------------------------------------------------------------------------
    def video_plan(self):
        """What video_frames() renders, from the kept rewards and flags (synchronises): (steps [F, K] int64, next_gate [F, K] int32,
        lengths [K]).  lengths[k] = the steps of env k's first episode; frame f shows env k at step min(f * video_every_step, the last
        multiple of video_every_step below lengths[k]) -- a finished env holds its last frame -- and F covers the longest of the K
        episodes.  next_gate of a step = the gate steps BEFORE it (k = rint(r / reward_scaling) in {1, 11, -2, 8}, pc_first_episodes'
        decoding) modulo the gate count of the env's track."""
        if self._vid is None:
            raise RuntimeError("Evaluator(video_envs=K) keeps the rows of a video; this evaluator does not")
        v, K, every = self._vid, self.video_envs, self.video_every_step
        rew = v["rew"].cpu().numpy().astype(np.float64)
        done = (v["term"].cpu().numpy() != 0) | (v["trunc"].cpu().numpy() != 0)
        lengths = np.where(done.any(0), done.argmax(0) + 1, PC_TIME_LIMIT).astype(np.int64)
        k = np.rint(rew / self.reward_scaling)
        gate = np.isin(k, (1.0, 11.0, -2.0, 8.0))
        before = np.cumsum(gate, axis=0) - gate                     # exclusive
        tid = self.envs._track_id[:K].astype(np.int64) if self.envs._track_id is not None else np.zeros(K, np.int64)
        n_gates = np.array([t.n_gates for t in self.envs._tracks], np.int64)[tid]
        F = int((lengths.max() + every - 1) // every)
        last = (lengths - 1) // every * every
        steps = np.minimum(np.arange(F, dtype=np.int64)[:, None] * every, last[None, :])
        ng = (before[steps, np.arange(K)[None, :]] % n_gates[None, :]).astype(np.int32)
        return steps, ng, lengths

    def video_frames(self, cols=None):
        """The contact sheets of the last run(): host uint8 [F, rows * H, cols * W, 3], env k of frame f at row k // cols, column
        k % cols (cols: default ceil(sqrt(K))).  Rendered in chunks of at most 256 frames."""
        from .render import contact_sheet
        steps, ng, _ = self.video_plan()
        F, K = steps.shape
        cols = int(cols) if cols is not None else int(math.ceil(math.sqrt(K)))
        r = self._renderer
        t_idx = torch.from_numpy(steps.reshape(-1)).to(self.device)
        k_idx = torch.arange(K, device=self.device).repeat(F)
        rows = self._vid["obs"][t_idx, k_idx]                      # [F * K, D]
        gates = torch.from_numpy(ng.reshape(-1)).to(self.device)
        tid = None
        if self.envs._track_id is not None:
            tid = torch.from_numpy(self.envs._track_id[:K].copy()).to(self.device).repeat(F)
        out = np.empty((F * K, r.H, r.W, 3), np.uint8)
        for a in range(0, F * K, 256):
            b = min(a + 256, F * K)
            out[a:b] = r.frames(rows[a:b], next_gate=gates[a:b], track_id=None if tid is None else tid[a:b]).cpu().numpy()
        out = out.reshape(F, K, r.H, r.W, 3)
        return np.stack([contact_sheet(out[f], cols) for f in range(F)])

    def close(self):
        self.envs.close()
