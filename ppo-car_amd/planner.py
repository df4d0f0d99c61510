"""A model-based baseline: receding-horizon random shooting on the env's own exact model (pc_env_rollout_sequences_state, K22).

Planner.act(step_index) scores `candidates` action sequences of `horizon` steps from every env's CURRENT state in one launch and
returns, per env, the first action of the best one (the lowest index on ties).  The candidate table is shared by all envs, uint8,
time-major [H, K]:
  k = 0 .. 8   "hold action k for H steps"
  k >= 9       drawn by pc_sample on all-zero logits [H * K][9] with (seed, offset = step_index): entry (t, k) is element t * K + k of
               that call -- the library's documented Philox stream (include/ppocar.h, "The stream"), so a host can regenerate the table.
Nothing is learned and nothing synchronises: a draw, the overwrite of the nine constant columns, the scoring launches.

CEMPlanner is the planner that improves on its own draws: the cross-entropy method on the same model.  Every env keeps a distribution
over the 9 actions for each of the H steps ahead -- integer weights [N, H, 9], 65536 = one -- and a planning step is `iterations` rounds
of: pc_cem_sample (K23) draws that env's K sequences from ITS weights, K22 scores them from its state (one table per state), pc_cem_refit
(K24) moves the weights towards the E best.  The nine constant sequences stay in columns 0 .. 8 of every round and the best sequence of
the round before in column 9, so an env's best return never falls from one round to the next.  With warm_start the weights are carried
from one real step to the next, shifted by one step.  All integer: a host can reproduce every table (tests/cem_reference.py).

Both planners take agent=None, gamma=1.0, bootstrap="none": with an agent and bootstrap "running" or "running_truncated" a sequence
is scored by its discounted return plus gamma^n * the agent's critic at the state it ends in (pc_env_rollout_sequences_value: K25, the
fused policy step, K26), so a short horizon sees what a long one would; CEM then refits on those returns.  The agent's weights are packed
once per act() / plan().  The defaults make the calls, and give the bits, the planners always did.

Both planners take action_values=False, temperature=0.0: when on, pc_sequences_action_values (K28) follows every scoring launch and
`out` gains q float64 [N, 9] (what the best sequence beginning with each action earned, -inf where none does), q_count int32, q_alive
uint8 (an action with a sequence that survives its first step) and soft float32 [N, 9] (the target over the alive actions: exact
ties share the mass at temperature 0, a softmax of q / temperature above it).  CEM pools its iterations' tables.  act() returns
what it returns without; off, nothing is allocated or launched.

PlannerEvaluator is the Evaluator's counterpart for the planner: the first episodes of N fresh envs, PC_TIME_LIMIT steps of act() +
pc_env_step, pc_first_episodes over windows, reported through evaluation_scalars -- the same eval/* keys a policy evaluation prints, so
a trained policy's lap and crash figures have something to stand beside."""
import torch

from ._capi import SEQ_BOOTSTRAP, PC_CEM_MAX_HORIZON, PC_CEM_W_MAX, PC_EPISODE_STEPS, PC_SEQ_MAX_CANDIDATES, PC_TIME_LIMIT, check, lib
from .env import VecCarEnv
from .evaluation import evaluation_scalars, new_state, state_totals

N_ACTIONS = 9


def _critic_args(who, envs, agent, gamma, bootstrap):
    """The scoring call's extra keywords for a planner: {} for the defaults (the call without a discount, today's bits), else gamma,
    bootstrap and agent for score_sequences / rollout_sequences -- and, for the planner's `out`, the arrays that call requires."""
    if bootstrap not in SEQ_BOOTSTRAP:
        raise ValueError(f"{who}: bootstrap must be one of {sorted(SEQ_BOOTSTRAP)}, not {bootstrap!r}")
    gamma = float(gamma)
    if not 0.0 <= gamma <= 1.0:      # (NaN fails both comparisons)
        raise ValueError(f"{who}: gamma must be in 0 .. 1, not {gamma!r}")
    if bootstrap != "none" and agent is None:
        raise ValueError(f"{who}: bootstrap={bootstrap!r} needs an agent (its critic values the end states)")
    if agent is None and gamma == 1.0:
        return {}
    return dict(gamma=gamma, bootstrap=bootstrap, agent=agent)


def _action_value_args(who, action_values, temperature):
    temperature = float(temperature)
    if not (0.0 <= temperature < float("inf")):      # (NaN fails both comparisons)
        raise ValueError(f"{who}: temperature must be finite and >= 0, not {temperature!r}")
    return bool(action_values), temperature


def _action_value_out(on, M, dev):
    """the tensors K28 fills, for a planner's `out` dict"""
    if not on:
        return {}
    return dict(q=torch.empty(M, N_ACTIONS, dtype=torch.float64, device=dev), q_count=torch.empty(M, N_ACTIONS, dtype=torch.int32, device=dev),
                q_alive=torch.empty(M, N_ACTIONS, dtype=torch.uint8, device=dev), soft=torch.empty(M, N_ACTIONS, dtype=torch.float32, device=dev))


def _action_values(dev, out, table, state_stride, M, K, active_ptr, accumulate, temperature):
    """one K28 launch on the scoring launch's outputs in `out`"""
    check(lib.pc_sequences_action_values(dev.index, out["ret"].data_ptr(), table.data_ptr(), state_stride, out["steps"].data_ptr(),
                                         out["status"].data_ptr(), active_ptr, M, K, int(accumulate), temperature, out["q"].data_ptr(),
                                         out["q_count"].data_ptr(), out["q_alive"].data_ptr(), out["soft"].data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream), "pc_sequences_action_values")


def _critic_out(kw, envs, M, K):
    """the tensors the value form fills beside K22's, for a planner's `out` dict"""
    if not kw or kw["agent"] is None:
        return {}
    dev = envs.device
    return dict(end_obs=torch.empty(M, K, envs.obs_dim, dtype=torch.float32, device=dev),
                end_value=torch.empty(M, K, dtype=torch.float32, device=dev))


class Planner:
    def __init__(self, envs, horizon=16, candidates=256, seed=0, agent=None, gamma=1.0, bootstrap="none", action_values=False,
                 temperature=0.0):
        self.action_values, self.temperature = _action_value_args("Planner", action_values, temperature)
        if not 1 <= int(horizon) <= PC_TIME_LIMIT:
            raise ValueError(f"Planner: horizon must be 1 .. {PC_TIME_LIMIT}, not {horizon!r}")
        if not N_ACTIONS <= int(candidates) <= PC_SEQ_MAX_CANDIDATES:
            raise ValueError(f"Planner: candidates must be {N_ACTIONS} (the constant sequences) .. {PC_SEQ_MAX_CANDIDATES}, not {candidates!r}")
        self._critic = _critic_args("Planner", envs, agent, gamma, bootstrap)
        self.envs, self.horizon, self.candidates, self.seed = envs, int(horizon), int(candidates), int(seed)
        dev, N, H, K = envs.device, envs.num_envs, self.horizon, self.candidates
        self.device = dev
        self._logits = torch.zeros(H * K, N_ACTIONS, dtype=torch.float32, device=dev)
        self._draw = torch.empty(H * K, dtype=torch.int64, device=dev)
        self._logprob = torch.empty(H * K, dtype=torch.float32, device=dev)
        self._const = torch.arange(N_ACTIONS, dtype=torch.uint8, device=dev).expand(H, N_ACTIONS)
        self.table = torch.empty(H, K, dtype=torch.uint8, device=dev)
        # what the scoring call fills: the per-lane totals (kept for inspection) and each env's best first action
        self.out = dict(ret=torch.empty(N, K, dtype=torch.float64, device=dev), steps=torch.empty(N, K, dtype=torch.int32, device=dev),
                        status=torch.empty(N, K, dtype=torch.uint8, device=dev), best_k=torch.empty(N, dtype=torch.int32, device=dev),
                        best_action=torch.empty(N, dtype=torch.int64, device=dev), best_ret=torch.empty(N, dtype=torch.float64, device=dev))
        self.out.update(_critic_out(self._critic, envs, N, K))
        self.out.update(_action_value_out(self.action_values, N, dev))

    def candidate_table(self, step_index):
        """The shared table of this step, uint8 [H, K] on the device (self.table, overwritten by every call)."""
        H, K = self.horizon, self.candidates
        check(lib.pc_sample(self.device.index, self._logits.data_ptr(), H * K, N_ACTIONS, self.seed, int(step_index), self._draw.data_ptr(),
                            self._logprob.data_ptr(), None, torch.cuda.current_stream(self.device).cuda_stream), "pc_sample")
        self.table.copy_(self._draw.view(H, K))
        self.table[:, :N_ACTIONS] = self._const
        return self.table

    def act(self, step_index):
        """int64 [N]: the first action of each env's best candidate from its current state (self.out["best_action"], overwritten by
        every call).  The env state is not modified; no host synchronisation."""
        self.envs.score_sequences(self.candidate_table(step_index), out=self.out, **self._critic)      # (an agent is packed here, once)
        if self.action_values:
            _action_values(self.device, self.out, self.table, 0, self.envs.num_envs, self.candidates, None, False, self.temperature)
        return self.out["best_action"]

    def drive(self, n_steps, start=0, out=None):
        """n_steps x (act(start + t); envs.step): the envs move.  Returns (rewards, terminateds, truncateds), float32 [n_steps, N] in the
        step layout (row t belongs to step t): what pc_first_episodes scans.  out: those three tensors to fill."""
        N = self.envs.num_envs
        if out is None:
            out = tuple(torch.empty(int(n_steps), N, dtype=torch.float32, device=self.device) for _ in range(3))
        rew, term, trunc = out
        obs = torch.empty(N, self.envs.obs_dim, dtype=torch.float32, device=self.device)
        for t in range(int(n_steps)):
            self.envs.step(self.act(int(start) + t), out=(obs, rew[t], term[t], trunc[t]))
        return rew, term, trunc


class CEMPlanner:
    STATE_KEYS = ("px", "py", "vx", "vy", "turns")      # of plan(states=...): required; next_gate, time_step, track_id, active optional

    def __init__(self, envs, horizon=16, candidates=64, elites=8, iterations=4, smoothing_shift=1, min_weight=64, init_weight=7281,
                 warm_start=True, seed=0, agent=None, gamma=1.0, bootstrap="none", action_values=False, temperature=0.0):
        self.action_values, self.temperature = _action_value_args("CEMPlanner", action_values, temperature)
        if not 1 <= int(horizon) <= PC_CEM_MAX_HORIZON:
            raise ValueError(f"CEMPlanner: horizon must be 1 .. {PC_CEM_MAX_HORIZON}, not {horizon!r}")
        if not N_ACTIONS + 1 <= int(candidates) <= PC_SEQ_MAX_CANDIDATES:
            raise ValueError(f"CEMPlanner: candidates must be {N_ACTIONS + 1} (the constant sequences and the kept one) .. "
                             f"{PC_SEQ_MAX_CANDIDATES}, not {candidates!r}")
        if not 1 <= int(elites) <= int(candidates):
            raise ValueError(f"CEMPlanner: elites must be 1 .. candidates = {candidates}, not {elites!r}")
        if int(iterations) < 1:
            raise ValueError(f"CEMPlanner: iterations must be >= 1, not {iterations!r}")
        if not 0 <= int(smoothing_shift) <= 16:
            raise ValueError(f"CEMPlanner: smoothing_shift must be 0 .. 16, not {smoothing_shift!r}")
        if not 0 <= int(min_weight) <= PC_CEM_W_MAX:
            raise ValueError(f"CEMPlanner: min_weight must be 0 .. {PC_CEM_W_MAX}, not {min_weight!r}")
        if not 0 <= int(init_weight) <= PC_CEM_W_MAX:
            raise ValueError(f"CEMPlanner: init_weight must be 0 .. {PC_CEM_W_MAX}, not {init_weight!r}")
        self.envs, self.horizon, self.candidates, self.elites = envs, int(horizon), int(candidates), int(elites)
        self.iterations, self.smoothing_shift, self.min_weight = int(iterations), int(smoothing_shift), int(min_weight)
        self.init_weight, self.warm_start, self.seed = int(init_weight), bool(warm_start), int(seed)
        self._critic = _critic_args("CEMPlanner", envs, agent, gamma, bootstrap)
        self.device = envs.device
        self.weights = self.table = self.best_seq = self.out = self.iter_best_ret = None
        self._rows(envs.num_envs)

    def _rows(self, M):
        """the planner's tensors for M states (plan(states=...) may bring another M than the handle's): fresh weights when M changes"""
        if self.weights is not None and self.weights.shape[0] == M:
            return
        dev, H, K = self.device, self.horizon, self.candidates
        # the weights are uint32 on the device side; int32 holds the same bits for 0 .. 65536 and torch can shift and select it
        self.weights = torch.full((M, H, N_ACTIONS), self.init_weight, dtype=torch.int32, device=dev)
        self.table = torch.empty(M, H, K, dtype=torch.uint8, device=dev)
        self.best_seq = torch.empty(M, H, dtype=torch.uint8, device=dev)
        self.iter_best_ret = torch.empty(self.iterations, M, dtype=torch.float64, device=dev)
        self.out = dict(ret=torch.empty(M, K, dtype=torch.float64, device=dev), steps=torch.empty(M, K, dtype=torch.int32, device=dev),
                        status=torch.empty(M, K, dtype=torch.uint8, device=dev), best_k=torch.empty(M, dtype=torch.int32, device=dev),
                        best_action=torch.empty(M, dtype=torch.int64, device=dev), best_ret=torch.empty(M, dtype=torch.float64, device=dev))
        self.out.update(_critic_out(self._critic, self.envs, M, K))
        self.out.update(_action_value_out(self.action_values, M, dev))

    def reset_plan(self):
        """Every state's weights back to init_weight: the plan of a planner just made."""
        self.weights.fill_(self.init_weight)

    def _carry(self, done):
        """Before planning: the weights one step on (step t + 1's become step t's, the new last step starts from init_weight), and the
        rows flagged in `done` from init_weight throughout.  Without warm_start every plan starts from init_weight.  torch ops only."""
        if not self.warm_start:
            self.weights.fill_(self.init_weight)
            return
        w = torch.roll(self.weights, -1, dims=1)
        w[:, -1] = self.init_weight
        if done is not None:
            w = torch.where((done != 0).view(-1, 1, 1), torch.full_like(w, self.init_weight), w)
        self.weights.copy_(w)

    def plan(self, step_index, states=None, done=None):
        """`iterations` x (sample at offset = step_index * iterations + i; score; refit) -> the last iteration's K22 outputs (self.out:
        ret, steps, status [M, K], best_k, best_action, best_ret [M]; overwritten by every call).  states=None: the handle's own state
        (score_sequences); else a dict of device tensors px, py, vx, vy (float64), turns (int32) and optionally next_gate, time_step,
        track_id, active as rollout_sequences takes them.  done: a device tensor [M], nonzero where the state is a fresh episode (the
        previous step's terminated | truncated): those rows' weights restart.  self.iter_best_ret [iterations, M] keeps each
        iteration's best return; self.weights ends as the last refit left it (what the warm start carries on).  Enqueues only."""
        H, K, dev = self.horizon, self.candidates, self.device
        if states is None:
            M, active = self.envs.num_envs, None
        else:
            missing = [k for k in self.STATE_KEYS if k not in states]
            if missing:
                raise ValueError(f"CEMPlanner.plan: states lacks {missing}")
            M, active = states["px"].numel(), states.get("active")
        if done is not None and done.numel() != M:
            raise ValueError(f"CEMPlanner.plan: done must have {M} entries, got {tuple(done.shape)}")
        self._rows(M)
        self._carry(done)
        stream = torch.cuda.current_stream(dev).cuda_stream
        act_ptr = None if active is None else self.envs._ptr(active, torch.uint8, M, "active")
        for i in range(self.iterations):
            check(lib.pc_cem_sample(dev.index, self.weights.data_ptr(), M, H, K, self.seed, int(step_index) * self.iterations + i, 1,
                                    self.best_seq.data_ptr() if i > 0 else None, act_ptr, self.table.data_ptr(), stream), "pc_cem_sample")
            kw = dict(self._critic, repack=i == 0) if self._critic else {}      # (the agent's image: packed once per plan, not per round)
            if states is None:
                self.envs.score_sequences(self.table, out=self.out, **kw)
            else:
                self.envs.rollout_sequences(states["px"], states["py"], states["vx"], states["vy"], states["turns"], self.table,
                                            next_gate=states.get("next_gate"), time_step=states.get("time_step"),
                                            track_id=states.get("track_id"), active=active, out=self.out, **kw)
            self.iter_best_ret[i].copy_(self.out["best_ret"])
            if self.action_values:      # the iterations score the same state: their tables pool
                _action_values(dev, self.out, self.table, H * K, M, K, act_ptr, i > 0, self.temperature)
            check(lib.pc_cem_refit(dev.index, self.weights.data_ptr(), self.out["ret"].data_ptr(), self.table.data_ptr(), M, H, K,
                                   self.elites, self.smoothing_shift, self.min_weight, act_ptr, self.best_seq.data_ptr(), stream),
                  "pc_cem_refit")
        return self.out

    def act(self, step_index, done=None):
        """int64 [N]: the first action of each env's best sequence after the last iteration, from its current state."""
        return self.plan(step_index, done=done)["best_action"]

    def drive(self, n_steps, start=0, out=None, done=None):
        """Planner.drive for this planner: step t > 0 plans with the flags step t - 1 wrote (its auto-reset rows restart their
        weights), step 0 with `done` (the flags of the step before this call, or None)."""
        N = self.envs.num_envs
        if out is None:
            out = tuple(torch.empty(int(n_steps), N, dtype=torch.float32, device=self.device) for _ in range(3))
        rew, term, trunc = out
        obs = torch.empty(N, self.envs.obs_dim, dtype=torch.float32, device=self.device)
        for t in range(int(n_steps)):
            self.envs.step(self.act(int(start) + t, done=done), out=(obs, rew[t], term[t], trunc[t]))
            done = term[t] + trunc[t]
        return rew, term, trunc


class PlannerEvaluator:
    """Evaluator's surface (run / totals / scalars / evaluate / close) for a planner instead of a policy: kind = "shooting" (Planner,
    the default) or "cem" (CEMPlanner with elites, iterations, smoothing_shift, min_weight, init_weight, warm_start)."""

    def __init__(self, tracks, n_envs=1024, num_rays=12, reward_scaling=0.1, device="cuda", dtype="f32", track_id=None, horizon=16,
                 candidates=256, seed=0, chunk=250, kind="shooting", elites=8, iterations=4, smoothing_shift=1, min_weight=64,
                 init_weight=7281, warm_start=True, agent=None, gamma=1.0, bootstrap="none"):
        if kind not in ("shooting", "cem"):
            raise ValueError(f"PlannerEvaluator: kind must be 'shooting' or 'cem', not {kind!r}")
        if int(n_envs) < 1:
            raise ValueError(f"PlannerEvaluator: n_envs must be >= 1, not {n_envs!r}")
        if int(chunk) < 1:
            raise ValueError(f"PlannerEvaluator: chunk must be >= 1, not {chunk!r}")
        self.envs = VecCarEnv(int(n_envs), tracks, num_rays=num_rays, reward_scaling=reward_scaling, device=device, dtype=dtype,
                              track_id=track_id)
        self.kind = kind
        try:
            if kind == "cem":
                self.planner = CEMPlanner(self.envs, horizon, candidates, elites, iterations, smoothing_shift, min_weight, init_weight,
                                          warm_start, seed, agent=agent, gamma=gamma, bootstrap=bootstrap)
            else:
                self.planner = Planner(self.envs, horizon, candidates, seed, agent=agent, gamma=gamma, bootstrap=bootstrap)
        except Exception:
            self.envs.close()
            raise
        self.device, self.num_envs, self.reward_scaling = self.envs.device, self.envs.num_envs, float(reward_scaling)
        self.chunk = min(int(chunk), PC_TIME_LIMIT)
        self.state = new_state(self.num_envs, self.device)
        self._state0 = self.state.clone()
        self._range = torch.zeros(1, dtype=torch.int32, device=self.device)      # (no weight image: always inside the domain)
        # the rows of all PC_TIME_LIMIT steps, step layout
        self.rew, self.term, self.trunc = (torch.empty(PC_TIME_LIMIT, self.num_envs, dtype=torch.float32, device=self.device) for _ in range(3))
        self.last_path = None

    @torch.no_grad()
    def run(self, index=0):
        """The first episodes of all envs under the planner -> self.state ([8, N] float64, device).  Step t plans with the table of
        step_index = index * PC_TIME_LIMIT + t.  Enqueues only."""
        self.envs.reset()
        self.state.copy_(self._state0)
        base = int(index) * PC_TIME_LIMIT
        cem = self.kind == "cem"
        if cem:
            self.planner.reset_plan()      # run(index) does not depend on what ran before
        for t0 in range(0, PC_TIME_LIMIT, self.chunk):
            T = min(self.chunk, PC_TIME_LIMIT - t0)
            rows = (self.rew[t0:t0 + T], self.term[t0:t0 + T], self.trunc[t0:t0 + T])
            if cem:      # the step before this window is the row above it
                self.planner.drive(T, start=base + t0, out=rows, done=self.term[t0 - 1] + self.trunc[t0 - 1] if t0 else None)
            else:
                self.planner.drive(T, start=base + t0, out=rows)
            check(lib.pc_first_episodes(self.device.index, rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(), None, None, T,
                                        self.num_envs, PC_EPISODE_STEPS, self.reward_scaling, self.state.data_ptr(),
                                        torch.cuda.current_stream(self.device).cuda_stream), "pc_first_episodes")
        self.last_path = "planner"
        return self.state

    def totals(self):
        """Evaluator.totals() of the planner's episodes: float64 [EVAL_TOTALS] on the device, no host synchronisation."""
        return state_totals(self.state, self._range)

    def scalars(self, host_totals, reward_scaling=None):
        return evaluation_scalars(host_totals, self.reward_scaling if reward_scaling is None else reward_scaling)

    def evaluate(self, index=0):
        """run + fetch: the eval/* dict of one evaluation (synchronises)."""
        self.run(index)
        return self.scalars(self.totals().tolist())

    def close(self):
        self.envs.close()
