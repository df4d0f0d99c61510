"""A model-based baseline: receding-horizon random shooting on the env's own exact model (pc_env_rollout_sequences_state, K22).

Planner.act(step_index) scores `candidates` action sequences of `horizon` steps from every env's CURRENT state in one launch and
returns, per env, the first action of the best one (the lowest index on ties).  The candidate table is shared by all envs, uint8,
time-major [H, K]:
  k = 0 .. 8   "hold action k for H steps"
  k >= 9       drawn by pc_sample on all-zero logits [H * K][9] with (seed, offset = step_index): entry (t, k) is element t * K + k of
               that call -- the library's documented Philox stream (include/ppocar.h, "The stream"), so a host can regenerate the table.
Nothing is learned and nothing synchronises: a draw, the overwrite of the nine constant columns, the scoring launches.

PlannerEvaluator is the Evaluator's counterpart for the planner: the first episodes of N fresh envs, PC_TIME_LIMIT steps of act() +
pc_env_step, pc_first_episodes over windows, reported through evaluation_scalars -- the same eval/* keys a policy evaluation prints, so
a trained policy's lap and crash figures have something to stand beside."""
import torch

from ._capi import PC_EPISODE_STEPS, PC_SEQ_MAX_CANDIDATES, PC_TIME_LIMIT, check, lib
from .env import VecCarEnv
from .evaluation import evaluation_scalars, new_state, state_totals

N_ACTIONS = 9


class Planner:
    def __init__(self, envs, horizon=16, candidates=256, seed=0):
        if not 1 <= int(horizon) <= PC_TIME_LIMIT:
            raise ValueError(f"Planner: horizon must be 1 .. {PC_TIME_LIMIT}, not {horizon!r}")
        if not N_ACTIONS <= int(candidates) <= PC_SEQ_MAX_CANDIDATES:
            raise ValueError(f"Planner: candidates must be {N_ACTIONS} (the constant sequences) .. {PC_SEQ_MAX_CANDIDATES}, not {candidates!r}")
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
        self.envs.score_sequences(self.candidate_table(step_index), out=self.out)
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


class PlannerEvaluator:
    """Evaluator's surface (run / totals / scalars / evaluate / close) for a shooting planner instead of a policy."""

    def __init__(self, tracks, n_envs=1024, num_rays=12, reward_scaling=0.1, device="cuda", dtype="f32", track_id=None, horizon=16,
                 candidates=256, seed=0, chunk=250):
        if int(n_envs) < 1:
            raise ValueError(f"PlannerEvaluator: n_envs must be >= 1, not {n_envs!r}")
        if int(chunk) < 1:
            raise ValueError(f"PlannerEvaluator: chunk must be >= 1, not {chunk!r}")
        self.envs = VecCarEnv(int(n_envs), tracks, num_rays=num_rays, reward_scaling=reward_scaling, device=device, dtype=dtype,
                              track_id=track_id)
        try:
            self.planner = Planner(self.envs, horizon, candidates, seed)
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
        for t0 in range(0, PC_TIME_LIMIT, self.chunk):
            T = min(self.chunk, PC_TIME_LIMIT - t0)
            rows = (self.rew[t0:t0 + T], self.term[t0:t0 + T], self.trunc[t0:t0 + T])
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
