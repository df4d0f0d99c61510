"""Distilling the planners into the policy: behaviour cloning of a teacher's actions, with DAgger around it.

bc_loss is the supervised loss in torch ops -- the torch path and the tests' reference, the part ppo_loss plays in ppo.py:
    labelled_i = 0 <= label_i < A
    ce_i  = labelled_i ? -log_softmax(logits_i)[label_i] : 0        ent_i = labelled_i ? entropy(softmax(logits_i)) : 0
    vl_i  = 0.5 (v_i - target_i)^2
    loss  = (sum ce_i + vf_coef * sum vl_i - ent_coef * sum ent_i) / B
The divisor is always B; a label outside 0 .. A-1 is "no label" (the planners' doomed states carry -1).
bc_soft_loss is the same loss against a row of probabilities p_i [A] (pc_sequences_action_values' target): w_i = sum_k p_ik,
labelled_i = w_i > 0 (an all-zero or NaN row is "no label"), ce_i = -sum_k p_ik log_softmax(logits_i)[k]; a one-hot row gives bc_loss.

BCLearner owns the flat parameter bucket and a device-side Adam, as PPOLearner does, and takes one minibatch per step(): on the
GPU with the standard 256-wide agent pc_bc_minibatch (K27 + K11 + K12: no library GEMM, fixed summation order), otherwise bc_loss +
autograd + clip_grad_norm_ + torch.optim.Adam(eps=1e-5).  A 2-D label [M, A] is a table of soft targets: pc_bc_minibatch_soft /
bc_soft_loss.

PlannerDistiller runs DAgger on its own VecCarEnv: per round, `steps_per_round` steps from a reset in which the teacher (Planner /
CEMPlanner on the env's exact model) labels every env's current state and env i executes the teacher's action if it belongs to the
teacher's share of the round (teacher_envs), the student's sampled action otherwise; then BCLearner.fit on the labelled states.
labels="soft": the teacher also reports what the best sequence beginning with each action earned (K28) and the student is fitted to
the soft row over the actions -- exact ties share the mass -- while the envs execute what they execute under labels="best"."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._capi import PC_FIRST_TERMINATED, check, lib
from .env import VecCarEnv
from .planner import CEMPlanner, Planner
from .ppo import flatten_parameters


def bc_loss(agent, obs, label, target, vf_coef, ent_coef):
    """(total, ce, vl, ent) of one minibatch, any device and dtype.  label [B] of any real dtype; target [B] or None (vl = 0)."""
    logits = agent.actor(obs)
    B, A = logits.shape
    logp = F.log_softmax(logits, dim=-1)
    labelled = (label >= 0) & (label < A)
    a = torch.where(labelled, label, torch.zeros_like(label)).to(torch.int64)
    w = labelled.to(logits.dtype)
    ce = -(logp.gather(1, a.view(-1, 1)).view(-1) * w).sum() / B
    safe = torch.clamp(logp, min=torch.finfo(logp.dtype).min)      # (Categorical.entropy's guard: 0 * -inf)
    ent = (-(safe.exp() * safe).sum(-1) * w).sum() / B
    if target is None:
        vl = torch.zeros((), dtype=logits.dtype, device=logits.device)
    else:
        vl = 0.5 * ((agent.critic(obs).view(-1) - target) ** 2).sum() / B
    return ce + vf_coef * vl - ent_coef * ent, ce, vl, ent


def bc_soft_loss(agent, obs, soft, target, vf_coef, ent_coef):
    """(total, ce, vl, ent) of one minibatch against soft targets, any device and dtype.  soft [B, A]; target [B] or None (vl = 0)."""
    logits = agent.actor(obs)
    B, A = logits.shape
    logp = F.log_softmax(logits, dim=-1)
    w = soft.sum(-1)
    labelled = w > 0      # (a NaN row fails the comparison)
    on = labelled.to(logits.dtype)
    safe = torch.clamp(logp, min=torch.finfo(logp.dtype).min)      # (Categorical.entropy's guard: 0 * -inf)
    p = torch.where(labelled.view(-1, 1), soft, torch.zeros_like(soft))
    ce = -(p * safe).sum(-1).sum() / B      # (row by row: a one-hot row's sum is log p of its action, bc_loss's term)
    ent = (-(safe.exp() * safe).sum(-1) * on).sum() / B
    if target is None:
        vl = torch.zeros((), dtype=logits.dtype, device=logits.device)
    else:
        vl = 0.5 * ((agent.critic(obs).view(-1) - target) ** 2).sum() / B
    return ce + vf_coef * vl - ent_coef * ent, ce, vl, ent


def teacher_envs(n_envs, beta):
    """The teacher's share of the envs, bool [n_envs] (numpy): a pure function of (i, n_envs, beta), no random draw.
    Env i is the teacher's iff rank(i) < round(beta * n_envs) with rank(i) = (i * g) mod n_envs, g the smallest integer
    >= max(1, floor(0.618 n_envs)) coprime to n_envs.  rank is a permutation of 0 .. n_envs - 1, so exactly round(beta * n_envs) envs
    (Python's round) are the teacher's, the set at a smaller beta is a subset of the set at a larger one, and the golden-ratio stride
    spreads every share evenly over the env index (and so over the tracks of a mixed-track handle)."""
    n = int(n_envs)
    if n < 1:
        raise ValueError(f"teacher_envs: n_envs must be >= 1, not {n_envs!r}")
    if not 0.0 <= float(beta) <= 1.0:
        raise ValueError(f"teacher_envs: beta must be in 0 .. 1, not {beta!r}")
    g = max(1, int(0.6180339887498949 * n))
    while math.gcd(g, n) != 1:
        g += 1
    rank = (np.arange(n, dtype=np.int64) * g) % n
    return rank < round(float(beta) * n)


class BCLearner:
    KEYS = ("bc/ce", "bc/value_loss", "bc/entropy", "bc/loss")

    def __init__(self, agent, learning_rate=3e-4, batch_size=512, vf_coef=0.0, ent_coef=0.0, max_grad_norm=0.5, seed=0, device="cuda",
                 custom_mlp=True):
        if int(batch_size) != batch_size or int(batch_size) < 1:
            raise ValueError(f"BCLearner: batch_size must be a positive integer, not {batch_size!r}")
        if not vf_coef >= 0.0 or not ent_coef >= 0.0:
            raise ValueError(f"BCLearner: vf_coef and ent_coef must be >= 0, not {vf_coef!r} / {ent_coef!r}")
        self.agent, self.device = agent.to(device), torch.device(device)
        self.learning_rate, self.batch_size = float(learning_rate), int(batch_size)
        self.vf_coef, self.ent_coef, self.max_grad_norm, self.seed = float(vf_coef), float(ent_coef), float(max_grad_norm), int(seed)
        self.flat_param, self.flat_grad = flatten_parameters(agent)
        self.device = self.flat_param.device
        cuda = self.device.type == "cuda"
        hand = cuda and bool(custom_mlp) and agent._std_mlp() and agent.actor[0].out_features == 256
        self._dha = (agent.actor[0].in_features, 256, agent.actor[2].out_features) if hand else None
        # "custom": pc_bc_minibatch; "torch": bc_loss + autograd + clip_grad_norm_ + Adam.  Decided here, once.
        self.path = "custom" if hand and lib.pc_ppo_workspace_floats(self.batch_size, *self._dha) > 0 else "torch"
        if self.path == "custom":
            self.exp_avg = torch.zeros_like(self.flat_param)
            self.exp_avg_sq = torch.zeros_like(self.flat_param)
            self.step_count = torch.zeros(1, device=self.device)
            self.lr_dev = torch.full((1,), self.learning_rate, device=self.device, dtype=torch.float32)
            self._ws = torch.empty(lib.pc_ppo_workspace_floats(self.batch_size, *self._dha), device=self.device, dtype=torch.float32)
            self.optimizer = None
        else:
            self.optimizer = torch.optim.Adam(agent.parameters(), lr=self.learning_rate, eps=1e-5)
        self.metrics = torch.zeros(4, device=self.device)
        self.steps = 0
        self._np_rng = np.random.default_rng(self.seed)

    def _need_target(self, target):
        if target is None and self.vf_coef != 0.0:
            raise ValueError("BCLearner: vf_coef != 0 needs the critic's targets")

    def step(self, idx, obs, label, target=None):
        """One minibatch: idx int64 [batch_size] into obs [M, D], label [M] float32 (act_buf's layout) or [M, A] float32 (soft targets,
        row-major), target [M] float32 or None.  metrics += (ce, vl, ent, total); enqueues only."""
        self._need_target(target)
        if idx.numel() != self.batch_size:
            raise ValueError(f"BCLearner.step: idx must hold batch_size = {self.batch_size} indices, got {idx.numel()}")
        soft = label.dim() == 2
        if label.dim() > 2 or (soft and label.shape[1] != self.agent.actor[2].out_features):
            raise ValueError(f"BCLearner.step: label must be [M] or [M, {self.agent.actor[2].out_features}], not {tuple(label.shape)}")
        if self.path == "custom":
            for name, t in (("idx", idx), ("obs", obs), ("label", label), ("target", target)):
                want = torch.int64 if name == "idx" else torch.float32
                if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == want):
                    raise ValueError(f"BCLearner.step: {name} must be a contiguous {want} tensor on the device")
            if (obs.dim() != 2 or obs.shape[1] != self._dha[0] or label.numel() != obs.shape[0] * (self._dha[2] if soft else 1)
                    or (target is not None and target.numel() != obs.shape[0])):
                raise ValueError("BCLearner.step: obs must be [M, D], label [M] or [M, A] and target [M]")
            di = self.device.index if self.device.index is not None else torch.cuda.current_device()
            step, name = (lib.pc_bc_minibatch_soft, "pc_bc_minibatch_soft") if soft else (lib.pc_bc_minibatch, "pc_bc_minibatch")
            check(step(di, idx.data_ptr(), self.batch_size, *self._dha, obs.data_ptr(), label.data_ptr(),
                       target.data_ptr() if target is not None else None, self.flat_param.data_ptr(), self.flat_grad.data_ptr(),
                       self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.step_count.data_ptr(), self.lr_dev.data_ptr(),
                       self.vf_coef, self.ent_coef, self.max_grad_norm, 0.9, 0.999, 1e-5, self.metrics.data_ptr(),
                       self._ws.data_ptr(), 1, torch.cuda.current_stream(self.device).cuda_stream), name)
        else:
            loss, ce, vl, ent = (bc_soft_loss if soft else bc_loss)(self.agent, obs[idx], label[idx], None if target is None else target[idx],
                                                                    self.vf_coef, self.ent_coef)
            self.flat_grad.zero_()
            loss.backward()
            nn.utils.clip_grad_norm_(self.agent.parameters(), self.max_grad_norm)
            self.optimizer.step()
            with torch.no_grad():
                self.metrics += torch.stack([ce.detach(), vl.detach(), ent.detach(), loss.detach()]).to(self.metrics.dtype)
        self.steps += 1
        self.agent._image_ok = False      # the packed policy image is stale: the next act() packs again

    def draw_indices(self, M, epochs=1):
        """int64 [epochs, (M // batch_size) * batch_size] on the device: per epoch a host-side permutation of M from
        np.random.default_rng(seed), cut to full minibatches (PPOLearner.draw_indices' scheme)."""
        K = (M // self.batch_size) * self.batch_size
        if K == 0:
            raise ValueError(f"BCLearner.fit: {M} samples hold no full minibatch of {self.batch_size}")
        host = np.stack([self._np_rng.permutation(M)[:K] for _ in range(int(epochs))]).astype(np.int64)
        return torch.from_numpy(host).to(self.device)

    def fit(self, obs, label, target=None, epochs=1):
        """epochs x (M // batch_size) minibatch steps over obs [M, D] / label [M] or [M, A] (/ target [M]); the bc/* scalars as means over
        the steps taken.  One fetch, at the end."""
        self._need_target(target)
        idx = self.draw_indices(obs.shape[0], epochs)
        self.metrics.zero_()
        B, n = self.batch_size, 0
        for e in range(idx.shape[0]):
            for m in range(idx.shape[1] // B):
                self.step(idx[e, m * B:(m + 1) * B], obs, label, target)
                n += 1
        out = {k: v / n for k, v in zip(self.KEYS, self.metrics.tolist())}
        out["bc/steps"] = n
        return out

    def state_dict(self):
        sd = {"path": self.path, "param": self.flat_param.detach().clone(), "steps": self.steps, "rng": self._np_rng.bit_generator.state}
        if self.path == "custom":
            sd.update(exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(), step_count=self.step_count.clone(),
                      lr_dev=self.lr_dev.clone())
        else:
            sd["optimizer"] = self.optimizer.state_dict()
        return sd

    def load_state_dict(self, sd):
        if sd["path"] != self.path:
            raise ValueError(f"BCLearner.load_state_dict: the state was saved on the {sd['path']!r} path, this learner runs {self.path!r}")
        with torch.no_grad():
            self.flat_param.copy_(sd["param"])
            if self.path == "custom":
                for k in ("exp_avg", "exp_avg_sq", "step_count", "lr_dev"):
                    getattr(self, k).copy_(sd[k])
        if self.path != "custom":
            self.optimizer.load_state_dict(sd["optimizer"])
        self.steps = int(sd["steps"])
        self._np_rng.bit_generator.state = sd["rng"]
        self.agent._image_ok = False


class PlannerDistiller:
    """DAgger with a planner as the teacher.  planner: dict(kind="cem" | "shooting", ...) -- everything but `kind` goes to CEMPlanner /
    Planner as keywords (horizon, candidates, elites, iterations, ..., and agent=, gamma=, bootstrap= for a critic-bootstrapped
    teacher; seed defaults to this distiller's).  learner: BCLearner's keywords.  rounds: how many rounds' rows are allocated.
    reward_scaling is the env's, and so the scale of the returns the teacher compares: with a bootstrap it must be the one the
    teacher agent's critic was trained at (PPOConfig's default, 0.1).
    labels: "best" -- the first action of the teacher's best sequence, a hard label -- or "soft": the teacher is built with
    action_values=True, temperature=label_temperature, its soft row of every state goes to soft_buf [rounds, T, N, 9] beside label_buf
    (filled as under "best") and train() fits on soft_buf.  The temperature is in units of the SCALED return (reward_scaling).

    Round r: the teacher's share is beta_r = beta0 * beta_decay^r of the envs (teacher_envs); step t of the round plans with
    step_index = r * steps_per_round + t and the student samples from the stream (agent.rng_seed, offset = step_index)."""

    def __init__(self, agent, tracks, n_envs=1024, num_rays=16, planner=None, steps_per_round=250, beta0=1.0, beta_decay=0.5,
                 epochs_per_round=4, aggregate=True, learner=None, seed=0, device="cuda", dtype="f32", rounds=8, reward_scaling=0.1,
                 labels="best", label_temperature=0.0):
        if labels not in ("best", "soft"):
            raise ValueError(f"PlannerDistiller: labels must be 'best' or 'soft', not {labels!r}")
        self.labels, self.label_temperature = labels, float(label_temperature)
        if not (0.0 <= self.label_temperature < float("inf")):      # (NaN fails both comparisons)
            raise ValueError(f"PlannerDistiller: label_temperature must be finite and >= 0, not {label_temperature!r}")
        if labels == "best" and self.label_temperature != 0.0:
            raise ValueError("PlannerDistiller: label_temperature needs labels='soft'")
        if int(steps_per_round) < 1 or int(rounds) < 1 or int(epochs_per_round) < 1:
            raise ValueError("PlannerDistiller: steps_per_round, rounds and epochs_per_round must be >= 1")
        if not 0.0 <= float(beta0) <= 1.0 or not 0.0 <= float(beta_decay) <= 1.0:
            raise ValueError(f"PlannerDistiller: beta0 and beta_decay must be in 0 .. 1, not {beta0!r} / {beta_decay!r}")
        pk = dict(planner if planner is not None else dict(kind="cem"))
        self.kind = pk.pop("kind", "cem")
        if self.kind not in ("shooting", "cem"):
            raise ValueError(f"PlannerDistiller: planner kind must be 'shooting' or 'cem', not {self.kind!r}")
        pk.setdefault("seed", seed)
        if labels == "soft":
            pk.update(action_values=True, temperature=self.label_temperature)
        lk = dict(learner if learner is not None else {})
        lk.setdefault("seed", seed)
        self.learner = BCLearner(agent, device=device, **lk)
        self.agent = agent
        self.envs = VecCarEnv(int(n_envs), tracks, num_rays=num_rays, reward_scaling=reward_scaling, device=device, dtype=dtype)
        try:
            self.planner = (CEMPlanner if self.kind == "cem" else Planner)(self.envs, **pk)
        except Exception:
            self.envs.close()
            raise
        self.device = self.envs.device
        self.steps_per_round, self.rounds, self.epochs_per_round = int(steps_per_round), int(rounds), int(epochs_per_round)
        self.beta0, self.beta_decay, self.aggregate = float(beta0), float(beta_decay), bool(aggregate)
        T, N, D, dev = self.steps_per_round, self.envs.num_envs, self.envs.obs_dim, self.device
        # every round's rows, allocated up front: observations and the teacher's labels (float32: act_buf's layout; -1 = no label)
        self.obs_buf = torch.empty(self.rounds, T, N, D, dtype=torch.float32, device=dev)
        self.label_buf = torch.empty(self.rounds, T, N, dtype=torch.float32, device=dev)
        self.rew, self.term, self.trunc = (torch.empty(T, N, dtype=torch.float32, device=dev) for _ in range(3))      # the last round's
        self._obs = torch.empty(N, D, dtype=torch.float32, device=dev)
        self._student = torch.empty(N, dtype=torch.int64, device=dev)
        self._greedy = torch.empty(T * N, dtype=torch.int64, device=dev)
        self._no_label = torch.full((N,), -1, dtype=torch.int64, device=dev)
        if labels == "soft":
            self.soft_buf = torch.empty(self.rounds, T, N, self.envs.act_dim, dtype=torch.float32, device=dev)
            self._soft_stats = torch.zeros(3, dtype=torch.float64, device=dev)      # the round's non-zero rows, tied rows, entropy sum

    def beta(self, r):
        return self.beta0 * self.beta_decay ** int(r)

    @torch.no_grad()
    def collect(self, r):
        """steps_per_round steps from a reset under the round's mixture; fills obs_buf[r], label_buf[r], rew / term / trunc.
        Enqueues only."""
        r = int(r)
        if not 0 <= r < self.rounds:
            raise ValueError(f"PlannerDistiller.collect: round {r} outside the {self.rounds} allocated")
        T, N = self.steps_per_round, self.envs.num_envs
        share = teacher_envs(N, self.beta(r))
        mixed = not bool(share.all())
        teacher = torch.from_numpy(share).to(self.device) if mixed else None
        cem = self.kind == "cem"
        obs, done = self._obs, None
        self.envs.reset(out=obs)
        if cem:
            self.planner.reset_plan()
        soft = self.labels == "soft"
        if soft:
            self._soft_stats.zero_()
        for t in range(T):
            step_index = r * T + t
            ta = self.planner.act(step_index, done=done) if cem else self.planner.act(step_index)
            out = self.planner.out
            bk = out["best_k"].to(torch.int64).view(-1, 1)
            # a state whose best sequence crashes on its first step has no action worth imitating: every sequence crashes there
            doomed = (out["status"].gather(1, bk).view(-1) == PC_FIRST_TERMINATED) & (out["steps"].gather(1, bk).view(-1) == 1)
            self.obs_buf[r, t].copy_(obs)
            self.label_buf[r, t].copy_(torch.where(doomed, self._no_label, ta))
            if soft:
                p = out["soft"]
                self.soft_buf[r, t].copy_(p)
                top = p.max(-1).values
                some = top > 0
                ent = -(p * torch.log(torch.where(p > 0, p, torch.ones_like(p)))).sum(-1)
                self._soft_stats += torch.stack([some.sum(), (some & ((p == top.view(-1, 1)).sum(-1) >= 2)).sum(),
                                                 ent.sum()]).to(torch.float64)
            action = ta
            if mixed:
                self.agent.act(obs, out_action=self._student, offset=step_index, repack=t == 0)      # (the weights rest while collecting)
                action = torch.where(teacher, ta, self._student)
            self.envs.step(action, out=(obs, self.rew[t], self.term[t], self.trunc[t]))
            done = self.term[t] + self.trunc[t]

    @torch.no_grad()
    def measure(self, r, chunk=65536):
        """Device tensor [2]: (labelled states of round r whose label the student's greedy action equals, labelled states).
        labels="soft": a state is labelled where its soft row is non-zero, and the student agrees where its greedy action is one of
        the row's maximal entries."""
        T, N, D = self.steps_per_round, self.envs.num_envs, self.envs.obs_dim
        obs, label = self.obs_buf[r].view(T * N, D), self.label_buf[r].view(T * N)
        for i in range(0, T * N, chunk):
            self.agent.act(obs[i:i + chunk], out_action=self._greedy[i:i + chunk], greedy=True, repack=i == 0)
        if self.labels == "soft":
            p = self.soft_buf[r].view(T * N, -1)
            top = p.max(-1).values
            labelled = top > 0
            hit = p.gather(1, self._greedy.view(-1, 1)).view(-1) == top
            return torch.stack([(hit & labelled).sum(), labelled.sum()]).to(torch.float64)
        labelled = (label >= 0) & (label < self.envs.act_dim)
        return torch.stack([((self._greedy.to(torch.float32) == label) & labelled).sum(), labelled.sum()]).to(torch.float64)

    def train(self, r):
        """BCLearner.fit on round r's rows, or with aggregate on the rows of rounds 0 .. r."""
        T, N, D = self.steps_per_round, self.envs.num_envs, self.envs.obs_dim
        lo = 0 if self.aggregate else int(r)
        rows = (int(r) + 1 - lo) * T * N
        if self.labels == "soft":
            return self.learner.fit(self.obs_buf[lo:int(r) + 1].view(rows, D), self.soft_buf[lo:int(r) + 1].view(rows, -1),
                                    epochs=self.epochs_per_round)
        return self.learner.fit(self.obs_buf[lo:int(r) + 1].view(rows, D), self.label_buf[lo:int(r) + 1].view(rows), epochs=self.epochs_per_round)

    def round(self, r):
        """collect, measure, train -> the bc/* scalars, bc/agreement (the share of this round's labelled states where the student's
        greedy action equals the label, measured BEFORE training on them; 0 when nothing is labelled), bc/beta, bc/labelled.
        labels="soft" adds bc/ties (the share of the round's non-zero soft rows in which two or more entries equal the row's maximum)
        and bc/label_entropy (the mean entropy of those rows, nats)."""
        self.collect(r)
        stats = self.measure(r)
        soft_stats = self._soft_stats.tolist() if self.labels == "soft" else None
        out = self.train(r)
        if soft_stats is not None:
            rows, tied, ent = soft_stats
            out["bc/ties"] = tied / rows if rows > 0 else 0.0
            out["bc/label_entropy"] = ent / rows if rows > 0 else 0.0
        agree, labelled = stats.tolist()
        out["bc/agreement"] = agree / labelled if labelled > 0 else 0.0
        out["bc/beta"] = self.beta(r)
        out["bc/labelled"] = labelled / (self.steps_per_round * self.envs.num_envs)
        return out

    def close(self):
        self.envs.close()
