"""The soft-target imitation step (pc_bc_minibatch_soft: the LOSS_BC_SOFT head + K11 + K12) restated: the inputs of every case, the
float64 reference (imitation.bc_soft_loss on a .double() copy of the agent, clip_grad_norm_, torch.optim.Adam(lr 3e-4, eps 1e-5)), the
same steps in float32 torch on the CPU (the yardstick of the input conditions; never the code under test) and the two deliberately
wrong float64 gradients of the sensitivity condition.  Shapes, bars, allowances and `Call` are tests/ppo_update_reference.py's, the
agent, pool, obs, targets and index vectors tests/bc_update_reference.py's: nothing of them is restated here.

The soft table of a case, [pool, A]: row i = softmax(q_i / T_i), q_i ~ 0.3 N(0, 1), T_i drawn from {0.02, 0.1, 1}.  The first minibatch
is bc_update_reference's, whose hand-placed rows become:
  row 0 (sample 0)                an all-zero row: no label
  row pool - 1 (sample 1)         the one-hot row on A - 1          (B = 2: the genuinely soft LAST_ROW's recipe instead, see below)
  row 2 (samples 2 and 3)         a duplicate
  row 3 (sample 4, B >= 7)        half a softmax row: its sum is 0.5, w != 1
  B mod 8 != 0: the last sample is row LAST_ROW (B = 2: row pool - 1) = softmax(q) at T = 1 with its largest entry <= 0.9 (asserted;
      A = 1 has no soft row: [1]), and with B mod 8 >= 2 and B >= 7 the sample before it is row UNLABELLED_ROW, all zero: a live
      unlabelled sample next to live soft ones in the partly dead group.  (B mod 8 = 1: the last group's only live sample is the soft
      one; B = 2, 3: sample 0's zero row is in the same group.)"""
import functools

import numpy as np
import torch

import bc_update_reference as Q
import ppo_update_reference as R
from ppo_update_reference import (APPLIED, GRAD_ATOL, GRAD_RTOL, MET_ABS, MET_REL, PARAM_ATOL, Call, allowance, n_param, slice_bounds,  # noqa: F401
                                  worst, worst_by_slice)
from bc_update_reference import BC_IDLE_NORM, BC_MAX_NORM, LAST_ROW, UNLABELLED_ROW, actor_end, metric_worst  # noqa: F401
from ppo_car_amd import _capi
from ppo_car_amd.imitation import bc_soft_loss

VF, EC, LR = R.VF, R.EC, R.LR
HALF_ROW = 3
TEMPERATURES = (0.02, 0.1, 1.0)
COMPILED = [s for s in R.COMPILED if s[0] in (2, 7, 8, 9, 257, 1023, 1024)]
assert sorted(s[0] for s in COMPILED) == [2, 7, 8, 9, 257, 1023, 1024]
GENERIC = [(2, 1, 1), (9, 1, 15), (65, 25, 2), (1023, 40, 15), (33, 40, 1), (513, 7, 3)]
SHAPES = COMPILED + GENERIC
ONE_ACTION = [s for s in SHAPES if s[2] == 1]
ONE_HOT_SHAPES = [(2, 23, 9), (9, 39, 9), (257, 39, 9), (1023, 40, 15), (65, 25, 2), (33, 40, 1)]
# The case table: the seed of a shape's soft rows (default 5000 + B) where the default breaks an input condition of
# tests/test_bc_soft_f64_host.py
SEEDS = {}
# (shape, scale, steps, max_norm) of every case tests/test_bc_soft_f64_gpu.py runs against float64; tests/test_bc_soft_f64_host.py holds
# each to the input conditions
ONE_STEP = [(s, scale, 1, BC_MAX_NORM) for scale in (1.0, 40.0) for s in SHAPES]
MULTI = [(s, 1.0, 4, mn) for s in APPLIED for mn in (BC_MAX_NORM, BC_IDLE_NORM)]


def ids(cases):
    return [f"B{s[0]}-D{s[1]}-A{s[2]}-x{scale:g}-n{steps}-norm{mn:g}" for s, scale, steps, mn in cases]


@functools.lru_cache(maxsize=None)
def inputs(B, D, A, scale=1.0, steps=1):
    """bc_update_reference.inputs' case with the soft table under `soft` (float32 [pool, A]; read-only, shared)"""
    c = dict(Q.inputs(B, D, A, scale, steps))
    pool = c["pool"]
    g = torch.Generator().manual_seed(SEEDS.get((B, D, A), 5000 + B))
    q = 0.3 * torch.randn(pool, A, generator=g, dtype=torch.float64)
    T = torch.tensor(TEMPERATURES, dtype=torch.float64)[torch.randint(0, 3, (pool,), generator=g)]
    last = pool - 1 if B == 2 else LAST_ROW
    T[last] = 1.0
    soft = torch.softmax(q / T.view(-1, 1), -1)
    soft[0] = 0.0
    if B > 2:
        soft[pool - 1] = 0.0
        soft[pool - 1, A - 1] = 1.0
    idx = [ix.clone() for ix in c["idx"]]
    if B >= 7:
        idx[0][4] = HALF_ROW
        soft[HALF_ROW] *= 0.5
        if B % 8 >= 2:
            assert int(idx[0][B - 2]) == UNLABELLED_ROW
            soft[UNLABELLED_ROW] = 0.0
    if B % 8 != 0:
        assert int(idx[0][B - 1]) == last
        assert A == 1 or float(soft[last].max()) <= 0.9, (B, D, A, float(soft[last].max()))
    c["idx"], c["soft"] = idx, soft.float().contiguous()
    del c["label"]
    return c


def _cat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).double().numpy().copy()


def run_steps(c, max_norm=BC_MAX_NORM, dtype=torch.float64, vf=VF, ec=EC, targets=True, soft=None):
    """bc_soft_loss -> backward -> clip_grad_norm_ -> Adam over the case's minibatches in `dtype` on the CPU: bc_update_reference.run_steps'
    dict per step.  soft: a table to use instead of the case's."""
    a = R._agent_as(c, dtype)
    opt = torch.optim.Adam(a.parameters(), lr=LR, eps=1e-5)
    table = c["soft"] if soft is None else soft
    out = []
    for ix in c["idx"]:
        obs, p, target = c["obs"][ix].to(dtype), table[ix].to(dtype), c["target"][ix].to(dtype)
        for q in a.parameters():      # (zeros, not None: without targets the critic's gradient is 0 and Adam still visits it)
            q.grad = torch.zeros_like(q)
        total, ce, vl, ent = bc_soft_loss(a, obs, p, target if targets else None, vf, ec)
        total.backward()
        raw = _cat([q.grad for q in a.parameters()])
        norm = float(torch.nn.utils.clip_grad_norm_(a.parameters(), max_norm))
        clipped = _cat([q.grad for q in a.parameters()])
        opt.step()
        params = list(a.parameters())
        out.append(dict(grad=raw, grad_clipped=clipped, norm=norm, metrics=np.array([float(t.detach()) for t in (ce, vl, ent, total)]),
                        param=_cat(params), exp_avg=_cat([opt.state[q]["exp_avg"] for q in params]),
                        exp_avg_sq=_cat([opt.state[q]["exp_avg_sq"] for q in params])))
    return out


@functools.lru_cache(maxsize=None)
def case(B, D, A, scale=1.0, steps=1, max_norm=BC_MAX_NORM):
    """The inputs of a case with its float64 reference under `ref` (one entry per step); computed once, shared, read-only."""
    c = dict(inputs(B, D, A, scale, steps))
    c["max_norm"] = max_norm
    c["ref"] = run_steps(c, max_norm)
    return c


@functools.lru_cache(maxsize=None)
def restated32(B, D, A, scale=1.0, steps=1, max_norm=BC_MAX_NORM):
    """the same steps in float32 torch on the CPU"""
    return run_steps(inputs(B, D, A, scale, steps), max_norm, torch.float32)


def gradient_of(c, weight=None, rows=None):
    """The first minibatch's loss written out per sample (bc_soft_loss's operations) in float64: the flat gradient of
    sum_i weight_i (labelled_i (ce_i - EC ent_i) + VF vl_i) / B.  weight: per-sample weights (a 0 drops the sample, the divisor stays B).
    rows: the B soft rows to use instead of the case's.  With neither this is bc_soft_loss's gradient (the host test holds the two to
    each other)."""
    dtype = torch.float64
    a = R._agent_as(c, dtype)
    ix = c["idx"][0]
    obs, target = c["obs"][ix].to(dtype), c["target"][ix].to(dtype)
    p = (c["soft"][ix] if rows is None else rows).to(dtype)
    B = c["B"]
    w = torch.ones(B, dtype=dtype) if weight is None else torch.as_tensor(weight, dtype=dtype)
    logp = torch.log_softmax(a.actor(obs), -1)
    on = (p.sum(-1) > 0).to(dtype)
    ce = -(p * logp).sum(-1)
    ent = -(logp.exp() * logp).sum(-1)
    val = 0.5 * (a.critic(obs).view(-1) - target) ** 2
    ((w * (on * (ce - EC * ent) + VF * val)).sum() / B).backward()
    return torch.cat([(q.grad if q.grad is not None else torch.zeros_like(q)).reshape(-1) for q in a.parameters()]).double().numpy()


def last_row_is_soft(c):
    """the first minibatch's last sample carries a row that is neither zero nor (nearly) one-hot"""
    p = c["soft"][c["idx"][0][-1]]
    return c["A"] >= 2 and 0.0 < float(p.max()) <= 0.9 * float(p.sum())


def wrong_gradients(c):
    """(the last sample dropped, the divisor still B -- what a partly dead workgroup would lose; the last sample's soft row replaced by
    its arg-max one-hot -- what a head that reads a hard label out of the row would give, or None where that row is not soft)"""
    B = c["B"]
    w = np.ones(B)
    w[B - 1] = 0.0
    hard = None
    if last_row_is_soft(c):
        rows = c["soft"][c["idx"][0]].clone()
        a = int(rows[B - 1].argmax())
        rows[B - 1] = 0.0
        rows[B - 1, a] = 1.0
        hard = gradient_of(c, rows=rows)
    return gradient_of(c, weight=w), hard


def one_hot(label, A):
    """float32 [M, A]: the one-hot row of every label in 0 .. A - 1, a zero row for any other"""
    on = (label >= 0) & (label < A)
    rows = torch.zeros(label.numel(), A)
    rows[on, label[on].long()] = 1.0
    return rows.contiguous()


def soft_call(call, idx, obs, soft, target, vf=VF, ec=EC, apply=0):
    """pc_bc_minibatch_soft on a ppo_update_reference.Call's device state"""
    return call._done(_capi.lib.pc_bc_minibatch_soft(0, idx.data_ptr(), call.B, call.D, 256, call.A, obs.data_ptr(), soft.data_ptr(),
                                                     target.data_ptr() if target is not None else None, *call._state(), vf, ec, call.max_norm, 0.9,
                                                     0.999, 1e-5, call.metrics.data_ptr(), call.ws.data_ptr(), apply,
                                                     torch.cuda.current_stream().cuda_stream), "pc_bc_minibatch_soft")
