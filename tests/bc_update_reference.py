"""The imitation step (pc_bc_minibatch: K27 + K11 + K12) restated: the inputs of every edge-shape case, the float64 reference
(imitation.bc_loss on a .double() copy of the agent, clip_grad_norm_, torch.optim.Adam(lr 3e-4, eps 1e-5)) over consecutive minibatches,
the same steps in float32 torch on the CPU (the yardstick of the input conditions; never the code under test), the four deliberately
wrong float64 gradients of the sensitivity condition, the table of label values at the edges of "labelled", and the agreeing-labels
case.  Shapes, bars, allowances and `Call` are tests/ppo_update_reference.py's: nothing of it is restated here.

Inputs of a case (B, D, A, scale, steps): a pool of B + 7 rows, Agent(D, A) at its seeded initial weights with actor[2] multiplied by
`scale`, obs uniform in [-1, 1.6], label = randint(-1, A) as float32 (about 1 / (A + 1) of the rows carry no label), target = N(0, 1),
`steps` index vectors drawn WITH replacement.  The first minibatch is then arranged by hand:
  B >= 4: its first four indices are (0, pool - 1, 2, 2) -- the first row, the last row, a duplicate -- with labels -1, A - 1 and 0;
  B = 2, 3: its first two indices are (0, pool - 1) with labels -1 and A - 1;
  B mod 8 != 0 and B >= 3: its last sample is row 4, labelled (argmax of the row's float64 logits + 1) mod A, so the sample a partly
      dead workgroup would lose moves the actor as well as the critic; from B = 7 on with B mod 8 >= 2 the sample before it is row 5
      without a label, so the last group holds a live unlabelled sample next to live labelled ones.  (B mod 8 = 1: the last group has
      ONE live sample, the labelled one; its unlabelled lanes are the seven dead ones.  B = 2: the last sample is row pool - 1 with
      label A - 1, and the seed is one at which that is not the row's argmax.)
agree = True: every row's label is the argmax of its own float64 logits instead (no unlabelled row): -log p is as small as it gets."""
import functools

import numpy as np
import torch

import ppo_update_reference as R
from ppo_update_reference import (APPLIED, GRAD_ATOL, GRAD_RTOL, MET_ABS, MET_REL, PARAM_ATOL, ROBUST, SATURATED, SHAPES, Call, allowance,  # noqa: F401
                                  n_param, saturated_allowance, slice_bounds, worst, worst_by_slice)
from ppo_car_amd import Agent
from ppo_car_amd.imitation import bc_loss

VF, EC, LR = R.VF, R.EC, R.LR
# the norm clip: acting / idle.  The float64 gradient norms of the APPLIED cases' four steps are 0.32 .. 2.6 (the host test prints
# them): 0.05 is below every one of them by a factor of six and more
BC_MAX_NORM, BC_IDLE_NORM = 0.05, 1e9
ONE_ACTION = [s for s in SHAPES if s[2] == 1]                     # (2, 1, 1), (33, 40, 1)
EDGE_SHAPES = [(9, 39, 9), (65, 25, 2)]                           # the label-edge table: a compiled and a generic shape, B mod 8 = 1
IGNORE_SHAPES = [(7, 23, 9), (257, 39, 9), (1023, 40, 15), (65, 25, 2)]      # every kind of "no label"; no unlabelled sample at all
SINGLE_LABEL = [(9, 39, 9), (1023, 40, 15)]                       # one labelled sample in the whole minibatch
SHARED = [(3, 18, 9), (257, 39, 9), (1023, 40, 15), (65, 25, 2), (9, 1, 15)]      # the halves shared with pc_ppo_minibatch
LEARNER_B = [2, 9, 257, 1023]
# the agreeing-labels case: a compiled and a generic shape at scale 4000 and at 24000, where (8, 23, 9)'s ce is 7e-5 and its logits
# reach 160.  (The larger SATURATED shapes are no cases here: with agreeing labels torch's own float32 is 0.9 .. 1.5 x the standard
# gradient allowance at (1023, 40, 15) and (257, 39, 9) at scale 4000 and 7 x at 16000 -- 1 - p cancels -- so that bar would not be
# the kernel's to keep; at these two shapes it stays below 0.2 of it at both scales.)
AGREE_SHAPES = [(8, 23, 9), (65, 25, 2)]
AGREE_SCALES = (4000.0, 24000.0)
# The case table: the seed of a shape's draws (default 3000 + B) where the default breaks an input condition of
# tests/test_bc_update_f64_host.py
SEEDS = {(2, 23, 9): 2,         # 3002: the last sample's label A - 1 is its row's argmax (seed 1 likewise)
         (9, 1, 15): 1,         # 3009: the last sample dropped moves the critic's slices by 8 x the allowance only
         (65, 25, 2): 1}        # 3065: at scale 4000 the first unlabelled sample taken as label 0 moves 0.01 x the allowance (p_0 = 1 there)
# (shape, scale, steps, max_norm, agree) of every case tests/test_bc_update_f64_gpu.py runs against float64;
# tests/test_bc_update_f64_host.py holds each to the input conditions
ONE_STEP = [(s, scale, 1, BC_MAX_NORM, False) for scale in (1.0, 40.0) for s in SHAPES]
SATURATED_CASES = [(s, 4000.0, 1, BC_MAX_NORM, False) for s in SATURATED]
AGREEING = [(s, scale, 1, BC_MAX_NORM, True) for scale in AGREE_SCALES for s in AGREE_SHAPES]
MULTI = [(s, 1.0, 4, mn, False) for s in APPLIED for mn in (BC_MAX_NORM, BC_IDLE_NORM)]
LEARNER_NORM, LEARNER_SEED = 0.5, 3                               # BCLearner's default max_grad_norm; its seed in the test
LAST_ROW, UNLABELLED_ROW = 4, 5


def ids(cases):
    return [f"B{s[0]}-D{s[1]}-A{s[2]}-x{scale:g}-n{steps}-norm{mn:g}" + ("-agree" if agree else "") for s, scale, steps, mn, agree in cases]


def _agent_as(c, dtype):
    return R._agent_as(c, dtype)


def logits64(c, rows=None):
    """the float64 logits of the case's agent on (rows of) its pool"""
    with torch.no_grad():
        return _agent_as(c, torch.float64).actor(c["obs"].double() if rows is None else c["obs"][rows].double())


@functools.lru_cache(maxsize=None)
def inputs(B, D, A, scale=1.0, steps=1, agree=False):
    """The inputs of one case (float32 CPU tensors; read-only, shared): `steps` minibatches over one pool."""
    seed = SEEDS.get((B, D, A), 3000 + B)
    torch.manual_seed(seed)
    agent = Agent(D, A)
    with torch.no_grad():
        agent.actor[2].weight *= scale
        agent.actor[2].bias *= scale
    g = torch.Generator().manual_seed(seed)
    pool = B + 7
    obs = torch.rand(pool, D, generator=g) * 2.6 - 1.0
    label = torch.randint(-1, A, (pool,), generator=g).float()
    target = torch.randn(pool, generator=g)
    idx = [torch.randint(0, pool, (B,), generator=g).contiguous() for _ in range(steps)]
    c = dict(B=B, D=D, A=A, scale=scale, pool=pool, agent=agent, p0=R.flat(agent), obs=obs, label=label, target=target, idx=idx, agree=agree)
    best = logits64(c).argmax(-1)
    first = idx[0]
    if B >= 4:
        first[:4] = torch.tensor([0, pool - 1, 2, 2])
        label[0], label[pool - 1], label[2] = -1.0, A - 1.0, 0.0
    else:
        first[:2] = torch.tensor([0, pool - 1])
        label[0], label[pool - 1] = -1.0, A - 1.0
    if B % 8 != 0 and B >= 3:
        first[B - 1] = LAST_ROW
        label[LAST_ROW] = float((int(best[LAST_ROW]) + 1) % A)
        if B % 8 >= 2 and B >= 7:
            first[B - 2] = UNLABELLED_ROW
            label[UNLABELLED_ROW] = -1.0
    if agree:
        label.copy_(best.float())
    return c


def run_steps(c, max_norm=BC_MAX_NORM, dtype=torch.float64, vf=VF, ec=EC, targets=True):
    """bc_loss -> backward -> clip_grad_norm_ -> Adam over the case's minibatches in `dtype` on the CPU.  One dict per step, numpy
    float64: grad (raw), grad_clipped, norm, metrics (ce, vl, ent, total: the kernel's order), param / exp_avg / exp_avg_sq after the
    step."""
    a = _agent_as(c, dtype)
    opt = torch.optim.Adam(a.parameters(), lr=LR, eps=1e-5)
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).double().numpy().copy()
    out = []
    for ix in c["idx"]:
        obs, label, target = (c[k][ix].to(dtype) for k in ("obs", "label", "target"))
        for p in a.parameters():      # (zeros, not None: without targets the critic's gradient is 0 and Adam still visits it)
            p.grad = torch.zeros_like(p)
        total, ce, vl, ent = bc_loss(a, obs, label, target if targets else None, vf, ec)
        total.backward()
        raw = cat([p.grad for p in a.parameters()])
        norm = float(torch.nn.utils.clip_grad_norm_(a.parameters(), max_norm))
        clipped = cat([p.grad for p in a.parameters()])
        opt.step()
        params = list(a.parameters())
        out.append(dict(grad=raw, grad_clipped=clipped, norm=norm, metrics=np.array([float(t.detach()) for t in (ce, vl, ent, total)]),
                        param=cat(params), exp_avg=cat([opt.state[p]["exp_avg"] for p in params]),
                        exp_avg_sq=cat([opt.state[p]["exp_avg_sq"] for p in params])))
    return out


@functools.lru_cache(maxsize=None)
def case(B, D, A, scale=1.0, steps=1, max_norm=BC_MAX_NORM, agree=False):
    """The inputs of a case with its float64 reference under `ref` (one entry per step); computed once, shared, read-only."""
    c = dict(inputs(B, D, A, scale, steps, agree))
    c["max_norm"] = max_norm
    c["ref"] = run_steps(c, max_norm)
    return c


@functools.lru_cache(maxsize=None)
def restated32(B, D, A, scale=1.0, steps=1, max_norm=BC_MAX_NORM, agree=False):
    """the same steps in float32 torch on the CPU"""
    return run_steps(inputs(B, D, A, scale, steps, agree), max_norm, torch.float32)


def first_labels(c):
    """the first minibatch's labels, float32 [B]"""
    return c["label"][c["idx"][0]]


def is_labelled(lab, A):
    return (lab >= 0) & (lab < A)


def gradient_of(c, weight=None, labelled_divisor=False, label=None, dtype=torch.float64, vf=VF, ec=EC):
    """The first minibatch's loss written out per sample (bc_loss's operations), so that single samples can be tampered with: the flat
    float64 gradient of  sum_i weight_i labelled_i (ce_i - ec ent_i) / div + vf sum_i weight_i vl_i / B.
    weight: per-sample weights (default ones; a 0 drops the sample, the divisors stay).  labelled_divisor: div = the number of labelled
    samples instead of B (the value term keeps B).  label: the B labels to use instead of the case's.  With none of them this is
    bc_loss's gradient (the host test holds the two to each other)."""
    a = _agent_as(c, dtype)
    ix = c["idx"][0]
    obs, target = c["obs"][ix].to(dtype), c["target"][ix].to(dtype)
    lab = (first_labels(c) if label is None else torch.as_tensor(label)).to(dtype)
    B, A = c["B"], c["A"]
    w = torch.ones(B, dtype=dtype) if weight is None else torch.as_tensor(weight, dtype=dtype)
    logp = torch.log_softmax(a.actor(obs), -1)
    on = is_labelled(lab, A)
    act = torch.where(on, lab, torch.zeros_like(lab)).long()
    ce = -logp.gather(1, act.view(-1, 1)).view(-1)
    ent = -(logp.exp() * logp).sum(-1)
    val = 0.5 * (a.critic(obs).view(-1) - target) ** 2
    div = float(on.sum()) if labelled_divisor else float(B)
    ((w * on.to(dtype) * (ce - ec * ent)).sum() / div + vf * (w * val).sum() / B).backward()
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in a.parameters()]).double().numpy()


def wrong_gradients(c):
    """The four wrong answers of the sensitivity condition, in the issue's order: (a) the last sample dropped, the divisor still B (what
    a partly dead workgroup would lose); (b) the ce and ent sums divided by the number of labelled samples; (c) the first unlabelled
    sample taken as label 0; (d) the first labelled sample's label moved to (label + 1) mod A."""
    B, A = c["B"], c["A"]
    lab = first_labels(c)
    on = is_labelled(lab, A)
    assert bool(on.any()) and not bool(on.all()), "the first minibatch needs a labelled and an unlabelled sample"
    w = np.ones(B)
    w[B - 1] = 0.0
    as_zero, moved = lab.clone(), lab.clone()
    as_zero[int(torch.nonzero(~on)[0])] = 0.0
    j = int(torch.nonzero(on)[0])
    moved[j] = float((int(lab[j]) + 1) % A)
    return dict(a=gradient_of(c, weight=w), b=gradient_of(c, labelled_divisor=True), c=gradient_of(c, label=as_zero),
                d=gradient_of(c, label=moved))


def actor_end(D, A):
    """the flat offset at which the critic's slices begin"""
    return slice_bounds(D, A)[4][1]


def metric_worst(m, mref):
    return float((np.abs(np.asarray(m, np.float64) - mref) / (MET_ABS + MET_REL * np.abs(mref))).max())


def label_edges(A):
    """[(name, the label as a float32 value, the whole label bc_loss makes of it or -1 for none)]: the edges of
    labelled = (0 <= label < A) and of the truncation (int)label."""
    f = np.float32
    e = [("-0.0", f(-0.0), 0), ("0.999", f(0.999), 0), ("A-1+0.5", f(A - 1 + 0.5), A - 1),
         ("nextafter(A,0)", np.nextafter(f(A), f(0.0)), A - 1)]
    if A > 2:
        e.append(("2.5", f(2.5), 2))
    e += [("A", f(A), -1), ("nextafter(0,-1)", np.nextafter(f(0.0), f(-1.0)), -1), ("-0.5", f(-0.5), -1), ("nan", f("nan"), -1),
          ("+inf", f("inf"), -1), ("-inf", f("-inf"), -1), ("3e38", f(3e38), -1), ("-3e38", f(-3e38), -1), ("2**31", f(2.0 ** 31), -1),
          ("2**32+1", f(2.0 ** 32 + 1.0), -1)]
    return [(name, f(v), int(whole)) for name, v, whole in e]


LABEL_EDGES = {A: label_edges(A) for A in sorted({s[2] for s in EDGE_SHAPES})}


def with_label(c, sample, value):
    """the case's pool labels with the row of first-minibatch sample `sample` overwritten by `value` (a copy, float32); every sample
    of that row carries the value"""
    lab = c["label"].clone()
    lab[int(c["idx"][0][sample])] = float(value)
    return lab


def edge_samples(c):
    """(a sample of the first, full group; the last live sample, in the partly dead group): where the label-edge values are placed"""
    assert c["B"] % 8 != 0 and c["B"] > 8
    ix = c["idx"][0].tolist()
    return next(j for j in range(4, 8) if ix[j] != ix[-1]), c["B"] - 1


def all_labelled(c):
    """the first minibatch's indices with every unlabelled sample replaced by the first labelled sample's row: the same B, no sample
    ignored"""
    on = is_labelled(first_labels(c), c["A"])
    ix = c["idx"][0].clone()
    ix[~on] = ix[int(torch.nonzero(on)[0])]
    return ix


def single_label(c):
    """(idx, label, the sample): the first minibatch with ONE labelled sample, the last one -- every other label of the pool is -1 and
    no other sample shares its row (LAST_ROW elsewhere in the minibatch becomes row 6)"""
    B = c["B"]
    ix = c["idx"][0].clone()
    assert int(ix[B - 1]) == LAST_ROW
    ix[:B - 1][ix[:B - 1] == LAST_ROW] = 6
    lab = torch.full_like(c["label"], -1.0)
    lab[LAST_ROW] = c["label"][LAST_ROW]
    return ix, lab, B - 1


def ce_emulated(c, order):
    """The ce metric of the first minibatch in float32 on the CPU from the float32 logits, the log-softmax in one of two operation
    orders: "kernel": l_a - (max + log(sum exp(l - max))) (K27's lse form); "torch": (l_a - max) - log(sum).  The sum over the samples
    is taken in float64: the question is the per-sample rounding."""
    a = _agent_as(c, torch.float32)
    ix = c["idx"][0]
    with torch.no_grad():
        l = a.actor(c["obs"][ix])
    lab = first_labels(c)
    on = is_labelled(lab, c["A"])
    la = l.gather(1, torch.where(on, lab, torch.zeros_like(lab)).long().view(-1, 1)).view(-1)
    mx = l.max(-1).values
    s = torch.exp(l - mx.view(-1, 1)).sum(-1)
    lp = la - (mx + torch.log(s)) if order == "kernel" else (la - mx) - torch.log(s)
    return float((-lp.double() * on.double()).sum() / c["B"])


@functools.lru_cache(maxsize=None)
def learner_case(B, D=23, A=9):
    """BCLearner(batch_size = B, vf_coef = VF, ent_coef = EC, seed = LEARNER_SEED).fit on M = 3 B + 5 rows, one epoch: M // B steps --
    three, the tail of five rows cut (B = 2: five steps and a tail of one).  idx is what draw_indices draws (a permutation from
    np.random.default_rng(seed), cut to full minibatches), `ref` the float64 trajectory on it."""
    M = 3 * B + 5
    n = M // B
    base = inputs(B, D, A)
    g = torch.Generator().manual_seed(7000 + B)
    obs = torch.rand(M, D, generator=g) * 2.6 - 1.0
    label = torch.randint(-1, A, (M,), generator=g).float()
    target = torch.randn(M, generator=g)
    perm = np.random.default_rng(LEARNER_SEED).permutation(M)[:n * B].astype(np.int64)
    idx = [torch.from_numpy(perm[m * B:(m + 1) * B].copy()) for m in range(n)]
    c = dict(B=B, D=D, A=A, scale=1.0, pool=M, agent=base["agent"], p0=base["p0"], obs=obs, label=label, target=target, idx=idx, agree=False,
             max_norm=LEARNER_NORM)
    c["ref"] = run_steps(c, LEARNER_NORM)
    c["ref32"] = run_steps(c, LEARNER_NORM, torch.float32)
    return c
