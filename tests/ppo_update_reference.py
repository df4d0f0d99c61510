"""The small-minibatch PPO step (pc_ppo_minibatch: K10 + K11 + K12) restated: the inputs of every edge-shape case, the float64 reference
(ppo.ppo_loss on a .double() copy of the agent, clip_grad_norm_, torch.optim.Adam(lr 3e-4, eps 1e-5)) over consecutive minibatches, the
same steps in float32 torch on the CPU (the yardstick of the input conditions; never the code under test), the two deliberately wrong
float64 gradients of the sensitivity condition, and `Call`, one entry-point call's device state.  The large-minibatch step
(pc_ppo_adv_stats + pc_ppo_minibatch_large: KLs + K10L + K11 + K12) takes the same inputs and reference at 1024 < B: its case tables
(LARGE_*), a third wrong gradient for its walk, `adv_stats` and `Call.large`.

Inputs of a case: a pool of B + 7 rows, Agent(D, A) at its seeded initial weights with actor[2] multiplied by `scale`, obs uniform in
[-1, 1.6], old log-probs = the agent's own + 0.3 N(0, 1), adv = 3 + 0.5 N(0, 1), ret = N(0, 1), indices drawn WITH replacement, the
first four forced to (0, pool - 1, 2, 2) from B = 4 on: the first row, the last row, a duplicate."""
import functools

import numpy as np
import torch

from ppo_car_amd import Agent, _capi
from ppo_car_amd.ppo import ppo_loss

lib = _capi.lib
CLIP, VF, EC, MAX_NORM, LR = 0.2, 0.5, 0.01, 0.5, 3e-4
GRAD_RTOL, GRAD_ATOL = 2e-4, 2e-7            # the project's bars (tests/test_ppo_golden.py): the gradient,
MET_REL, MET_ABS = 1e-5, 1e-6                # the metric sums,
PARAM_ATOL = 3e-6                            # the parameters after an applied step
SLICES = ("actor.0.weight", "actor.0.bias", "actor.2.weight", "actor.2.bias", "critic.0.weight", "critic.0.bias", "critic.2.weight",
          "critic.2.bias")

COMPILED = [(2, 23, 9), (3, 18, 9), (7, 23, 9), (8, 23, 9), (9, 39, 9), (255, 18, 9), (256, 23, 9), (257, 39, 9), (1023, 23, 9), (1024, 39, 9)]
GENERIC = [(2, 1, 1), (9, 1, 15), (64, 24, 15), (65, 25, 2), (1023, 40, 15), (33, 40, 1), (513, 7, 3)]
SHAPES = COMPILED + GENERIC
SATURATED = [(8, 23, 9), (257, 39, 9), (65, 25, 2), (1023, 40, 15)]          # at scale 4000
APPLIED = [(9, 39, 9), (256, 23, 9), (1023, 40, 15), (65, 25, 2)]            # four applied steps, max_norm 0.5 and 1e9
ROBUST = [(9, 39, 9), (1023, 23, 9), (65, 25, 2)]
FORMS = [(B, D, A) for B in (2, 9, 257, 1023) for D, A in ((23, 9), (39, 9), (25, 2), (24, 15))]
# The case table: the seed of a shape's draws (default 1000 + B) where the default breaks an input condition of
# tests/test_ppo_update_f64_host.py, and the hand-made (ratio, adv) rows of the small cases: sample j of the first minibatch gets
# old_lp = own - log(ratio) and that advantage, so that B = 7, 8, 9 together hold a ratio below, inside and above the clip range with
# a normalised advantage of either sign.
SEEDS = {(2, 23, 9): 2,         # 1002: no sample outside the clip range, and torch's float32 misses the metric sums' allowance (1.9 x)
         (2, 1, 1): 1,          # 1002: no sample outside the clip range
         (256, 23, 9): 19,      # 1256: gradient norms of 0.39 .. 0.41, the norm clip at 0.5 never acts
         (1023, 40, 15): 1,     # 2023: norms of 0.24 .. 0.38
         (65, 25, 2): 2,        # 1065: a norm of 0.495 at the third step
         (1024, 40, 16): 4,     # 2024: a norm of 0.37 at the fourth step (seeds 1, 3: norms of 0.22 .. 0.45; seed 2: a ratio 1.5e-6 from an
                                #       edge in the idle-clip steps).  A = 16: tests/test_update_tail_f64_gpu.py, the learner's fused path
         # the large cases (conditions of tests/test_large_minibatch_f64_host.py)
         (2049, 39, 9): 2,      # 3049: at scale 4000 an inverted clip decision is 13 x the allowance; a ratio 8.2e-6 from an edge in the
                                #       four idle-clip steps (seed 1: a flip that moves nothing at scale 4000)
         (4097, 23, 9): 1,      # 5097: a ratio 4.5e-6 from a clip edge in the four idle-clip steps
         (6151, 18, 9): 1,      # 7151: at scale 40 torch's float32 misses the gradient allowance (6.2 x); a ratio 1.7e-5 from an edge
         (1026, 1, 15): 5,      # 2026: a gradient norm of 0.047, the norm clip at 0.05 idle in the first step (seeds 1 .. 4 likewise, or
                                #       a ratio 2e-6 from an edge)
         (2054, 25, 2): 3,      # 3054: at scale 4000 an inverted clip decision is 11 x the allowance (seed 1: sample 2048 dropped 8 x;
                                #       seed 2: torch's float32 26 x the gradient allowance at scale 40)
         (4097, 40, 15): 3}     # 5097: a ratio 4.2e-6 from a clip edge (seed 1: the last sample dropped 13 x at scale 4000; seed 2: 1e-6)
HAND = {(B, D, A): [((0.6, 1.0, 1.45)[j % 3], 3.0 + (0.9 if (j // 3) % 2 == 0 else -0.9)) for j in range(B)]
        for B, D, A in ((7, 23, 9), (8, 23, 9), (9, 39, 9))}
ADV_RAISED = {}         # (B, D, A, scale) -> {sample of the first minibatch: its advantage}, where the sensitivity condition needed it

# ---- the large-minibatch step (pc_ppo_adv_stats + pc_ppo_minibatch_large: KLs + K10L + K11 + K12), the same inputs at 1024 < B.
# B is laid out for a K10L grid of 256 workgroups (the compute units of an MI355X): 129 groups of eight samples (every workgroup one
# group), 257 (workgroup 0 a second), 513 (a third: the first whose indices were requested two groups ahead), 769 (a fourth), with
# every residue of B mod 8 in the last group.  (D, A) as above: the compiled shapes, and the generic forms at the ends of their
# ranges -- 24-wide at D = 1, 7, 24; rolled 40-wide at D = 25, 40; A = 1, 2, 3, 8, 15, which cut layer 2 into 4, 4, 4, 3, 2 parts.
LARGE_COMPILED = [(1025, 23, 9), (1031, 18, 9), (2049, 39, 9), (2056, 23, 9), (4097, 23, 9), (4104, 39, 9), (6151, 18, 9)]
LARGE_GENERIC = [(1025, 1, 1), (1026, 1, 15), (2049, 24, 15), (2054, 25, 2), (4097, 40, 15), (1029, 40, 1), (4099, 7, 3), (2052, 24, 8)]
LARGE_SHAPES = LARGE_COMPILED + LARGE_GENERIC
LARGE_SATURATED = [(1025, 23, 9), (2049, 39, 9), (4097, 40, 15), (2054, 25, 2)]       # at scale 4000
LARGE_APPLIED = [(2049, 39, 9), (4097, 23, 9), (2054, 25, 2), (1026, 1, 15)]          # four applied steps, max_norm 0.05 and 1e9
LARGE_ROBUST = [(2049, 39, 9), (6151, 18, 9), (4097, 40, 15)]
LARGE_CONST_ADV = [(2056, 23, 9), (4097, 23, 9)]                                      # every advantage 0.5
LARGE_MAX_NORM, LARGE_IDLE_NORM = 0.05, 1e9      # tests/test_large_minibatch_gpu.py's: at these B the gradient norms are below 0.5
WALK_SAMPLE = 8 * 256                            # the first sample of workgroup 0's second group on 256 compute units
# (shape, scale, steps, max_norm) of every case tests/test_large_minibatch_f64_gpu.py runs against float64;
# tests/test_large_minibatch_f64_host.py holds each to the input conditions
LARGE_ONE_STEP = ([(s, scale, 1, LARGE_MAX_NORM) for scale in (1.0, 40.0) for s in LARGE_SHAPES]
                  + [(s, 4000.0, 1, LARGE_MAX_NORM) for s in LARGE_SATURATED])
LARGE_MULTI = [(s, 1.0, 4, mn) for s in LARGE_APPLIED for mn in (LARGE_MAX_NORM, LARGE_IDLE_NORM)]


def n_param(D, A):
    return 2 * (256 * D + 256) + A * 256 + A + 256 + 1


def slice_bounds(D, A):
    """[(name, start, end)] of the eight parameter slices in the flat buffers (torch's module.parameters() order)"""
    sizes = (256 * D, 256, A * 256, A, 256 * D, 256, 256, 1)
    ends = np.cumsum(sizes)
    return [(k, int(e - s), int(e)) for k, s, e in zip(SLICES, sizes, ends)]


def flat(agent, dtype=torch.float32):
    return torch.cat([p.detach().reshape(-1) for p in agent.parameters()]).to(dtype).contiguous()


@functools.lru_cache(maxsize=None)
def inputs(B, D, A, scale=1.0, steps=1, const_adv=None):
    """The inputs of one case (float32 CPU tensors; read-only, shared): `steps` minibatches over one pool."""
    seed = SEEDS.get((B, D, A), 1000 + B)
    torch.manual_seed(seed)
    agent = Agent(D, A)
    with torch.no_grad():
        agent.actor[2].weight *= scale
        agent.actor[2].bias *= scale
    g = torch.Generator().manual_seed(seed)
    pool = B + 7
    obs = torch.rand(pool, D, generator=g) * 2.6 - 1.0
    act = torch.randint(0, A, (pool,), generator=g).float()
    with torch.no_grad():
        own = torch.log_softmax(agent.actor(obs), -1).gather(1, act.long().view(-1, 1)).view(-1)
    old_lp = own + 0.3 * torch.randn(pool, generator=g)
    adv = 3.0 + 0.5 * torch.randn(pool, generator=g)
    ret = torch.randn(pool, generator=g)
    idx = []
    for _ in range(steps):
        ix = torch.randint(0, pool, (B,), generator=g)
        if B >= 4:
            ix[:4] = torch.tensor([0, pool - 1, 2, 2])
        idx.append(ix.contiguous())
    for j, (ratio, a) in enumerate(HAND.get((B, D, A), [])):
        old_lp[idx[0][j]] = own[idx[0][j]] - float(np.log(ratio))
        adv[idx[0][j]] = a
    for j, a in ADV_RAISED.get((B, D, A, scale), {}).items():
        adv[idx[0][j]] = a
    if const_adv is not None:
        adv.fill_(const_adv)
    return dict(B=B, D=D, A=A, scale=scale, pool=pool, agent=agent, p0=flat(agent), obs=obs, act=act, old_lp=old_lp, adv=adv, ret=ret, idx=idx)


def _agent_as(c, dtype):
    a = Agent(c["D"], c["A"]).to(dtype)
    a.load_state_dict({k: v.to(dtype) for k, v in c["agent"].state_dict().items()})
    return a


def run_steps(c, max_norm=MAX_NORM, dtype=torch.float64, ec=EC):
    """ppo_loss -> backward -> clip_grad_norm_ -> Adam over the case's minibatches in `dtype` on the CPU.  One dict per step, numpy
    float64: grad (raw), grad_clipped, norm, metrics (policy loss, value loss, entropy, total), param / exp_avg / exp_avg_sq after the
    step, and ratio / adv_n, the step's per-sample ratios and normalised advantages at the parameters it started from."""
    a = _agent_as(c, dtype)
    opt = torch.optim.Adam(a.parameters(), lr=LR, eps=1e-5)
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).double().numpy().copy()
    out = []
    for ix in c["idx"]:
        obs, act, old_lp, adv, ret = (c[k][ix].to(dtype) for k in ("obs", "act", "old_lp", "adv", "ret"))
        opt.zero_grad()
        loss, pl, vl, en = ppo_loss(a, obs, act, old_lp, adv, ret, CLIP, VF, ec)
        loss.backward()
        with torch.no_grad():
            new_lp = torch.log_softmax(a.actor(obs), -1).gather(1, act.long().view(-1, 1)).view(-1)
            ratio = torch.exp(new_lp - old_lp).double().numpy()
            adv_n = ((adv - adv.mean()) / adv.std().clamp_min(1e-5)).double().numpy()
        raw = cat([p.grad for p in a.parameters()])
        norm = float(torch.nn.utils.clip_grad_norm_(a.parameters(), max_norm))
        clipped = cat([p.grad for p in a.parameters()])
        opt.step()
        params = list(a.parameters())
        out.append(dict(grad=raw, grad_clipped=clipped, norm=norm, metrics=np.array([float(t.detach()) for t in (pl, vl, en, loss)]),
                        param=cat(params), exp_avg=cat([opt.state[p]["exp_avg"] for p in params]),
                        exp_avg_sq=cat([opt.state[p]["exp_avg_sq"] for p in params]), ratio=ratio, adv_n=adv_n))
    return out


@functools.lru_cache(maxsize=None)
def case(B, D, A, scale=1.0, steps=1, max_norm=MAX_NORM, const_adv=None):
    """The inputs of a case with its float64 reference under `ref` (one entry per step); computed once, shared, read-only."""
    c = dict(inputs(B, D, A, scale, steps, const_adv))
    c["max_norm"] = max_norm
    c["ref"] = run_steps(c, max_norm)
    return c


@functools.lru_cache(maxsize=None)
def restated32(B, D, A, scale=1.0, steps=1, max_norm=MAX_NORM):
    """the same steps in float32 torch on the CPU"""
    return run_steps(inputs(B, D, A, scale, steps), max_norm, torch.float32)


def gradient_of(c, weight=None, flip=None, dtype=torch.float64, entropy_only=False):
    """The first minibatch's loss written out per sample (ppo_loss's operations), so that single samples can be tampered with: the flat
    float64 gradient of  (sum_i weight_i (policy_i + VF value_i - EC entropy_i)) / B  with the advantage statistics of all B samples.
    weight: per-sample weights (default ones; a 0 drops the sample, the divisor stays B).  flip: a sample whose clip decision is
    inverted -- where torch.max took the unclipped term it takes the clipped one and the other way round.  entropy_only: the entropy
    term alone.  With neither weight nor flip this is ppo_loss's gradient (the host test holds the two to each other)."""
    a = _agent_as(c, dtype)
    ix = c["idx"][0]
    obs, act, old_lp, adv, ret = (c[k][ix].to(dtype) for k in ("obs", "act", "old_lp", "adv", "ret"))
    B = c["B"]
    w = torch.ones(B, dtype=dtype) if weight is None else torch.as_tensor(weight, dtype=dtype)
    logp = torch.log_softmax(a.actor(obs), -1)
    ent = -(logp.exp() * logp).sum(-1)
    new_lp = logp.gather(1, act.long().view(-1, 1)).view(-1)
    ratio = torch.exp(new_lp - old_lp)
    an = (adv - adv.mean()) / adv.std().clamp_min(1e-5)
    pl1, pl2 = -an * ratio, -an * torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP)
    first = pl1 >= pl2
    if flip is not None:
        first = first.clone()
        first[flip] = ~first[flip]
    pol = torch.where(first, pl1, pl2)
    val = 0.5 * (a.critic(obs).view(-1) - ret) ** 2
    per_sample = -EC * ent if entropy_only else pol + VF * val - EC * ent
    ((w * per_sample).sum() / B).backward()
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in a.parameters()]).double().numpy()


def allowance(gref):
    """the project's gradient allowance per element"""
    return GRAD_ATOL + GRAD_RTOL * np.abs(gref)


def worst(g, gref, allow=None):
    """worst error / allowance over the elements"""
    return float((np.abs(g - gref) / (allowance(gref) if allow is None else allow)).max())


def worst_by_slice(g, gref, D, A, allow=None):
    al = allowance(gref) if allow is None else allow * np.ones_like(gref)
    return {k: float((np.abs(g[s:e] - gref[s:e]) / al[s:e]).max()) for k, s, e in slice_bounds(D, A)}


def saturated_allowance(g32, g64):
    """the gradient allowance at scale 4000: 2e-4 |g64| + 4 max_i |g32_i - g64_i|"""
    return GRAD_RTOL * np.abs(g64) + 4.0 * float(np.abs(g32 - g64).max())


def out_of_range_sample(r):
    """the first sample of a step whose ratio lies outside the clip range (None: there is none)"""
    out = np.nonzero((r["ratio"] < 1.0 - CLIP) | (r["ratio"] > 1.0 + CLIP))[0]
    return int(out[0]) if len(out) else None


def wrong_gradients(c):
    """The two wrong answers of the sensitivity condition: the last sample dropped (the one a partly dead workgroup would lose), and
    the clip decision of the first out-of-range sample inverted."""
    B = c["B"]
    w = np.ones(B)
    w[B - 1] = 0.0
    j = out_of_range_sample(c["ref"][0])
    assert j is not None, "the case holds no sample outside the clip range: change its seed"
    return gradient_of(c, weight=w), gradient_of(c, flip=j)


def walk_wrong_gradient(c):
    """The wrong answer of the large step's walk (B > 2048): sample 8 * 256 dropped, the first sample of workgroup 0's second group --
    what a workgroup would lose whose second group's rows never arrived."""
    assert c["B"] > WALK_SAMPLE
    w = np.ones(c["B"])
    w[WALK_SAMPLE] = 0.0
    return gradient_of(c, weight=w)


def adv_stats(idx2d, B, adv, idx_ld=None):
    """pc_ppo_adv_stats on the index rows idx2d [n_mb][>= B] (device; row m starts idx_ld = idx2d.stride(0) elements after row m - 1
    and its first B entries count) -> [n_mb][2] float32 (device).  Result and workspace are pre-filled with NaN."""
    n_mb = idx2d.shape[0]
    idx_ld = idx2d.stride(0) if idx_ld is None else idx_ld
    assert idx2d.stride(1) == 1 and idx_ld >= B
    stats = torch.full((n_mb, 2), float("nan"), device="cuda")
    n_ws = lib.pc_ppo_adv_stats_workspace_doubles(n_mb, B)
    assert n_ws > 0
    ws = torch.full((n_ws,), float("nan"), device="cuda", dtype=torch.float64)
    _capi.check(lib.pc_ppo_adv_stats(0, idx2d.data_ptr(), idx_ld, n_mb, B, adv.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "pc_ppo_adv_stats")
    torch.cuda.synchronize()
    return stats


class Call:
    """One pc_bc_minibatch / pc_ppo_minibatch (plain, prepared, diagnostics, epoch) / pc_ppo_minibatch_large call's device state.  grad
    is pre-filled with 7.0; the workspace has pc_ppo_workspace_floats floats (the diagnostics forms: pc_ppo_diag_workspace_floats;
    large = True: pc_ppo_large_workspace_floats on device 0) and is pre-filled with ws_fill.  shift = n > 0: grad, the moments, step,
    lr and metrics each start n floats into a larger allocation."""

    def __init__(self, param, B, D, A, max_norm=MAX_NORM, ec=EC, ws_fill=0.0, shift=0, diag=False, large=False):
        n = param.numel()
        assert n == n_param(D, A)
        self.B, self.D, self.A, self.max_norm, self.ec = B, D, A, max_norm, ec

        def buf(k, fill):
            whole = torch.full((k + 2 * shift,), -3.0, device="cuda")
            part = whole[shift:shift + k]
            part.fill_(fill)
            return part

        self.param = param.clone()
        self.grad = buf(n, 7.0)
        self.m, self.v = buf(n, 0.0), buf(n, 0.0)
        self.step = buf(1, 0.0)
        self.lr = buf(1, LR)
        self.metrics = buf(4, 0.0)
        assert not (diag and large)
        if large:
            n_ws = lib.pc_ppo_large_workspace_floats(0, B, D, 256, A)
        else:
            n_ws = (lib.pc_ppo_diag_workspace_floats if diag else lib.pc_ppo_workspace_floats)(B, D, 256, A)
        assert n_ws > 0
        self.ws = torch.full((n_ws,), ws_fill, device="cuda")
        self.diag = torch.zeros(8, device="cuda") if diag else None

    def _state(self):
        return (self.param.data_ptr(), self.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.step.data_ptr(), self.lr.data_ptr())

    def _coef(self):
        return (CLIP, VF, self.ec, self.max_norm, 0.9, 0.999, 1e-5)

    def _done(self, rc, name):
        _capi.check(rc, name)
        torch.cuda.synchronize()
        return self

    def bc(self, idx, obs, label, target, vf=VF, ec=EC, apply=0):
        return self._done(lib.pc_bc_minibatch(0, idx.data_ptr(), self.B, self.D, 256, self.A, obs.data_ptr(), label.data_ptr(),
                                              target.data_ptr() if target is not None else None, *self._state(), vf, ec, self.max_norm, 0.9, 0.999,
                                              1e-5, self.metrics.data_ptr(), self.ws.data_ptr(), apply, torch.cuda.current_stream().cuda_stream),
                          "pc_bc_minibatch")

    def ppo(self, idx, obs, act, old_lp, adv, ret, apply=0):
        return self._done(lib.pc_ppo_minibatch(0, idx.data_ptr(), self.B, self.D, 256, self.A, obs.data_ptr(), act.data_ptr(), old_lp.data_ptr(),
                                               adv.data_ptr(), ret.data_ptr(), *self._state(), *self._coef(), self.metrics.data_ptr(),
                                               self.ws.data_ptr(), apply, torch.cuda.current_stream().cuda_stream), "pc_ppo_minibatch")

    def large(self, idx, obs, act, old_lp, adv, ret, stats, apply=0):
        """`stats`: this minibatch's (mean, std) pair from adv_stats (device)"""
        return self._done(lib.pc_ppo_minibatch_large(0, idx.data_ptr(), self.B, self.D, 256, self.A, obs.data_ptr(), act.data_ptr(),
                                                     old_lp.data_ptr(), adv.data_ptr(), ret.data_ptr(), stats.data_ptr(), *self._state(),
                                                     *self._coef(), self.metrics.data_ptr(), self.ws.data_ptr(), apply,
                                                     torch.cuda.current_stream().cuda_stream), "pc_ppo_minibatch_large")

    def ppo_diag(self, idx, obs, act, old_lp, adv, ret, apply=0, target_kl=0.0):
        return self._done(lib.pc_ppo_minibatch_diag(0, idx.data_ptr(), self.B, self.D, 256, self.A, obs.data_ptr(), act.data_ptr(),
                                                    old_lp.data_ptr(), adv.data_ptr(), ret.data_ptr(), *self._state(), *self._coef(),
                                                    self.metrics.data_ptr(), self.ws.data_ptr(), apply, self.diag.data_ptr(), target_kl,
                                                    torch.cuda.current_stream().cuda_stream), "pc_ppo_minibatch_diag")

    def prepared(self, block, apply=0):
        """`block`: one minibatch's part of a pc_ppo_prepare buffer"""
        return self._done(lib.pc_ppo_minibatch_prepared(0, block.data_ptr(), self.B, self.D, 256, self.A, *self._state(), *self._coef(),
                                                        self.metrics.data_ptr(), self.ws.data_ptr(), apply, torch.cuda.current_stream().cuda_stream),
                          "pc_ppo_minibatch_prepared")

    def epoch(self, prepared, n_mb):
        n_state = lib.pc_ppo_epoch_state_floats(self.D, 256, self.A)
        assert n_state > 0
        self.state2 = torch.full((n_state,), float("nan"), device="cuda")
        return self._done(lib.pc_ppo_epoch_prepared(0, prepared.data_ptr(), n_mb, self.B, self.D, 256, self.A, *self._state(), *self._coef(),
                                                    self.metrics.data_ptr(), self.ws.data_ptr(), self.state2.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), "pc_ppo_epoch_prepared")


def prepare(idx2d, B, D, obs, act, old_lp, adv, ret):
    """pc_ppo_prepare on idx2d [n_mb][B] (device): the buffer as [n_mb][pc_ppo_prepared_floats(B, D)]"""
    n_mb, pf = idx2d.shape[0], lib.pc_ppo_prepared_floats(B, D)
    assert pf > 0 and idx2d.is_contiguous()
    out = torch.full((n_mb, pf), float("nan"), device="cuda")
    _capi.check(lib.pc_ppo_prepare(0, idx2d.data_ptr(), idx2d.stride(0), n_mb, B, D, obs.data_ptr(), act.data_ptr(), old_lp.data_ptr(),
                                   adv.data_ptr(), ret.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream), "pc_ppo_prepare")
    torch.cuda.synchronize()
    return out
