"""The small-minibatch PPO step (pc_ppo_minibatch: K10 + K11 + K12) restated: the inputs of every edge-shape case, the float64 reference
(ppo.ppo_loss on a .double() copy of the agent, clip_grad_norm_, torch.optim.Adam(lr 3e-4, eps 1e-5)) over consecutive minibatches, the
same steps in float32 torch on the CPU (the yardstick of the input conditions; never the code under test), the two deliberately wrong
float64 gradients of the sensitivity condition, and `Call`, one entry-point call's device state.

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
         (65, 25, 2): 2}        # 1065: a norm of 0.495 at the third step
HAND = {(B, D, A): [((0.6, 1.0, 1.45)[j % 3], 3.0 + (0.9 if (j // 3) % 2 == 0 else -0.9)) for j in range(B)]
        for B, D, A in ((7, 23, 9), (8, 23, 9), (9, 39, 9))}
ADV_RAISED = {}         # (B, D, A, scale) -> {sample of the first minibatch: its advantage}, where the sensitivity condition needed it


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


class Call:
    """One pc_bc_minibatch / pc_ppo_minibatch (plain, prepared, diagnostics, epoch) call's device state.  grad is pre-filled with 7.0;
    the workspace has pc_ppo_workspace_floats floats (the diagnostics forms: pc_ppo_diag_workspace_floats) and is pre-filled with
    ws_fill.  shift = n > 0: grad, the moments, step, lr and metrics each start n floats into a larger allocation."""

    def __init__(self, param, B, D, A, max_norm=MAX_NORM, ec=EC, ws_fill=0.0, shift=0, diag=False):
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
