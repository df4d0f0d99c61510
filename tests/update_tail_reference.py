"""The update kernels outside pc_ppo_minibatch restated: K6 ppo_gather_kernel (pc_ppo_gather), K7 ppo_loss_kernel<16, false>
(pc_ppo_loss; pc_ppo_loss_diag), K8 clip_adam_kernel<false> (pc_clip_adam) -- the update of every agent off the hand-written menu --
and K12m clip_adam_mb_kernel (pc_clip_adam_advanced), the clip + Adam step of every multi-rank minibatch.  Here: the loss on given
network outputs through autograd (`loss_on_outputs`: float64 the reference, float32 on the CPU the yardstick of the input conditions,
never the code under test), clip + Adam over consecutive gradients (`clip_adam_steps`, likewise), the case tables with their seeds, the
wrong answers of the sensitivity conditions, and `Tail`, one call's device state between guard floats.  Constants, `allowance`, `worst`
and `saturated_allowance` are tests/ppo_update_reference.py's.

Loss inputs of a case (B, A, s): logits = s N(0, 1) (s = 30: probabilities near 1 and 1e-20), values and ret N(0, 1), act uniform with
act[0] = 0 and act[1] = A - 1, old_lp = the own log-prob + 0.3 N(0, 1), adv = 3 + 0.5 N(0, 1); from B = 63 on the first six samples get
hand-made (ratio, advantage) rows: a ratio below, inside and above the clip range with a normalised advantage of either sign.

Clip + Adam inputs of a case n: parameters 0.1 N(0, 1) (the size of the agent's initial weights), gradients of random sign and
magnitude uniform in [0.5, 1.5], scaled to a norm of 2 (1 + 0.1 t).  The magnitudes are kept within a factor of three because the
moments' bars are relative to the clipped gradient of the step they are checked after: exp_avg_sq inherits 0.999 of its value -- and of
the float32 rounding of that value, 6e-8 of up to 0.011 g_max^2 -- from the steps before, against an allowance of 4e-7 g^2 for this
step's g.  A normal draw has elements a thousand times below their predecessors and float32 arithmetic of any order misses the bar
there: float32 torch on the CPU, four steps from zero moments on N(0, 1) gradients of norm 2, is at 18 x .. 2500 x the exp_avg_sq bar
at n = 1024 and 23 050 (parameters 0.02, exp_avg 0.05), against 0.027 at these inputs (tests/test_update_tail_f64_host.py holds it to
half of every bar).  A bucket for
grad_scale = 1 / W holds W x the gradient (exact: W is a power of two), as the sum over W ranks would."""
import functools

import numpy as np
import torch

import ppo_update_reference as R
from ppo_car_amd import _capi
from ppo_update_reference import (CLIP, EC, GRAD_ATOL, GRAD_RTOL, LR, MAX_NORM, MET_ABS, MET_REL, PARAM_ATOL, VF, allowance,  # noqa: F401
                                  saturated_allowance, worst)

lib = _capi.lib
BETA1, BETA2, EPS = 0.9, 0.999, 1e-5

# ---- K7: (B, A).  B: the launch rounds to 64 threads and block_sum has 16 wave slots -- 2, 3 one partly dead wave; 63 / 64 / 65 around
# one wave; 255 / 257 around four; 1023 / 1024 the sixteenth wave partly dead and full.  A: 1, 2 and 15, 16 are the ends of the 16-wide
# template (A = 16 is reachable through K7 alone), 9 is CarEnv's.
LOSS_CASES = [(2, 1), (3, 9), (63, 2), (64, 16), (65, 9), (255, 15), (257, 16), (1023, 9), (1024, 16), (1024, 1)]
LOSS_SATURATED = [(3, 9), (65, 9), (257, 16), (1024, 16)]          # at s = 30
LOSS_CONST_ADV = [(64, 16), (1024, 16)]                            # every advantage 0.5
SAT = 30.0
# (B, A, s) -> seed (default 2000 + 17 B + A) where the default breaks an input condition of tests/test_update_tail_f64_host.py
LOSS_SEEDS = {(2, 1, 1.0): 1,          # 2035: advantages 0.04 apart, float32 torch misses the metric sums' allowance (6.7 x)
              (3, 9, 1.0): 1,          # 2060: float32 torch at 0.63 of the metric sums' allowance
              (1023, 9, 1.0): 1,       # 19400: float32 torch at 0.73 of the dlogits allowance
              (1024, 16, 1.0): 3,      # 19424: a ratio 8.3e-6 from a clip edge (seeds 1, 2: float32 torch at 0.79, 1.18 of the dlogits allowance)
              (1024, 16, SAT): 1}      # 19424: a ratio 8.4e-6 from a clip edge
HAND_ROWS = [((0.6, 1.0, 1.45)[j % 3], 3.0 + (0.9 if (j // 3) % 2 == 0 else -0.9)) for j in range(6)]

# ---- K8 (one workgroup of 1024 striding) and K12m (256 per workgroup; norm pass of 16 x 256 float4 = 16 384 floats, a scalar tail
# for n % 4, a scalar loop for a bucket off a 16-byte boundary): 14 858 = the (23, 9) agent, 23 050 = the (39, 9) agent
K8_N = [1, 2, 1023, 1024, 1025, 14858, 23050]
K12M_N = [1, 3, 4, 5, 255, 256, 257, 16383, 16384, 16385, 16387, 23050]
NORMS = [0.5, 1e9]                  # the clip acting / idle
STARTS = [0, 7]                     # step0: zero moments / the state after seven reference steps
WORLDS = [1, 2, 8]                  # grad_scale = 1 / W
STEPS = 4
PROBE_N = [23050, 16387]
SPIKE = 3.0


def probe_positions(n):
    """the spike's positions: the ends of the first float4, of the first 256-thread stride, of the first pass, of the vector part,
    and the scalar tail"""
    n4 = 4 * (n // 4)
    return sorted({k for k in (0, 3, 4, 1023, 1024, 16383, 16384, n4 - 1, *range(n4, n)) if 0 <= k < n})


# ---- K7 -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_inputs(B, A, s=1.0, const_adv=None):
    """float32 CPU tensors of one case (read-only, shared)"""
    g = torch.Generator().manual_seed(LOSS_SEEDS.get((B, A, s), 2000 + 17 * B + A))
    logits = (s * torch.randn(B, A, generator=g)).contiguous()
    values, ret = torch.randn(B, generator=g), torch.randn(B, generator=g)
    act = torch.randint(0, A, (B,), generator=g)
    act[0], act[1] = 0, A - 1
    own = torch.log_softmax(logits.double(), -1).gather(1, act.view(-1, 1)).view(-1)
    old_lp = own + 0.3 * torch.randn(B, generator=g).double()
    adv = 3.0 + 0.5 * torch.randn(B, generator=g)
    if B >= 63:
        for j, (ratio, a) in enumerate(HAND_ROWS):
            old_lp[j] = own[j] - float(np.log(ratio))
            adv[j] = a
    if const_adv is not None:
        adv.fill_(const_adv)
    return dict(B=B, A=A, s=s, logits=logits, values=values, act=act.float(), old_lp=old_lp.float(), adv=adv, ret=ret)


def loss_on_outputs(logits, values, act, old_lp, adv, ret, dtype=torch.float64, weight=None, flip=None):
    """train.py:235-255 on given network outputs, through autograd with logits / values as leaves: the gradient of
    (sum_i weight_i (policy_i + VF value_i - EC entropy_i)) / B.  weight: per-sample weights (default ones; a 0 drops the sample, the
    divisor stays B and the advantage statistics stay those of all B).  flip: a sample whose clip decision is inverted.  Returns numpy
    float64: dlogits [B][A], dvalues [B], metrics (policy loss, value loss, entropy, total), ratio, adv_n."""
    lg = logits.detach().to(dtype).clone().requires_grad_(True)
    v = values.detach().to(dtype).clone().requires_grad_(True)
    act, old_lp, adv, ret = act.long(), old_lp.to(dtype), adv.to(dtype), ret.to(dtype)
    B = lg.shape[0]
    w = torch.ones(B, dtype=dtype) if weight is None else torch.as_tensor(weight, dtype=dtype)
    logp = torch.log_softmax(lg, -1)
    ent = -(logp.exp() * logp).sum(-1)
    new_lp = logp.gather(1, act.view(-1, 1)).view(-1)
    ratio = torch.exp(new_lp - old_lp)
    an = (adv - adv.mean()) / adv.std().clamp_min(1e-5)
    pl1, pl2 = -an * ratio, -an * torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP)
    first = pl1 >= pl2
    if flip is not None:
        first = first.clone()
        first[flip] = ~first[flip]
    pol = torch.where(first, pl1, pl2)
    val = 0.5 * (v - ret) ** 2
    sums = [(w * t).sum() / B for t in (pol, val, ent)]
    loss = sums[0] + VF * sums[1] - EC * sums[2]
    loss.backward()
    f = lambda t: t.detach().double().numpy().copy()
    return dict(dlogits=f(lg.grad), dvalues=f(v.grad), metrics=np.array([float(t.detach()) for t in (*sums, loss)]), ratio=f(ratio), adv_n=f(an))


@functools.lru_cache(maxsize=None)
def loss_case(B, A, s=1.0, const_adv=None):
    """the inputs with the float64 reference (`ref`) and the float32 CPU restatement (`r32`); computed once, shared, read-only"""
    c = dict(loss_inputs(B, A, s, const_adv))
    args = [c[k] for k in ("logits", "values", "act", "old_lp", "adv", "ret")]
    c["ref"], c["r32"] = loss_on_outputs(*args), loss_on_outputs(*args, dtype=torch.float32)
    return c


def loss_allowances(c):
    """(dlogits, dvalues): GRAD_ATOL / B + GRAD_RTOL |ref| (the outputs carry the 1 / B); at s = 30 `saturated_allowance` on the
    float32 CPU restatement"""
    r, r32 = c["ref"], c["r32"]
    if c["s"] == SAT:
        return tuple(saturated_allowance(r32[k], r[k]) for k in ("dlogits", "dvalues"))
    return tuple(GRAD_ATOL / c["B"] + GRAD_RTOL * np.abs(r[k]) for k in ("dlogits", "dvalues"))


def loss_wrong_answers(c):
    """The last sample dropped, and the clip decision inverted of the first sample whose ratio lies outside the clip range and whose
    taken action has a probability below 0.5 (None where the case holds none).  The probability: dlogits carries the decision times
    (1[k = a] - p_k), which at s = 30 is 1e-20 for a sample that took its policy's one likely action -- no decision of such a sample
    reaches an output, right or wrong."""
    args = [c[k] for k in ("logits", "values", "act", "old_lp", "adv", "ret")]
    w = np.ones(c["B"])
    w[-1] = 0.0
    r = c["ref"]["ratio"]
    p_taken = torch.softmax(c["logits"].double(), -1).gather(1, c["act"].long().view(-1, 1)).view(-1).numpy()
    out = np.nonzero(((r < 1.0 - CLIP) | (r > 1.0 + CLIP)) & (p_taken < 0.5))[0]
    return loss_on_outputs(*args, weight=w), (loss_on_outputs(*args, flip=int(out[0])) if len(out) else None)


# ---- K8 / K12m ----------------------------------------------------------------------------------------------------------------------
def clip_adam_steps(p0, m0, v0, step0, grads, max_norm, grad_scale, dtype=torch.float64, norm_skip=None, norm_eps=1e-6):
    """Per step: g = grad * grad_scale; coef = min(max_norm / (|g| + 1e-6), 1) (clip_grad_norm_); Adam(lr 3e-4, betas 0.9 / 0.999,
    eps 1e-5) with torch's bias correction.  One dict per step, numpy float64: param, exp_avg, exp_avg_sq, grad_clipped, norm.
    norm_skip (an element left out of the norm) and norm_eps are the wrong answers' knobs."""
    t = lambda x: torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(dtype).clone()
    p, m, v, step = t(p0), t(m0), t(v0), int(step0)
    f = lambda x: x.double().numpy().copy()
    out = []
    for grad in grads:
        g = t(grad) * grad_scale
        counted = g.clone()
        if norm_skip is not None:
            counted[norm_skip] = 0.0
        norm = torch.sqrt((counted * counted).sum())
        coef = torch.clamp(max_norm / (norm + norm_eps), max=1.0)
        gc = g * coef
        step += 1
        m = m + (1.0 - BETA1) * (gc - m)
        v = BETA2 * v + (1.0 - BETA2) * gc * gc
        bc1, bc2 = 1.0 - BETA1 ** step, 1.0 - BETA2 ** step
        p = p - (LR / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + EPS))
        out.append(dict(param=f(p), exp_avg=f(m), exp_avg_sq=f(v), grad_clipped=f(gc), norm=float(norm)))
    return out


def _gradients(n, g, count, first=0):
    out = []
    for t in range(first, first + count):
        x = (0.5 + torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g).float() * 2.0 - 1.0)
        out.append((x * (2.0 * (1.0 + 0.1 * (t % STEPS)) / float(x.double().norm()))).contiguous())
    return out


@functools.lru_cache(maxsize=None)
def adam_inputs(n, step0=0):
    """float32 CPU tensors: the start state (p, m, v at counter step0) and the STEPS gradients"""
    g = torch.Generator().manual_seed(5000 + n)
    p = 0.1 * torch.randn(n, generator=g)
    m, v = torch.zeros(n), torch.zeros(n)
    grads = _gradients(n, g, STEPS)
    if step0:
        last = clip_adam_steps(p, m, v, 0, _gradients(n, g, step0, first=1), MAX_NORM, 1.0)[-1]
        p, m, v = (torch.from_numpy(last[k]).float() for k in ("param", "exp_avg", "exp_avg_sq"))
    return dict(n=n, step0=step0, p=p, m=m, v=v, grads=grads)


@functools.lru_cache(maxsize=None)
def adam_case(n, step0, max_norm, dtype=torch.float64):
    """the reference of a cell (the same for every W: the bucket W g with grad_scale 1 / W is g)"""
    c = adam_inputs(n, step0)
    return clip_adam_steps(c["p"], c["m"], c["v"], step0, c["grads"], max_norm, 1.0, dtype)


def moment_allowances(gc):
    """(exp_avg, exp_avg_sq) from the float64 clipped gradient of the step: tests/test_ppo_update_f64_gpu.py's form"""
    al = allowance(gc)
    return 0.1 * al, 0.002 * np.abs(gc) * al + 1e-15


def adam_worst(got, r):
    """worst error / bar of (param, exp_avg, exp_avg_sq) of one step against its reference r; got: numpy float64 triples"""
    am, av = moment_allowances(r["grad_clipped"])
    return (float(np.abs(got[0] - r["param"]).max() / PARAM_ATOL), float((np.abs(got[1] - r["exp_avg"]) / am).max()),
            float((np.abs(got[2] - r["exp_avg_sq"]) / av).max()))


@functools.lru_cache(maxsize=None)
def probe_bucket(n, k):
    g = torch.Generator().manual_seed(7000 + n)
    b = 1e-3 * torch.randn(n, generator=g)
    b[k] = SPIKE
    return b.contiguous()


@functools.lru_cache(maxsize=None)
def probe_params(n):
    return 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(7100 + n))


# ---- the device state of one call ---------------------------------------------------------------------------------------------------
GUARD, GUARD_FILL, SENTINEL = 8, -3.0, 7.0


class Tail:
    """The device buffers of one pc_ppo_gather / pc_ppo_loss(_diag) / pc_clip_adam / pc_clip_adam_advanced call.  Every buffer lies
    between GUARD floats of GUARD_FILL on either side (`guards_hold` after the call); `out` buffers are pre-filled with SENTINEL.
    shift = n: every buffer starts n more floats into its allocation (n = 1: 4 bytes past a 16-byte boundary)."""

    def __init__(self, shift=0):
        self.shift, self._all = shift, []

    def _buf(self, numel, dtype):
        whole = torch.full((self.shift + 2 * GUARD + numel,), GUARD_FILL, device="cuda", dtype=dtype)
        lo = self.shift + GUARD
        self._all.append((whole, lo, lo + numel))
        part = whole[lo:lo + numel]
        assert part.data_ptr() % 16 == (4 * self.shift) % 16 or dtype != torch.float32
        return part

    def put(self, t):
        part = self._buf(t.numel(), t.dtype)
        part.copy_(t.reshape(-1))
        return part.view(t.shape)

    def out(self, *shape, fill=SENTINEL):
        part = self._buf(int(np.prod(shape)), torch.float32)
        part.fill_(fill)
        return part.view(shape)

    def guards_hold(self):
        torch.cuda.synchronize()
        return all(bool((w[:lo] == GUARD_FILL).all()) and bool((w[hi:] == GUARD_FILL).all()) for w, lo, hi in self._all)

    @staticmethod
    def _done(rc, name):
        _capi.check(rc, name)
        torch.cuda.synchronize()

    # K6
    @classmethod
    def gather(cls, idx, obs, act, lp, adv, ret, shift=0):
        t = cls(shift)
        B, D = idx.numel(), obs.shape[1]
        t.idx, t.src = t.put(idx), [t.put(x) for x in (obs, act, lp, adv, ret)]
        t.dst = [t.out(B, D)] + [t.out(B) for _ in range(4)]
        cls._done(lib.pc_ppo_gather(0, t.idx.data_ptr(), B, D, *(x.data_ptr() for x in t.src), *(x.data_ptr() for x in t.dst),
                                    torch.cuda.current_stream().cuda_stream), "pc_ppo_gather")
        return t

    # K7
    @classmethod
    def for_loss(cls, c, shift=0, fill=SENTINEL):
        t = cls(shift)
        t.B, t.A = c["B"], c["A"]
        t.inp = [t.put(c[k]) for k in ("logits", "values", "act", "old_lp", "adv", "ret")]
        t.dlogits, t.dvalues = t.out(t.B, t.A, fill=fill), t.out(t.B, fill=fill)
        t.metrics, t.diag = t.out(4, fill=0.0), t.out(_capi.PC_DIAG_FLOATS, fill=0.0)
        return t

    def _loss_args(self):
        return (0, *(x.data_ptr() for x in self.inp), self.B, self.A, CLIP, VF, EC, self.dlogits.data_ptr(), self.dvalues.data_ptr(),
                self.metrics.data_ptr())

    def loss(self):
        self._done(lib.pc_ppo_loss(*self._loss_args(), torch.cuda.current_stream().cuda_stream), "pc_ppo_loss")
        return self

    def loss_diag(self, target_kl=0.0):
        self._done(lib.pc_ppo_loss_diag(*self._loss_args(), self.diag.data_ptr(), target_kl, torch.cuda.current_stream().cuda_stream),
                   "pc_ppo_loss_diag")
        return self

    # K8 / K12m
    @classmethod
    def for_adam(cls, p, m, v, step, grad=None, shift=0):
        t = cls(shift)
        t.param, t.m, t.v = t.put(p), t.put(m), t.put(v)
        t.step, t.lr = t.out(1, fill=float(step)), t.out(1, fill=LR)
        t.grad = t.put(grad) if grad is not None else t.out(p.numel())
        return t

    def _adam_args(self, max_norm, grad_scale):
        return (0, self.param.data_ptr(), self.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.step.data_ptr(),
                self.lr.data_ptr(), self.param.numel(), max_norm, grad_scale, BETA1, BETA2, EPS, torch.cuda.current_stream().cuda_stream)

    def clip_adam(self, max_norm, grad_scale=1.0):
        self._done(lib.pc_clip_adam(*self._adam_args(max_norm, grad_scale)), "pc_clip_adam")
        return self

    def clip_adam_advanced(self, max_norm, grad_scale=1.0):
        self._done(lib.pc_clip_adam_advanced(*self._adam_args(max_norm, grad_scale)), "pc_clip_adam_advanced")
        return self

    def state(self):
        """(param, exp_avg, exp_avg_sq) as numpy float64"""
        return tuple(x.cpu().double().numpy() for x in (self.param, self.m, self.v))
