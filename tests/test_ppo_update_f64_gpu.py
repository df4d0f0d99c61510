"""The small-minibatch PPO step on the GPU at its edge shapes: pc_ppo_minibatch (K10 forward / loss / backward, K11 reduce, K12 clip +
Adam) through the C-ABI against the float64 restatement of tests/ppo_update_reference.py (ppo.ppo_loss on a .double() copy of the agent,
clip_grad_norm_, torch.optim.Adam(lr 3e-4, eps 1e-5), computed on the CPU once per case), and the other forms of the step -- prepared
minibatches, the diagnostics entry point, the epoch chain -- against the plain step on bits.  The bars are tests/test_ppo_golden.py's:
gradient rtol 2e-4 / atol 2e-7, metric sums rel 1e-5 / abs 1e-6, parameters 3e-6.  tests/test_ppo_update_f64_host.py holds the inputs
to the conditions these bars rest on.

Shapes (B, D, A).  B: 2, 3, 7 one partly dead workgroup of eight samples; 8 one full; 9 a second with one live sample; 255 / 256 / 257
around the 256 threads of the advantage statistics; 1023 a last workgroup of seven; 1024 the limit, 128 partials.  (D, A): the three
compiled shapes (23, 9), (18, 9), (39, 9); the generic forms at their ends D = 1, 24 | 25, 40 and A = 1, 2, 3, 15, which cut layer 2
into 4, 4, 4 and 2 parts (A = 9: 3)."""
import functools

import numpy as np
import pytest
import torch

import ppo_update_reference as R
from ppo_update_reference import Call

pytestmark = pytest.mark.gpu

DATA = ("obs", "act", "old_lp", "adv", "ret")
STATE = ("param", "grad", "m", "v", "step", "metrics")
sid = lambda s: f"B{s[0]}-D{s[1]}-A{s[2]}"


def _dev(c):
    """the case's tensors on the device: (the five data tensors), [idx of every step]"""
    return tuple(c[k].cuda().contiguous() for k in DATA), [ix.cuda() for ix in c["idx"]]


def _np(t):
    return t.cpu().double().numpy()


def _metrics_hold(got, ref):
    for a, b, key in zip(got, ref, ("policy_loss", "value_loss", "entropy", "loss")):
        assert float(a) == pytest.approx(float(b), rel=R.MET_REL, abs=R.MET_ABS), key


def _one_step(c, apply=0, **kw):
    data, idx = _dev(c)
    return Call(c["p0"].cuda(), c["B"], c["D"], c["A"], **kw).ppo(idx[0], *data, apply=apply)


def _untouched(call, c):
    assert torch.equal(call.param.cpu(), c["p0"]) and float(call.step) == 0.0 and not call.m.any() and not call.v.any()


# ---- a. the gradient and the metric sums ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("shape", R.SHAPES, ids=sid)
def test_gradient_and_metrics_against_float64(shape, scale):
    """apply = 0 against ppo_loss in float64.  Worst error / allowance measured on an MI355X over the 17 shapes: 0.102 at both scales
    ((9, 39, 9), critic.2.weight), 0.06 or less everywhere else; torch's own float32 on the CPU: 0.073 (DESIGN 4.3 has the table)."""
    c = R.case(*shape, scale)
    r = c["ref"][0]
    call = _one_step(c)
    g, m = _np(call.grad), _np(call.metrics)
    print(f"B={shape[0]} D={shape[1]} A={shape[2]} scale={scale}: worst error / allowance = {R.worst(g, r['grad']):.3f}; by slice "
          f"{ {k: round(v, 3) for k, v in R.worst_by_slice(g, r['grad'], shape[1], shape[2]).items()} }; metrics {m} reference {r['metrics']}")
    assert np.allclose(g, r["grad"], rtol=R.GRAD_RTOL, atol=R.GRAD_ATOL)
    _metrics_hold(m, r["metrics"])
    _untouched(call, c)


# ---- b. one action ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[2] == 1], ids=sid)
def test_one_action_leaves_the_actor_exactly_at_rest(shape, scale):
    """A = 1: the log-prob is 0 whatever the weights, so the actor's four gradient slices are exactly zero (either sign) and so is the
    entropy sum; the critic's slices are held as above."""
    c = R.case(*shape, scale)
    r = c["ref"][0]
    call = _one_step(c)
    bounds = R.slice_bounds(shape[1], 1)
    for k, s, e in bounds[:4]:
        assert torch.equal(call.grad[s:e], torch.zeros(e - s, device="cuda")), k
        assert not r["grad"][s:e].any()
    assert float(call.metrics[2]) == 0.0
    o = bounds[4][1]
    g = _np(call.grad)
    assert np.allclose(g[o:], r["grad"][o:], rtol=R.GRAD_RTOL, atol=R.GRAD_ATOL) and np.abs(g[o:]).max() > 0
    _metrics_hold(_np(call.metrics), r["metrics"])


# ---- c. the saturated softmax -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SATURATED, ids=sid)
def test_saturated_softmax_against_float64(shape):
    """actor[2] x 4000: logits of tens, probabilities of 1 and e-20.  torch's own float32 misses the gradient's bar here by 1.0 .. 5.2 x
    (the host test prints it; the figure moves with the CPU), so the gradient is held per element to  2e-4 |g64| + 4 max_i |g32_i - g64_i|,  g32 = the float32 CPU
    restatement of the same case: the kernel sums the same ill-conditioned terms in another order (k-parts, groups of eight, partials)
    and may exceed torch's worst element by a small factor; a dropped sample or a wrong branch is hundreds of times that allowance (host
    test).  The metric sums keep the project's bar.  Measured max|g - g64| / max|g32 - g64| on an MI355X: DESIGN 4.3."""
    c = R.case(*shape, 4000.0)
    r, r32 = c["ref"][0], R.restated32(*shape, 4000.0)[0]
    call = _one_step(c)
    g, m = _np(call.grad), _np(call.metrics)
    e32 = float(np.abs(r32["grad"] - r["grad"]).max())
    allow = R.saturated_allowance(r32["grad"], r["grad"])
    print(f"B={shape[0]} D={shape[1]} A={shape[2]} scale=4000: max|g - g64| {np.abs(g - r['grad']).max():.3e}, max|g32 - g64| {e32:.3e}, ratio "
          f"{np.abs(g - r['grad']).max() / e32:.3f}; worst error / the project's allowance {R.worst(g, r['grad']):.3f} (float32 torch: "
          f"{R.worst(r32['grad'], r['grad']):.3f}); metrics {m} reference {r['metrics']}")
    assert (np.abs(g - r["grad"]) <= allow).all()
    _metrics_hold(m, r["metrics"])
    _untouched(call, c)


# ---- d. several applied steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [0.5, 1e9])
@pytest.mark.parametrize("shape", R.APPLIED, ids=sid)
def test_four_applied_steps_against_float64(shape, max_norm):
    """Four apply = 1 steps on four minibatches: bias correction after the first step, non-zero moments, the norm clip acting (0.5) and
    idle (1e9).  The moments' bars after the first step follow from the gradient's: m = 0.1 gc, v = 0.001 gc^2."""
    c = R.case(*shape, 1.0, 4, max_norm)
    for r in c["ref"]:      # (the host test has the same condition)
        assert (r["norm"] > max_norm) == (max_norm == 0.5)
    data, idx = _dev(c)
    call = Call(c["p0"].cuda(), *shape, max_norm=max_norm)
    before = c["p0"].double().numpy()
    for t, r in enumerate(c["ref"]):
        call.ppo(idx[t], *data, apply=1)
        p, g = _np(call.param), _np(call.grad)
        print(f"{sid(shape)} max_norm {max_norm} step {t + 1}: parameters max abs err {np.abs(p - r['param']).max():.3e}; clipped gradient worst "
              f"error / allowance {R.worst(g, r['grad_clipped']):.3f}")
        assert np.abs(p - r["param"]).max() <= R.PARAM_ATOL
        assert np.abs(r["param"] - before).max() > 1e-4          # (the step is visible at that tolerance)
        assert float(call.step) == t + 1.0
        assert np.allclose(g, r["grad_clipped"], rtol=R.GRAD_RTOL, atol=R.GRAD_ATOL)
        if t == 0:
            gc = r["grad_clipped"]
            al = R.allowance(gc)
            assert (np.abs(_np(call.m) - 0.1 * gc) <= 0.1 * al).all()
            assert (np.abs(_np(call.v) - 0.001 * gc * gc) <= 0.002 * np.abs(gc) * al + 1e-15).all()
        before = r["param"]


@pytest.mark.parametrize("max_norm", [0.5, 1e9])
@pytest.mark.parametrize("shape", R.APPLIED, ids=sid)
def test_apply_2_advances_the_counter_and_leaves_the_raw_gradient(shape, max_norm):
    """include/ppocar.h: apply == 2 stops after the gradient but advances the step counter (the caller exchanges the gradient, then
    pc_clip_adam_advanced): parameters and moments untouched, grad unclipped whatever max_norm."""
    c = R.case(*shape, 1.0, 4, max_norm)
    r = c["ref"][0]
    zero, two = _one_step(c, 0, max_norm=max_norm), _one_step(c, 2, max_norm=max_norm)
    assert float(two.step) == 1.0 and float(zero.step) == 0.0
    assert torch.equal(two.param.cpu(), c["p0"]) and not two.m.any() and not two.v.any()
    assert np.allclose(_np(two.grad), r["grad"], rtol=R.GRAD_RTOL, atol=R.GRAD_ATOL)
    assert torch.equal(two.grad, zero.grad) and torch.equal(two.metrics, zero.metrics)


# ---- e. constant advantages -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8, 256])
def test_constant_advantages(B):
    """Every adv = 0.5 with B a power of two: sum and mean are exact, the deviations are 0, the standard deviation takes its floor 1e-5,
    the normalised advantage is exactly 0: the policy-loss sum is exactly 0 and the actor's gradient is the entropy term's alone."""
    D, A = 23, 9
    c = R.case(B, D, A, 1.0, 1, R.MAX_NORM, 0.5)
    r = c["ref"][0]
    assert not r["adv_n"].any() and r["metrics"][0] == 0.0
    ent_only = R.gradient_of(c, entropy_only=True)
    o = R.slice_bounds(D, A)[4][1]
    assert np.abs(ent_only[:o] - r["grad"][:o]).max() <= 1e-15 and not ent_only[o:].any() and np.abs(ent_only[:o]).max() > 1e-6
    call = _one_step(c)
    g = _np(call.grad)
    print(f"B={B}: actor against the entropy term alone, worst error / allowance {R.worst(g[:o], ent_only[:o]):.3f}; whole gradient {R.worst(g, r['grad']):.3f}")
    assert float(call.metrics[0]) == 0.0
    assert np.allclose(g[:o], ent_only[:o], rtol=R.GRAD_RTOL, atol=R.GRAD_ATOL)
    assert np.allclose(g, r["grad"], rtol=R.GRAD_RTOL, atol=R.GRAD_ATOL)
    _metrics_hold(_np(call.metrics), r["metrics"])


# ---- f. robustness, on bits -------------------------------------------------------------------------------------------------------
def _one_element_in(t):
    """the same values as a view one element into a larger allocation: 4 bytes past a 16-byte boundary"""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = big[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("shape", R.ROBUST, ids=sid)
def test_the_same_bits_whatever_the_buffers(shape):
    """One applied step: twice; with the workspace full of NaN (nothing is read that the step has not written); with grad, the moments,
    step, lr and metrics each 16 bytes into a larger allocation; with obs / act / old_lp / adv / ret one element into a larger
    allocation, which no 16-byte load could take (include/ppocar.h asks no alignment of pc_ppo_minibatch's arguments)."""
    c = R.case(*shape)
    data, idx = _dev(c)
    p0 = c["p0"].cuda()
    run = lambda d=data, **kw: Call(p0, *shape, **kw).ppo(idx[0], *d, apply=1)
    base = run()
    others = dict(again=run(), nan_workspace=run(ws_fill=float("nan")), shifted_state=run(shift=4),
                  unaligned_inputs=run(tuple(_one_element_in(t) for t in data)))
    assert others["shifted_state"].grad.data_ptr() % 16 == 0 and others["shifted_state"].grad.data_ptr() != others["shifted_state"].grad.untyped_storage().data_ptr()
    assert float(base.step) == 1.0 and bool(torch.isfinite(base.param).all()) and not torch.equal(base.param, p0)
    for name, o in others.items():
        for k in STATE:
            assert torch.equal(getattr(base, k), getattr(o, k)), (name, k)


# ---- the other forms at the edge shapes, on bits ----------------------------------------------------------------------------------
def _snap(call):
    return {k: getattr(call, k).clone() for k in STATE}


@functools.lru_cache(maxsize=None)
def _plain(shape):
    """pc_ppo_minibatch on the case's three minibatches: the gradient-only call, and the state after each of three applied steps"""
    c = R.case(*shape, 1.0, 3)
    data, idx = _dev(c)
    only = _snap(Call(c["p0"].cuda(), *shape).ppo(idx[0], *data, apply=0))
    call, applied = Call(c["p0"].cuda(), *shape), []
    for ix in idx:
        applied.append(_snap(call.ppo(ix, *data, apply=1)))
    return only, applied


def _prepared(c):
    data, idx = _dev(c)
    prep = R.prepare(torch.stack(idx).contiguous(), c["B"], c["D"], *data)
    assert bool(torch.isfinite(prep).all())
    return prep


def _same(call, want, keys=STATE):
    for k in keys:
        assert torch.equal(getattr(call, k), want[k]), k


@pytest.mark.parametrize("shape", R.FORMS, ids=sid)
def test_prepared_minibatches_equal_the_plain_step(shape):
    c = R.case(*shape, 1.0, 3)
    only, applied = _plain(shape)
    prep = _prepared(c)
    _same(Call(c["p0"].cuda(), *shape).prepared(prep[0], apply=0), only)
    call = Call(c["p0"].cuda(), *shape)
    for t in range(3):
        _same(call.prepared(prep[t], apply=1), applied[t])
    assert float(call.step) == 3.0 and not torch.equal(applied[2]["param"], applied[0]["param"])


@pytest.mark.parametrize("shape", R.FORMS, ids=sid)
def test_diagnostics_form_equals_the_plain_step_and_float64(shape):
    """target_kl = 0: the stop is off.  grad, metrics, param and the moments are the plain step's bits; diag[0..2] = (approx_kl,
    clipfrac, 1) of float64 at test_update_diagnostics_gpu.py's bars: 1e-5 on the KL, the clipped count exact (no ratio is within
    1e-5 of a clip edge: the host test)."""
    c = R.case(*shape, 1.0, 3)
    r = c["ref"][0]["ratio"]
    kl, count = float(((r - 1.0) - np.log(r)).mean()), int((np.abs(r - 1.0) > R.CLIP).sum())
    data, idx = _dev(c)
    call = Call(c["p0"].cuda(), *shape, diag=True).ppo_diag(idx[0], *data, apply=1, target_kl=0.0)
    _same(call, _plain(shape)[1][0])
    d = call.diag.tolist()
    print(f"{sid(shape)}: approx_kl {d[0]!r} float64 {kl!r}; clipped {d[1] * shape[0]!r} float64 {count}")
    assert abs(d[0] - kl) <= 1e-5
    assert d[1] == float(np.float32(count) / np.float32(shape[0]))      # (one correctly rounded float32 division of two exact integers)
    assert d[2] == 1.0 and d[3] == 1.0 and d[4] == 0.0 and d[5] == d[0]


@pytest.mark.parametrize("shape", R.FORMS, ids=sid)
def test_epoch_chain_equals_three_prepared_steps(shape):
    """pc_ppo_epoch_prepared with n_mb = 3: the compiled shapes take the deferred chain (clip + Adam inside the next forward / backward
    launch), the generic ones three launches per minibatch: param, the moments, step, metrics and grad are the plain steps' bits."""
    c = R.case(*shape, 1.0, 3)
    call = Call(c["p0"].cuda(), *shape).epoch(_prepared(c), 3)
    _same(call, _plain(shape)[1][2])
    assert float(call.step) == 3.0
