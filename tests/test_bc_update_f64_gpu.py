"""The imitation step on the GPU at its edge shapes: pc_bc_minibatch (K27 forward / cross-entropy head / backward, K11 reduce, K12 clip +
Adam) through the C-ABI against the float64 restatement of tests/bc_update_reference.py (imitation.bc_loss on a .double() copy of the
agent, clip_grad_norm_, torch.optim.Adam(lr 3e-4, eps 1e-5), computed on the CPU once per case), and on bits where the header promises
bits: the ignore rule, the label's truncation, the divisor, apply = 2, the buffers.  The bars are the PPO step's: gradient rtol 2e-4 /
atol 2e-7, metric sums rel 1e-5 / abs 1e-6, parameters 3e-6.  tests/test_bc_update_f64_host.py holds the inputs to the conditions these
bars rest on, among them that a head which loses the last sample, divides by the labelled count, takes an unlabelled sample as label 0
or moves a label by one is more than 20 x the allowance away.

Shapes (B, D, A): tests/ppo_update_reference.py's 17.  B: 2, 3, 7 one partly dead workgroup of eight samples; 8 one full; 9 a second
with one live sample; 255 / 256 / 257; 1023 a last workgroup of seven; 1024 the limit.  (D, A): the three compiled shapes and the
generic forms at their ends D = 1, 24 | 25, 40 and A = 1, 2, 3, 15.  Every workspace is pre-filled with NaN unless a test says 0."""
import functools

import numpy as np
import pytest
import torch

import bc_update_reference as Q
import ppo_update_reference as R
import update_tail_reference as U
from bc_update_reference import Call
from ppo_car_amd import _capi

pytestmark = pytest.mark.gpu

ONE_STEP, SATURATED_CASES, AGREEING, MULTI = Q.ONE_STEP, Q.SATURATED_CASES, Q.AGREEING, Q.MULTI
ONE_ACTION, EDGE_SHAPES, IGNORE_SHAPES, SINGLE_LABEL, SHARED, LEARNER_B, LABEL_EDGES = (Q.ONE_ACTION, Q.EDGE_SHAPES, Q.IGNORE_SHAPES, Q.SINGLE_LABEL,
                                                                                        Q.SHARED, Q.LEARNER_B, Q.LABEL_EDGES)
STATE = ("param", "grad", "m", "v", "step", "metrics")
NAN = float("nan")
sid = lambda s: f"B{s[0]}-D{s[1]}-A{s[2]}"


def _np(t):
    return t.cpu().double().numpy()


def _bc(c, label=None, idx=None, targets=True, vf=Q.VF, ec=Q.EC, apply=0, max_norm=Q.BC_MAX_NORM, ws_fill=NAN, call=None, **kw):
    """one pc_bc_minibatch call on the case's first minibatch (or `idx`), with the case's labels (or the pool labels `label`)"""
    call = Call(c["p0"].cuda(), c["B"], c["D"], c["A"], max_norm=max_norm, ec=ec, ws_fill=ws_fill, **kw) if call is None else call
    ix = (c["idx"][0] if idx is None else idx).cuda()
    lab = (c["label"] if label is None else label).cuda().contiguous()
    return call.bc(ix, c["obs"].cuda().contiguous(), lab, c["target"].cuda().contiguous() if targets else None, vf=vf, ec=ec, apply=apply)


def _metrics_hold(got, ref):
    for a, b, key in zip(got, ref, ("ce", "value_loss", "entropy", "loss")):
        assert float(a) == pytest.approx(float(b), rel=Q.MET_REL, abs=Q.MET_ABS), key


def _untouched(call, c):
    assert torch.equal(call.param.cpu(), c["p0"]) and float(call.step) == 0.0 and not call.m.any() and not call.v.any()


def _same(a, b, keys=STATE):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k      # (bits: NaN would equal NaN, -0 would differ from +0)


def _slices(by):
    return {k: round(v, 3) for k, v in by.items()}


# ---- 1. the gradient and the metric sums ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale,steps,max_norm,agree", ONE_STEP, ids=Q.ids(ONE_STEP))
def test_gradient_and_metrics_against_float64(shape, scale, steps, max_norm, agree):
    """apply = 0 against bc_loss in float64; param, the moments and step stay as they were.  Worst error / allowance measured on an
    MI355X: DESIGN 4.17 has the table."""
    c = Q.case(*shape, scale)
    r = c["ref"][0]
    call = _bc(c)
    g, m = _np(call.grad), _np(call.metrics)
    print(f"{sid(shape)} scale={scale:g}: worst error / allowance = {Q.worst(g, r['grad']):.3f}; by slice "
          f"{_slices(Q.worst_by_slice(g, r['grad'], *shape[1:]))}; metrics {m} reference {r['metrics']} ({Q.metric_worst(m, r['metrics']):.3f} of the bar)")
    assert np.allclose(g, r["grad"], rtol=Q.GRAD_RTOL, atol=Q.GRAD_ATOL)
    _metrics_hold(m, r["metrics"])
    _untouched(call, c)


@pytest.mark.parametrize("shape", R.SHAPES, ids=sid)
def test_without_targets_the_critic_rests_at_plus_zero(shape):
    """target = NULL with vf_coef = 0 against the call with targets and vf_coef = 0: the actor's four slices and the ce / ent sums are
    the same bits; without targets every critic element is +0.0f (no sign bit) and metrics[1] gets +0."""
    c = Q.case(*shape)
    o = Q.actor_end(*shape[1:])
    none, zero = _bc(c, targets=False, vf=0.0), _bc(c, vf=0.0)
    assert torch.equal(none.grad[:o].view(torch.int32), zero.grad[:o].view(torch.int32))
    assert not none.grad[o:].view(torch.int32).any()                       # (all bits clear: +0.0f)
    assert not none.metrics[1].view(torch.int32).any() and float(zero.metrics[1]) > 0.0
    assert torch.equal(none.metrics[[0, 2]], zero.metrics[[0, 2]])
    r = Q.run_steps(c, vf=0.0, targets=False)[0]
    assert np.allclose(_np(none.grad), r["grad"], rtol=Q.GRAD_RTOL, atol=Q.GRAD_ATOL) and not r["grad"][o:].any()
    _metrics_hold(_np(none.metrics), r["metrics"])
    _untouched(none, c)


# ---- 2. one action ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("shape", ONE_ACTION, ids=sid)
def test_one_action_leaves_the_actor_exactly_at_rest(shape, scale):
    """A = 1: log_softmax of one logit is the constant 0, so whatever the labels -- the case's, all 0, none -- the actor's four
    gradient slices are exact zeros and so are the ce and ent sums; the critic's slices are held to float64."""
    c = Q.case(*shape, scale)
    r = c["ref"][0]
    bounds = Q.slice_bounds(shape[1], 1)
    o = bounds[4][1]
    assert not r["grad"][:o].any()
    for name, lab in (("the case's", c["label"]), ("all 0", torch.zeros_like(c["label"])), ("none", torch.full_like(c["label"], -1.0))):
        call = _bc(c, label=lab)
        for k, s, e in bounds[:4]:
            assert torch.equal(call.grad[s:e], torch.zeros(e - s, device="cuda")), (name, k)
        assert float(call.metrics[0]) == 0.0 and float(call.metrics[2]) == 0.0, name
        g = _np(call.grad)
        assert np.allclose(g[o:], r["grad"][o:], rtol=Q.GRAD_RTOL, atol=Q.GRAD_ATOL) and np.abs(g[o:]).max() > 0, name
        _metrics_hold(_np(call.metrics), r["metrics"])


# ---- 3. the saturated softmax -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale,steps,max_norm,agree", SATURATED_CASES, ids=Q.ids(SATURATED_CASES))
def test_saturated_softmax_against_float64(shape, scale, steps, max_norm, agree):
    """actor[2] x 4000: logits of tens, probabilities of 1 and e-20.  torch's own float32 reaches 0.1 .. 0.8 of the standard gradient
    allowance here (the host test prints it; the figure moves with the CPU), so the gradient is held per element to  2e-4 |g64| + 4 max_i |g32_i - g64_i|,  g32 = the
    float32 CPU restatement of the same case, exactly as the PPO step's saturated cases are; a wrong head is hundreds of times that
    allowance away (host test).  The metric sums keep the project's bar."""
    c = Q.case(*shape, scale)
    r, r32 = c["ref"][0], Q.restated32(*shape, scale)[0]
    call = _bc(c)
    g, m = _np(call.grad), _np(call.metrics)
    e32 = float(np.abs(r32["grad"] - r["grad"]).max())
    print(f"{sid(shape)} scale=4000: max|g - g64| {np.abs(g - r['grad']).max():.3e}, max|g32 - g64| {e32:.3e}, ratio "
          f"{np.abs(g - r['grad']).max() / e32:.3f}; worst error / the standard allowance {Q.worst(g, r['grad']):.3f} (float32 torch: "
          f"{Q.worst(r32['grad'], r['grad']):.3f}); metrics {m} reference {r['metrics']} ({Q.metric_worst(m, r['metrics']):.3f} of the bar)")
    assert (np.abs(g - r["grad"]) <= Q.saturated_allowance(r32["grad"], r["grad"])).all()
    _metrics_hold(m, r["metrics"])
    _untouched(call, c)


@pytest.mark.parametrize("shape,scale,steps,max_norm,agree", AGREEING, ids=Q.ids(AGREEING))
def test_agreeing_labels_against_float64(shape, scale, steps, max_norm, agree):
    """Every label its row's float64 argmax, at scale 4000 and 24000: -log p is small and rounding in the log-softmax shows in the ce
    sum.  The standard allowance for the gradient, the project's bars for the metric sums."""
    c = Q.case(*shape, scale, 1, max_norm, True)
    r = c["ref"][0]
    call = _bc(c)
    g, m = _np(call.grad), _np(call.metrics)
    bar = Q.MET_ABS + Q.MET_REL * abs(r["metrics"][0])
    print(f"{sid(shape)} scale={scale:g} agreeing labels: ce {m[0]:.9e} float64 {r['metrics'][0]:.9e}: {abs(m[0] - r['metrics'][0]) / bar:.3f} of "
          f"the bar (float32 on the CPU in the kernel's order {abs(Q.ce_emulated(c, 'kernel') - r['metrics'][0]) / bar:.3f}, in torch's "
          f"{abs(Q.ce_emulated(c, 'torch') - r['metrics'][0]) / bar:.3f}); gradient worst error / allowance {Q.worst(g, r['grad']):.3f}")
    assert np.allclose(g, r["grad"], rtol=Q.GRAD_RTOL, atol=Q.GRAD_ATOL)
    _metrics_hold(m, r["metrics"])


# ---- 4. several applied steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale,steps,max_norm,agree", MULTI, ids=Q.ids(MULTI))
def test_four_applied_steps_against_float64(shape, scale, steps, max_norm, agree):
    """Four apply = 1 steps on four minibatches, the norm clip acting (BC_MAX_NORM) and idle (1e9), after every step: param at 3e-6,
    grad = the clipped gradient at the gradient's allowance, step, the metric increments, and the moments.  The moments' bars follow
    from the gradient's, which is asserted at every step: m_t = 0.9 m_(t-1) + 0.1 gc_t and v_t = 0.999 v_(t-1) + 0.001 gc_t^2 carry
    0.1 allowance(gc_t) and 0.002 |gc_t| allowance(gc_t) of each step forward with the same decay."""
    c = Q.case(*shape, scale, steps, max_norm)
    for r in c["ref"]:      # (the host test has the same condition)
        assert (r["norm"] > max_norm) == (max_norm == Q.BC_MAX_NORM)
    call = Call(c["p0"].cuda(), *shape, max_norm=max_norm, ws_fill=NAN)
    before, met = c["p0"].double().numpy(), np.zeros(4)
    am, av = 0.0, 0.0
    for t, r in enumerate(c["ref"]):
        _bc(c, idx=c["idx"][t], apply=1, call=call)
        p, g, m = _np(call.param), _np(call.grad), _np(call.metrics)
        a1, a2 = U.moment_allowances(r["grad_clipped"])
        am, av = 0.9 * am + a1, 0.999 * av + a2
        wm, wv = float((np.abs(_np(call.m) - r["exp_avg"]) / am).max()), float((np.abs(_np(call.v) - r["exp_avg_sq"]) / av).max())
        print(f"{sid(shape)} max_norm {max_norm:g} step {t + 1}: parameters max abs err {np.abs(p - r['param']).max():.3e}; clipped gradient "
              f"worst error / allowance {Q.worst(g, r['grad_clipped']):.3f}; exp_avg {wm:.3f}, exp_avg_sq {wv:.3f} of their bars; metric "
              f"increments {Q.metric_worst(m - met, r['metrics']):.3f} of theirs")
        assert np.abs(p - r["param"]).max() <= Q.PARAM_ATOL
        assert np.abs(r["param"] - before).max() > 1e-4          # (the step is visible at that tolerance)
        assert float(call.step) == t + 1.0
        assert np.allclose(g, r["grad_clipped"], rtol=Q.GRAD_RTOL, atol=Q.GRAD_ATOL)
        assert wm <= 1.0 and wv <= 1.0
        _metrics_hold(m - met, r["metrics"])
        before, met = r["param"], m


# ---- 5. apply = 2 -----------------------------------------------------------------------------------------------------------------
def _advanced(call, max_norm):
    _capi.check(_capi.lib.pc_clip_adam_advanced(0, call.param.data_ptr(), call.grad.data_ptr(), call.m.data_ptr(), call.v.data_ptr(),
                                                call.step.data_ptr(), call.lr.data_ptr(), call.param.numel(), max_norm, 1.0, U.BETA1, U.BETA2,
                                                U.EPS, torch.cuda.current_stream().cuda_stream), "pc_clip_adam_advanced")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape,scale,steps,max_norm,agree", MULTI, ids=Q.ids(MULTI))
def test_apply_2_leaves_the_raw_gradient_and_the_exchange_step_completes_it(shape, scale, steps, max_norm, agree):
    """include/ppocar.h: apply == 2 stops after the gradient but advances the step counter: grad is apply = 0's raw gradient bit for
    bit whatever max_norm, parameters and moments untouched.  pc_clip_adam_advanced (K12m) on that gradient then completes the step:
    over four steps it is held to the float64 trajectory, and with the clip idle K12 and K12m share adam_coef / adam_elem with
    coef == 1.0f, so parameters, moments, counter and metrics are apply = 1's bits."""
    c = Q.case(*shape, scale, steps, max_norm)
    zero, two = _bc(c, apply=0, max_norm=max_norm), _bc(c, apply=2, max_norm=max_norm)
    assert float(two.step) == 1.0 and float(zero.step) == 0.0
    assert torch.equal(two.param.cpu(), c["p0"]) and not two.m.any() and not two.v.any()
    _same(two, zero, ("grad", "metrics", "param", "m", "v"))
    assert np.allclose(_np(two.grad), c["ref"][0]["grad"], rtol=Q.GRAD_RTOL, atol=Q.GRAD_ATOL)
    one = Call(c["p0"].cuda(), *shape, max_norm=max_norm, ws_fill=NAN)
    two = Call(c["p0"].cuda(), *shape, max_norm=max_norm, ws_fill=NAN)
    for t, r in enumerate(c["ref"]):
        _bc(c, idx=c["idx"][t], apply=1, call=one)
        _bc(c, idx=c["idx"][t], apply=2, call=two)
        raw = two.grad.clone()
        _advanced(two, max_norm)
        assert torch.equal(two.grad, raw) and float(two.step) == t + 1.0
        if max_norm == Q.BC_IDLE_NORM:
            _same(one, two)
        err = float(np.abs(_np(two.param) - r["param"]).max())
        print(f"{sid(shape)} max_norm {max_norm:g} step {t + 1}: apply = 2 + pc_clip_adam_advanced, parameters max abs err {err:.3e}")
        assert err <= Q.PARAM_ATOL


# ---- 6. the label's edges, on bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first_group", "last_group"])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=sid)
def test_label_edges_give_the_bits_of_their_whole_label(shape, where):
    """One live sample's label overwritten with each value of LABEL_EDGES, in the first (full) group and in the last, partly dead one:
    grad and metrics are the bits of the call with the stated whole label or with -1 -- `labelled` is 0 <= label < A on the float,
    (int)label truncates, -0.0 is label 0, the largest float below A is label A - 1, the largest negative denormal, NaN, +-inf, +-3e38
    and 2^31, 2^32 are no label (include/ppocar.h: "outside 0 .. A-1: no label").  Nothing non-finite anywhere: grad, metrics, or the
    workspace (pre-filled with 0 here, so it is finite iff everything written to it is)."""
    c = Q.case(*shape)
    A = shape[2]
    j = Q.edge_samples(c)[where == "last_group"]
    whole = functools.lru_cache(maxsize=None)(lambda w: _bc(c, label=Q.with_label(c, j, float(w)), ws_fill=0.0))
    if A > 1:      # (not vacuous: label 0, label A - 1 and no label are three gradients)
        assert not torch.equal(whole(0).grad, whole(A - 1).grad) and not torch.equal(whole(0).grad, whole(-1).grad)
        assert not torch.equal(whole(A - 1).grad, whole(-1).grad)
    for name, value, w in LABEL_EDGES[A]:
        lab = Q.with_label(c, j, value)
        assert lab.view(torch.int32)[int(c["idx"][0][j])].item() == np.float32(value).view(np.int32)      # (the value arrived bit for bit)
        call = _bc(c, label=lab, ws_fill=0.0)
        for k in ("grad", "metrics"):
            assert torch.equal(getattr(call, k).view(torch.int32), getattr(whole(w), k).view(torch.int32)), (name, k)
        for k in ("grad", "metrics", "ws"):
            assert bool(torch.isfinite(getattr(call, k)).all()), (name, k)
        _untouched(call, c)


# ---- 7. the divisor and the ignore rule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", IGNORE_SHAPES, ids=sid)
def test_every_kind_of_no_label_is_the_same_bits_and_a_label_is_not(shape):
    """Every unlabelled row's -1 replaced by another "no label" value (A, A + 3, NaN, -inf, 3e38, -0.5 in turn): no bit of grad or
    metrics changes.  The unlabelled samples replaced by copies of the first labelled sample's row (the same B): another gradient, held
    to float64 -- so the first half is no vacuous pass, and a divisor of "labelled samples" (host test: 340 x the allowance and more)
    would show in one of the two."""
    c = Q.case(*shape)
    A = shape[2]
    base = _bc(c)
    none = torch.nonzero(c["label"] == -1.0).view(-1)
    other = c["label"].clone()
    other[none] = torch.tensor([float(A), A + 3.0, NAN, float("-inf"), 3e38, -0.5])[torch.arange(len(none)) % 6]
    assert len(none) >= 2 and not bool(Q.is_labelled(other[none], A).any())
    _same(_bc(c, label=other), base, ("grad", "metrics"))
    ix = Q.all_labelled(c)
    r = Q.run_steps(dict(c, idx=[ix]))[0]
    call = _bc(c, idx=ix)
    assert not torch.equal(call.grad, base.grad) and not torch.equal(call.metrics[0], base.metrics[0])
    assert np.allclose(_np(call.grad), r["grad"], rtol=Q.GRAD_RTOL, atol=Q.GRAD_ATOL)
    _metrics_hold(_np(call.metrics), r["metrics"])


@pytest.mark.parametrize("shape", SINGLE_LABEL, ids=sid)
def test_one_labelled_sample_in_the_minibatch(shape):
    """One labelled sample, the last one (in the partly dead group); every other label is -1.  The actor's gradient is 1 / B of that
    sample's alone (host test): held to float64 at the standard allowance, and where the reference is exactly 0 at atol alone -- the
    dead and the unlabelled lanes add exact zeros.  The ce and ent sums are that sample's / B."""
    c = Q.case(*shape)
    ix, lab, j = Q.single_label(c)
    r = Q.run_steps(dict(c, idx=[ix], label=lab))[0]
    call = _bc(c, label=lab, idx=ix)
    g = _np(call.grad)
    zero = r["grad"] == 0.0
    print(f"{sid(shape)} one labelled sample: worst error / allowance {Q.worst(g, r['grad']):.3f}; {int(zero.sum())} reference elements are exactly "
          f"0, the kernel's largest there {np.abs(g[zero]).max() if zero.any() else 0.0:.3e}")
    assert np.allclose(g, r["grad"], rtol=Q.GRAD_RTOL, atol=Q.GRAD_ATOL)
    assert (np.abs(g[zero]) <= Q.GRAD_ATOL).all()
    _metrics_hold(_np(call.metrics), r["metrics"])
    # without its label the actor rests exactly, and the critic's slices keep their bits
    o = Q.actor_end(*shape[1:])
    rest = _bc(c, label=torch.full_like(lab, -1.0), idx=ix)
    assert not rest.grad[:o].any() and torch.equal(rest.grad[o:], call.grad[o:]) and bool(call.grad[:o].any())
    assert float(rest.metrics[0]) == 0.0 and float(rest.metrics[2]) == 0.0 and torch.equal(rest.metrics[1], call.metrics[1])


# ---- 8. robustness, on bits -------------------------------------------------------------------------------------------------------
def _into(t, n):
    """the same values as a view n elements into a larger allocation whose other elements are NaN (idx: -1)"""
    big = torch.full((t.numel() + 2 * n,), -1 if t.dtype == torch.int64 else NAN, dtype=t.dtype, device="cuda")
    v = big[n:n + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (n * t.element_size()) % 16 and v.is_contiguous()
    return v


@pytest.mark.parametrize("shape", R.ROBUST, ids=sid)
def test_the_same_bits_whatever_the_buffers(shape):
    """One applied step: twice in a row on fresh state; with the workspace full of NaN and full of 0 (nothing is read that the step has
    not written); with grad, the moments, step, lr and metrics 1 and 3 floats into a larger allocation and idx, obs, label, target 1 and
    3 elements into theirs (include/ppocar.h asks 16-byte alignment of `param` and the workspace, nothing else); the floats around grad,
    the moments, step, lr and metrics keep their fill."""
    c = Q.case(*shape)
    p0 = c["p0"].cuda()
    ix, obs, lab, tgt = (c["idx"][0].cuda(), c["obs"].cuda(), c["label"].cuda(), c["target"].cuda())

    def run(n=0, **kw):
        call = Call(p0, *shape, max_norm=Q.BC_MAX_NORM, **kw)
        args = (ix, obs, lab, tgt) if n == 0 else tuple(_into(t, n) for t in (ix, obs, lab, tgt))
        return call.bc(*args, apply=1)

    base = run(ws_fill=NAN)
    assert float(base.step) == 1.0 and bool(torch.isfinite(base.param).all()) and not torch.equal(base.param, p0)
    assert bool(torch.isfinite(base.grad).all()) and bool(torch.isfinite(base.metrics).all())
    others = dict(again=run(ws_fill=NAN), zero_workspace=run(ws_fill=0.0), shift_1=run(1, ws_fill=NAN, shift=1), shift_3=run(3, ws_fill=NAN, shift=3))
    for name, o in others.items():
        _same(base, o)
    for n in (1, 3):
        o = others[f"shift_{n}"]
        assert o.grad.data_ptr() % 16 == 4 * n and o.param.data_ptr() % 16 == 0 and o.ws.data_ptr() % 16 == 0
        for k in ("grad", "m", "v", "step", "lr", "metrics"):
            whole = getattr(o, k)._base
            assert whole.numel() == getattr(o, k).numel() + 2 * n and bool((whole[:n] == -3.0).all()) and bool((whole[-n:] == -3.0).all()), (n, k)
    # a second step on the same state object: the workspace it left behind is overwritten, not read
    a, b = run(ws_fill=NAN), run(ws_fill=0.0)
    for call in (a, b):
        call.bc(ix, obs, lab, tgt, apply=1)
    _same(a, b)
    assert float(a.step) == 2.0


# ---- 9. the halves shared with pc_ppo_minibatch, at the edges ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHARED, ids=sid)
def test_the_shared_halves_are_the_ppo_steps_bits(shape):
    """The PPO case's inputs (tests/ppo_update_reference.py): every label live (= act), target = ret, the same coefficients.  The
    critic's four gradient slices and the value-loss and entropy sums are the same statements in both kernels: the same bits."""
    c = R.case(*shape)
    data = tuple(c[k].cuda().contiguous() for k in ("obs", "act", "old_lp", "adv", "ret"))
    ix = c["idx"][0].cuda()
    assert bool(Q.is_labelled(c["act"], shape[2]).all())
    p0 = c["p0"].cuda()
    bc = Call(p0, *shape, ws_fill=NAN).bc(ix, data[0], data[1], data[4])
    ppo = Call(p0, *shape, ws_fill=NAN).ppo(ix, *data)
    o = Q.actor_end(*shape[1:])
    assert torch.equal(bc.grad[o:].view(torch.int32), ppo.grad[o:].view(torch.int32)) and float(bc.grad[o:].abs().max()) > 0
    assert torch.equal(bc.metrics[1:3], ppo.metrics[1:3]) and bool((bc.metrics[1:3] > 0).all())
    assert not torch.equal(bc.grad[:o], ppo.grad[:o])      # (the actor's loss is another one)


# ---- 10. the learner --------------------------------------------------------------------------------------------------------------
def _learner(c, seed=Q.LEARNER_SEED, agent_seed=None):
    from ppo_car_amd.imitation import BCLearner
    if agent_seed is None:
        agent = Q._agent_as(c, torch.float32)
    else:
        torch.manual_seed(agent_seed)
        agent = Q.Agent(c["D"], c["A"])
    L = BCLearner(agent.cuda(), batch_size=c["B"], vf_coef=Q.VF, ent_coef=Q.EC, max_grad_norm=Q.LEARNER_NORM, learning_rate=Q.LR, seed=seed)
    assert L.path == "custom"
    return L


@pytest.mark.parametrize("B", LEARNER_B)
def test_learner_epoch_against_float64_and_restored_state(B):
    """BCLearner(batch_size = B) on the custom path: one fit epoch over 3 B + 5 rows is three steps on the permutation draw_indices
    draws, the tail of five cut (B = 2: five steps, a tail of one) -- parameters within 3e-6 x steps of run_steps in float64 on the same indices (tests/
    test_imitation_gpu.py's form of the bar), the bc/* means at the metric bars.  state_dict -> a fresh learner (other weights, other
    seed) -> load_state_dict -> one more epoch: the uninterrupted run's bits."""
    c = Q.learner_case(B)
    obs, label, target = (c[k].cuda().contiguous() for k in ("obs", "label", "target"))
    assert torch.equal(_learner(c).draw_indices(c["pool"]).cpu().view(-1), torch.cat(c["idx"]))
    L = _learner(c)
    assert torch.equal(L.flat_param.cpu(), c["p0"])
    out = L.fit(obs, label, target, epochs=1)
    r, n = c["ref"], len(c["idx"])
    err = float(np.abs(_np(L.flat_param) - r[-1]["param"]).max())
    print(f"BCLearner(batch_size={B}) after {n} steps: parameters max abs err {err:.3e}; {out}")
    assert n == (5 if B == 2 else 3) and out["bc/steps"] == n and float(L.step_count) == n and L.steps == n
    assert err <= Q.PARAM_ATOL * n and np.abs(r[-1]["param"] - c["p0"].double().numpy()).max() > 1e-4
    _metrics_hold([out[k] for k in L.KEYS], np.mean([s["metrics"] for s in r], 0))
    sd = L.state_dict()
    L.fit(obs, label, target, epochs=1)
    F = _learner(c, seed=11, agent_seed=99)
    assert not torch.equal(F.flat_param, sd["param"])
    F.load_state_dict(sd)
    F.fit(obs, label, target, epochs=1)
    for k in ("flat_param", "flat_grad", "exp_avg", "exp_avg_sq", "step_count", "metrics"):
        assert torch.equal(getattr(F, k), getattr(L, k)), k
    assert float(F.step_count) == 2 * n and F.steps == 2 * n
