"""The soft-target imitation step on the GPU at its edge shapes: pc_bc_minibatch_soft (the LOSS_BC_SOFT head of the shared forward /
backward body, K11 reduce, K12 clip + Adam) through the C-ABI against the float64 restatement of tests/bc_soft_reference.py
(imitation.bc_soft_loss on a .double() copy of the agent, clip_grad_norm_, torch.optim.Adam(lr 3e-4, eps 1e-5), computed on the CPU once
per case), and on bits where the header promises bits: a one-hot row gives pc_bc_minibatch's bits, an unlabelled row rests at +0, the
buffers.  The bars are the project's: gradient rtol 2e-4 / atol 2e-7, metric sums rel 1e-5 / abs 1e-6, parameters 3e-6.
tests/test_bc_soft_f64_host.py holds every case to the conditions these bars rest on.  Every workspace is pre-filled with NaN."""
import numpy as np
import pytest
import torch

import bc_soft_reference as S
import bc_update_reference as Q
import update_tail_reference as U
from bc_soft_reference import Call

pytestmark = pytest.mark.gpu

STATE = ("param", "grad", "m", "v", "step", "metrics")
NAN = float("nan")
sid = lambda s: f"B{s[0]}-D{s[1]}-A{s[2]}"


def _np(t):
    return t.cpu().double().numpy()


def _soft(c, soft=None, idx=None, targets=True, vf=S.VF, ec=S.EC, apply=0, max_norm=S.BC_MAX_NORM, ws_fill=NAN, call=None):
    """one pc_bc_minibatch_soft call on the case's first minibatch (or `idx`), with the case's soft table (or `soft`, a device tensor)"""
    call = Call(c["p0"].cuda(), c["B"], c["D"], c["A"], max_norm=max_norm, ec=ec, ws_fill=ws_fill) if call is None else call
    ix = (c["idx"][0] if idx is None else idx).cuda()
    rows = c["soft"].cuda().contiguous() if soft is None else soft
    return S.soft_call(call, ix, c["obs"].cuda().contiguous(), rows, c["target"].cuda().contiguous() if targets else None, vf=vf, ec=ec, apply=apply)


def _metrics_hold(got, ref):
    for a, b, key in zip(got, ref, ("ce", "value_loss", "entropy", "loss")):
        assert float(a) == pytest.approx(float(b), rel=S.MET_REL, abs=S.MET_ABS), key


def _same(a, b, keys=STATE):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k      # (bits: NaN would equal NaN, -0 would differ from +0)


@pytest.mark.parametrize("shape,scale,steps,max_norm", S.ONE_STEP, ids=S.ids(S.ONE_STEP))
def test_gradient_and_metrics_against_float64(shape, scale, steps, max_norm):
    """apply = 0 against bc_soft_loss in float64; param, the moments and step stay as they were."""
    c = S.case(*shape, scale)
    r = c["ref"][0]
    call = _soft(c)
    g, m = _np(call.grad), _np(call.metrics)
    print(f"{sid(shape)} scale={scale:g}: worst error / allowance = {S.worst(g, r['grad']):.3f}; metrics {m} reference {r['metrics']} "
          f"({S.metric_worst(m, r['metrics']):.3f} of the bar)")
    assert np.allclose(g, r["grad"], rtol=S.GRAD_RTOL, atol=S.GRAD_ATOL)
    _metrics_hold(m, r["metrics"])
    assert torch.equal(call.param.cpu(), c["p0"]) and float(call.step) == 0.0 and not call.m.any() and not call.v.any()


@pytest.mark.parametrize("shape,scale,steps,max_norm", S.MULTI, ids=S.ids(S.MULTI))
def test_four_applied_steps_against_float64(shape, scale, steps, max_norm):
    """Four apply = 1 steps on four minibatches, the norm clip acting and idle, after every step: param at 3e-6, grad = the clipped
    gradient at the gradient's allowance, step, the metric increments, and the moments at tests/test_bc_update_f64_gpu.py's bars."""
    c = S.case(*shape, scale, steps, max_norm)
    call = Call(c["p0"].cuda(), *shape, max_norm=max_norm, ws_fill=NAN)
    met = np.zeros(4)
    am, av = 0.0, 0.0
    for t, r in enumerate(c["ref"]):
        assert (r["norm"] > max_norm) == (max_norm == S.BC_MAX_NORM)
        _soft(c, idx=c["idx"][t], apply=1, call=call)
        p, g, m = _np(call.param), _np(call.grad), _np(call.metrics)
        a1, a2 = U.moment_allowances(r["grad_clipped"])
        am, av = 0.9 * am + a1, 0.999 * av + a2
        wm, wv = float((np.abs(_np(call.m) - r["exp_avg"]) / am).max()), float((np.abs(_np(call.v) - r["exp_avg_sq"]) / av).max())
        print(f"{sid(shape)} max_norm {max_norm:g} step {t + 1}: parameters max abs err {np.abs(p - r['param']).max():.3e}; clipped gradient "
              f"worst error / allowance {S.worst(g, r['grad_clipped']):.3f}; exp_avg {wm:.3f}, exp_avg_sq {wv:.3f} of their bars")
        assert np.abs(p - r["param"]).max() <= S.PARAM_ATOL
        assert float(call.step) == t + 1.0
        assert np.allclose(g, r["grad_clipped"], rtol=S.GRAD_RTOL, atol=S.GRAD_ATOL)
        assert wm <= 1.0 and wv <= 1.0
        _metrics_hold(m - met, r["metrics"])
        met = m


def _actor_at_plus_zero(call, D, A):
    o = S.actor_end(D, A)
    assert not call.grad[:o].view(torch.int32).any()      # (all bits clear: +0.0f)
    assert not call.metrics[[0, 2]].view(torch.int32).any()


@pytest.mark.parametrize("shape", S.ONE_ACTION, ids=sid)
def test_one_action_leaves_the_actor_exactly_at_rest(shape):
    c = S.case(*shape)
    call = _soft(c)
    _actor_at_plus_zero(call, *shape[1:])
    o = S.actor_end(*shape[1:])
    assert np.allclose(_np(call.grad)[o:], c["ref"][0]["grad"][o:], rtol=S.GRAD_RTOL, atol=S.GRAD_ATOL)


@pytest.mark.parametrize("shape", [(9, 39, 9), (257, 39, 9), (65, 25, 2), (1023, 40, 15)], ids=sid)
def test_an_all_zero_minibatch_leaves_the_actor_exactly_at_rest(shape):
    """every row zero, and every row NaN: no label anywhere -- +0.0f in every element of the actor's gradient, ce and ent exactly 0; the
    critic's slices are the case's"""
    c = S.case(*shape)
    o = S.actor_end(*shape[1:])
    ref = _soft(c)
    for fill in (0.0, NAN):
        call = _soft(c, soft=torch.full_like(c["soft"], fill).cuda())
        _actor_at_plus_zero(call, *shape[1:])
        assert torch.equal(call.grad[o:].view(torch.int32), ref.grad[o:].view(torch.int32))


@pytest.mark.parametrize("shape", [(9, 39, 9), (65, 25, 2)], ids=sid)
def test_without_targets_the_critic_rests_at_plus_zero(shape):
    c = S.case(*shape)
    o = S.actor_end(*shape[1:])
    none, zero = _soft(c, targets=False, vf=0.0), _soft(c, vf=0.0)
    assert torch.equal(none.grad[:o].view(torch.int32), zero.grad[:o].view(torch.int32))
    assert not none.grad[o:].view(torch.int32).any()
    assert not none.metrics[1].view(torch.int32).any() and float(zero.metrics[1]) > 0.0
    call = Call(c["p0"].cuda(), *shape)
    rc = S._capi.lib.pc_bc_minibatch_soft(0, c["idx"][0].cuda().data_ptr(), call.B, call.D, 256, call.A, c["obs"].cuda().data_ptr(),
                                          c["soft"].cuda().data_ptr(), None, *call._state(), 0.5, S.EC, call.max_norm, 0.9, 0.999, 1e-5,
                                          call.metrics.data_ptr(), call.ws.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    assert rc == S._capi.PC_ERR_INVALID_ARG


@pytest.mark.parametrize("shape", S.ONE_HOT_SHAPES, ids=sid)
def test_one_hot_rows_give_the_hard_step_bit_for_bit(shape):
    """soft = one_hot(label), zero rows where the label is outside 0 .. A - 1: apply = 0's gradient and metrics are pc_bc_minibatch's
    bits, and after one apply = 1 so are param, exp_avg and exp_avg_sq."""
    c = Q.case(*shape)
    B, D, A = shape
    lab = c["label"]
    assert A == 1 or (bool(((lab >= 0) & (lab < A)).any()) and bool((lab < 0).any()))
    rows = S.one_hot(lab, A).cuda()
    ix, obs, target = c["idx"][0].cuda(), c["obs"].cuda().contiguous(), c["target"].cuda().contiguous()
    for apply in (0, 1):
        hard = Call(c["p0"].cuda(), B, D, A, max_norm=S.BC_MAX_NORM, ws_fill=NAN).bc(ix, obs, lab.cuda(), target, apply=apply)
        soft = S.soft_call(Call(c["p0"].cuda(), B, D, A, max_norm=S.BC_MAX_NORM, ws_fill=NAN), ix, obs, rows, target, apply=apply)
        _same(soft, hard)
        assert apply == 0 or not torch.equal(soft.param.cpu(), c["p0"])


@pytest.mark.parametrize("shape", [(9, 39, 9), (1023, 40, 15), (65, 25, 2)], ids=sid)
def test_the_same_bits_again_whatever_the_workspace_and_the_alignment(shape):
    c = S.case(*shape)
    first = _soft(c)
    _same(_soft(c), first)
    _same(_soft(c, ws_fill=0.0), first)
    whole = torch.zeros(c["soft"].numel() + 8, device="cuda")
    off = next(o for o in range(1, 5) if (whole.data_ptr() + 4 * o) % 16 == 4)      # 4 bytes past a 16-byte boundary
    moved = whole[off:off + c["soft"].numel()].view_as(c["soft"])
    moved.copy_(c["soft"])
    assert moved.data_ptr() % 16 == 4
    _same(_soft(c, soft=moved), first)
