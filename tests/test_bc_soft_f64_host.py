"""The soft-target imitation step without a GPU: the input conditions of every case tests/test_bc_soft_f64_gpu.py runs against float64
(none excluded), the limits and NULL checks of pc_bc_minibatch_soft before the device, and bc_soft_loss against bc_loss on one-hot rows.

Conditions per case: float32 torch on the CPU stays within 0.5 of the gradient and metric allowances (the bars can be met in float32);
the float64 gradient with the last sample dropped is more than 20 x the allowance away in an actor slice; so is the one with the last
sample's soft row replaced by its arg-max one-hot, wherever A >= 2 and that row is soft (B mod 8 != 0 by construction)."""
import numpy as np
import pytest
import torch

import bc_soft_reference as S
import bc_update_reference as Q
from ppo_car_amd import Agent, _capi, bc_soft_loss
from ppo_car_amd.imitation import bc_loss

INV, UNS, NODEV = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_UNSUPPORTED, _capi.PC_ERR_NO_DEVICE
CASES = S.ONE_STEP + S.MULTI
P = 4096      # a non-NULL, 16-byte aligned address that is never dereferenced before the device check


def _actor_worst(g, gref, D, A):
    by = S.worst_by_slice(g, gref, D, A)
    return max(v for k, v in by.items() if k.startswith("actor"))


@pytest.mark.parametrize("shape,scale,steps,max_norm", CASES, ids=S.ids(CASES))
def test_input_conditions(shape, scale, steps, max_norm):
    c = S.case(*shape, scale, steps, max_norm)
    r32 = S.restated32(*shape, scale, steps, max_norm)
    B, D, A = shape
    for t, (r, q) in enumerate(zip(c["ref"], r32)):
        wg, wm = S.worst(q["grad"], r["grad"]), S.metric_worst(q["metrics"], r["metrics"])
        print(f"step {t}: float32 torch {wg:.3f} of the gradient allowance, {wm:.3f} of the metrics'; float64 norm {r['norm']:.3f}")
        assert wg <= 0.5 and wm <= 0.5
        if steps > 1:
            assert (r["norm"] > max_norm) == (max_norm == S.BC_MAX_NORM)
    own = S.gradient_of(c)
    g = c["ref"][0]["grad"]
    assert np.abs(own - g).max() <= 1e-12 * max(1.0, np.abs(g).max())      # the per-sample restatement is bc_soft_loss
    if B % 8 != 0 and A >= 2:
        assert S.last_row_is_soft(c)
    dropped, hardened = S.wrong_gradients(c)
    if A >= 2:      # (A = 1: log_softmax is the constant 0, the actor rests whatever the row)
        wd = _actor_worst(dropped, g, D, A)
        print(f"the last sample dropped: {wd:.1f} x the allowance in an actor slice")
        assert wd > 20.0
    if hardened is not None:
        wh = _actor_worst(hardened, g, D, A)
        print(f"the last sample's row hardened: {wh:.1f} x the allowance in an actor slice")
        assert wh > 20.0


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: f"B{s[0]}-D{s[1]}-A{s[2]}")
def test_the_hand_placed_rows(shape):
    c = S.inputs(*shape)
    B, D, A = shape
    p = c["soft"][c["idx"][0]]
    assert not p[0].any()
    if B > 2:
        assert float(p[1, A - 1]) == 1.0 and float(p[1].sum()) == 1.0
    if B >= 7:
        assert torch.equal(p[2], p[3]) and float(p[2].sum()) > 0.99
        assert abs(float(p[4].sum()) - 0.5) < 1e-6
        if B % 8 >= 2:
            assert not p[B - 2].any() and p[B - 1].any()
    assert (c["soft"] >= 0).all() and (c["soft"].sum(-1) <= 1.0 + 1e-6).all()


@pytest.mark.parametrize("B,D,A", [(2, 23, 9), (9, 39, 9), (65, 25, 2), (33, 40, 1), (64, 24, 15)])
def test_one_hot_rows_give_bc_loss(B, D, A):
    c = Q.inputs(B, D, A)
    a = Q._agent_as(c, torch.float64)
    ix = c["idx"][0]
    obs, label, target = c["obs"][ix].double(), c["label"][ix], c["target"][ix].double()
    hard = bc_loss(a, obs, label.double(), target, S.VF, S.EC)
    soft = bc_soft_loss(a, obs, S.one_hot(label, A).double(), target, S.VF, S.EC)
    for h, s in zip(hard, soft):
        assert abs(float(h.detach()) - float(s.detach())) <= 1e-15
    nan = S.one_hot(label, A).double()
    nan[0] = float("nan")      # a NaN row is "no label"
    label = label.clone()
    label[0] = -1.0
    for h, s in zip(bc_loss(a, obs, label.double(), target, S.VF, S.EC), bc_soft_loss(a, obs, nan, target, S.VF, S.EC)):
        assert abs(float(h.detach()) - float(s.detach())) <= 1e-15


def _soft(device=-1, idx=P, B=64, D=23, H=256, A=9, obs=P, soft=P, target=P, param=P, grad=P, state=(P,) * 4, vf=0.5, metrics=P, ws=P, apply=1):
    return _capi.lib.pc_bc_minibatch_soft(device, idx, B, D, H, A, obs, soft, target, param, grad, *state, vf, 0.01, 0.5, 0.9, 0.999, 1e-5, metrics,
                                          ws, apply, None)


@pytest.mark.parametrize("kw", [dict(B=1), dict(B=1025), dict(A=0), dict(A=16), dict(D=0), dict(D=41), dict(H=255)])
def test_limits_before_the_device(kw):
    assert _soft(**kw) == UNS


@pytest.mark.parametrize("kw", [dict(obs=None), dict(soft=None), dict(param=None), dict(ws=None), dict(idx=None), dict(grad=None),
                                dict(metrics=None), dict(target=None, vf=0.5), dict(apply=3), dict(apply=-1), dict(state=(None, P, P, P)),
                                dict(apply=2, state=(P, P, None, P)), dict(param=P + 4), dict(ws=P + 8)])
def test_null_and_alignment_checks(kw):
    assert _soft(**kw) == INV


def test_no_device():
    assert _soft() == NODEV and _soft(target=None, vf=0.0) == NODEV and _soft(soft=P + 4) == NODEV
