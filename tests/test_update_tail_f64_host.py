"""The inputs of tests/test_update_tail_f64_gpu.py held to their conditions on the CPU, and the refusals of pc_ppo_gather, pc_ppo_loss,
pc_clip_adam and pc_clip_adam_advanced that come before any device call.  The conditions make the GPU file's bars mean something:
(a) no ratio sits on a clip edge, (b) float32 torch on the CPU keeps half of every allowance, (c) one dropped sample or one inverted
clip decision is 10 x the allowance away, (d) so is each wrong clip + Adam answer, (e) no gradient element is a float32 denormal.  No
case is excluded: a seed that breaks a condition is changed in update_tail_reference's table.  No GPU needed.

The seed table is update_tail_reference.LOSS_SEEDS (five K7 cases off their default seed, each with the condition the default broke)
and ppo_update_reference.SEEDS[(1024, 40, 16)].  The figures this file prints at those seeds, float32 torch on the CPU against float64:
  (a) smallest distance of a ratio from a clip edge: 3.1e-5 at s = 1 ((1023, 9)), 1.7e-4 at s = 30 ((1024, 16))
  (b) K7, s = 1, worst error / allowance over dlogits and dvalues | over the metric sums:
      (2, 1) 0.000 | 0.258   (3, 9) 0.003 | 0.076   (63, 2) 0.025 | 0.052   (64, 16) 0.004 | 0.017   (65, 9) 0.093 | 0.184
      (255, 15) 0.404 | 0.288   (257, 16) 0.105 | 0.097   (1023, 9) 0.279 | 0.097   (1024, 16) 0.405 | 0.071   (1024, 1) 0.000 | 0.089
      constant advantages (64, 16) 0.002 | 0.003, (1024, 16) 0.002 | 0.013
      s = 30, against the same allowance (printed, not asserted: the GPU file takes `saturated_allowance` there):
      (3, 9) 0.036 | 0.066   (65, 9) 0.067 | 0.143   (257, 16) 0.298 | 0.027   (1024, 16) 0.690 | 0.236
  (c) the last sample dropped: 4.6e3 x the allowance at the least; one clip decision inverted: 3.8e3 x at the least (s = 30,
      (1024, 16)); A = 1 and constant advantages: no clip decision reaches an output, held exactly instead
  (b') K8 / K12m over all n, starts and max_norm: parameters and the clipped gradient 0.018 of their bars at the most, exp_avg 0.0053,
      exp_avg_sq 0.027
  (d) the spike left out of the norm: 2.5e4 x the bar of exp_avg[k] / exp_avg_sq[k] at the least over every k, at both n;
      the counter off by one at step0 = 0: 25.6 x on the parameters at every n;
      grad_scale ignored: 7.1e3 x (W = 2) and 1.5e5 x (W = 8) at the least with the clip idle -- with the clip acting the coefficient
      renormalises the bucket and the answer is right but for the + 1e-6 (0.002 x the bars): dropped there;
      the + 1e-6 omitted at max_norm 0.5: 0.0025 x the bars at the most (2.5e-7 relative against bars of 2e-4 relative) -- no input
      of norm 2 can show it at these bars: dropped (printed)."""
import numpy as np
import pytest
import torch

import ppo_update_reference as R
import update_tail_reference as U
from ppo_car_amd import _capi

INV, UNS, NODEV = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_UNSUPPORTED, _capi.PC_ERR_NO_DEVICE
P = 4096      # a non-NULL address, never dereferenced: every refusal below comes before any device call
lib = _capi.lib
LOSS_ALL = ([(B, A, 1.0, None) for B, A in U.LOSS_CASES] + [(B, A, U.SAT, None) for B, A in U.LOSS_SATURATED]
            + [(B, A, 1.0, 0.5) for B, A in U.LOSS_CONST_ADV])
lid = lambda c: f"B{c[0]}-A{c[1]}-s{c[2]:g}" + ("-const" if c[3] is not None else "")
ARGS = ("logits", "values", "act", "old_lp", "adv", "ret")


# ---- K7 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LOSS_ALL, ids=lid)
def test_no_ratio_near_a_clip_edge(case):
    """(a) in float64 every ratio is at least 1e-5 from 1 - clip and 1 + clip; at s = 30, where a float32 log-prob of magnitude 100 is
    good to a few 1e-6 only, 1e-4"""
    r = U.loss_case(*case)["ref"]["ratio"]
    d = float(np.minimum(np.abs(r - (1.0 - U.CLIP)), np.abs(r - (1.0 + U.CLIP))).min())
    print(f"smallest distance of a ratio from a clip edge: {d:.3e}")
    assert d >= (1e-4 if case[2] == U.SAT else 1e-5)


@pytest.mark.parametrize("case", [c for c in LOSS_ALL if c[0] >= 63 and c[1] > 1 and c[3] is None], ids=lid)
def test_every_branch_is_taken(case):
    """ratio below, inside, above the clip range x normalised advantage of either sign: all six from B = 63 on (the hand-made rows)"""
    r = U.loss_case(*case)["ref"]
    side = np.where(r["ratio"] < 1.0 - U.CLIP, 0, np.where(r["ratio"] > 1.0 + U.CLIP, 2, 1))
    assert len({(int(s), bool(a > 0)) for s, a in zip(side, r["adv_n"])}) == 6


def test_actions_reach_both_ends():
    for B, A in U.LOSS_CASES:
        act = U.loss_inputs(B, A)["act"]
        assert act[0] == 0 and act[1] == A - 1 and 0 <= act.min() and act.max() == A - 1


@pytest.mark.parametrize("case", LOSS_ALL, ids=lid)
def test_float32_torch_against_float64_on_the_loss(case):
    """(b) at s = 1 float32 torch on the CPU keeps half the allowance GRAD_ATOL / B + GRAD_RTOL |ref| on dlogits and dvalues and half
    the metric sums'.  At s = 30 its miss of that allowance is printed; it keeps 0.75 of the metric sums'."""
    c = U.loss_case(*case)
    r, r32, B = c["ref"], c["r32"], case[0]
    w = max(float((np.abs(r32[k] - r[k]) / (U.GRAD_ATOL / B + U.GRAD_RTOL * np.abs(r[k]))).max()) for k in ("dlogits", "dvalues"))
    wm = float((np.abs(r32["metrics"] - r["metrics"]) / (U.MET_ABS + U.MET_REL * np.abs(r["metrics"]))).max())
    print(f"float32 torch: dlogits / dvalues worst error / allowance {w:.3f}, metric sums {wm:.3f}")
    if case[2] == U.SAT:
        assert wm <= 0.75
    else:
        assert w <= 0.5 and wm <= 0.5


@pytest.mark.parametrize("case", LOSS_ALL, ids=lid)
def test_a_single_wrong_sample_is_far_outside_the_loss_allowance(case):
    """(c) in float64: the last sample dropped, and one out-of-range sample's clip decision inverted, each miss the GPU file's allowance
    by 10 x or more in some element of dlogits / dvalues"""
    c = U.loss_case(*case)
    r, allow = c["ref"], U.loss_allowances(c)
    dropped, flipped = U.loss_wrong_answers(c)
    miss = lambda x: max(float((np.abs(x[k] - r[k]) / a).max()) for k, a in zip(("dlogits", "dvalues"), allow))
    wd = miss(dropped)
    print(f"the last sample dropped: {wd:.1f} x the allowance")
    assert wd >= 10.0
    if case[1] == 1:          # one action: the log-prob is the constant 0 and no clip decision reaches an output
        assert flipped is None or (np.array_equal(flipped["dlogits"], r["dlogits"]) and not r["dlogits"].any())
    elif case[3] is not None:  # constant advantages: the normalised advantage is 0 and either branch gives 0
        assert not r["adv_n"].any() and r["metrics"][0] == 0.0
        assert flipped is None or np.array_equal(flipped["dlogits"], r["dlogits"])
    else:
        assert flipped is not None, "the case holds no sample outside the clip range: change its seed"
        wf = miss(flipped)
        print(f"one clip decision inverted: {wf:.1f} x")
        assert wf >= 10.0


def test_loss_on_outputs_is_ppo_loss():
    """the restatement on the outputs of a real agent gives ppo_loss's gradient w.r.t. those outputs and its four values"""
    from ppo_car_amd.ppo import ppo_loss
    c = R.case(65, 25, 2)
    a = R._agent_as(c, torch.float64)
    ix = c["idx"][0]
    obs, act, old_lp, adv, ret = (c[k][ix].double() for k in ("obs", "act", "old_lp", "adv", "ret"))
    logits, values = a.actor(obs), a.critic(obs).view(-1)
    loss, pl, vl, en = ppo_loss(a, obs, act, old_lp, adv, ret, U.CLIP, U.VF, U.EC)
    gl, gv = torch.autograd.grad(loss, [a.actor[2].bias, a.critic[2].bias])      # = the column sums of dlogits, the sum of dvalues
    got = U.loss_on_outputs(logits, values, act, old_lp, adv, ret)
    assert np.allclose(got["dlogits"].sum(0), gl.numpy(), rtol=1e-12, atol=1e-15) and np.allclose(got["dvalues"].sum(), gv.numpy(), rtol=1e-12, atol=1e-15)
    assert np.allclose(got["metrics"], [float(t.detach()) for t in (pl, vl, en, loss)], rtol=1e-13, atol=0)


# ---- K8 / K12m ----------------------------------------------------------------------------------------------------------------------
ALL_N = sorted(set(U.K8_N + U.K12M_N))


def test_clip_adam_steps_is_clip_grad_norm_and_adam():
    c = U.adam_inputs(257)
    p = torch.nn.Parameter(c["p"].double().clone())
    opt = torch.optim.Adam([p], lr=U.LR, eps=U.EPS)
    ours = U.clip_adam_steps(c["p"], c["m"], c["v"], 0, c["grads"], 0.5, 0.5)
    for g, r in zip(c["grads"], ours):
        p.grad = g.double() * 0.5
        torch.nn.utils.clip_grad_norm_([p], 0.5)
        assert np.allclose(p.grad.numpy(), r["grad_clipped"], rtol=1e-13, atol=0)
        opt.step()
        assert np.allclose(p.detach().numpy(), r["param"], rtol=0, atol=1e-14)
        assert np.allclose(opt.state[p]["exp_avg"].numpy(), r["exp_avg"], rtol=1e-12, atol=1e-16)
        assert np.allclose(opt.state[p]["exp_avg_sq"].numpy(), r["exp_avg_sq"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("n", ALL_N)
def test_gradients_and_buckets(n):
    """(e) every gradient element is 0 or at least 1e-30 in magnitude (so that W g, its product with 1 / W and their squares round as
    g's do: the power-of-two invariant); W g is exact; the norms are 2 .. 2.6, so the clip acts at 0.5 at every W and never at 1e9"""
    for step0 in U.STARTS:
        c = U.adam_inputs(n, step0)
        for g in c["grads"]:
            a = g.abs()
            assert bool(((a == 0) | (a >= 1e-30)).all()) and bool(torch.isfinite(g).all())
            assert 1.9 <= float(g.double().norm()) <= 2.7
            for W in U.WORLDS:
                assert torch.equal((g * W) * (1.0 / W), g)
        if step0:
            assert c["m"].abs().max() > 0 and c["v"].abs().max() > 0
    for mn in U.NORMS:
        for r in U.adam_case(n, 0, mn):
            assert (r["norm"] > mn) == (mn == 0.5)


@pytest.mark.parametrize("n", ALL_N)
def test_float32_torch_against_float64_on_clip_adam(n):
    """(b') float32 torch on the CPU keeps half of every bar of the GPU file at every cell and step"""
    w = np.zeros(3)
    for step0 in U.STARTS:
        for mn in U.NORMS:
            for r, r32 in zip(U.adam_case(n, step0, mn), U.adam_case(n, step0, mn, torch.float32)):
                w = np.maximum(w, U.adam_worst((r32["param"], r32["exp_avg"], r32["exp_avg_sq"]), r))
                w = np.maximum(w, [U.worst(r32["grad_clipped"], r["grad_clipped"]), 0, 0])
    print(f"n={n}: float32 torch worst error / bar: parameters (and the clipped gradient) {w[0]:.3f}, exp_avg {w[1]:.4f}, exp_avg_sq {w[2]:.4f}")
    assert (w <= 0.5).all()


def _miss(wrong, r):
    return max(U.adam_worst((wrong["param"], wrong["exp_avg"], wrong["exp_avg_sq"]), r))


@pytest.mark.parametrize("n", ALL_N)
def test_wrong_clip_adam_answers_are_far_outside_the_bars(n):
    """(d) in float64, first step: grad_scale ignored (clip idle; with the clip acting the coefficient renormalises the bucket: not a
    wrong answer these bars can see, printed) and the counter off by one at step0 = 0 each miss a bar by 10 x or more; the + 1e-6
    left out at max_norm 0.5 cannot (printed)."""
    c = U.adam_inputs(n, 0)
    for W in (2, 8):
        bucket = [g * W for g in c["grads"]]
        for mn in U.NORMS:
            r = U.adam_case(n, 0, mn)[0]
            w = _miss(U.clip_adam_steps(c["p"], c["m"], c["v"], 0, bucket[:1], mn, 1.0)[0], r)
            print(f"n={n} W={W} max_norm={mn:g}: grad_scale ignored {w:.3g} x")
            assert w >= 10.0 or mn == 0.5
    for mn in U.NORMS:
        r = U.adam_case(n, 0, mn)[0]
        w = _miss(U.clip_adam_steps(c["p"], c["m"], c["v"], 1, c["grads"][:1], mn, 1.0)[0], r)
        print(f"n={n} max_norm={mn:g}: the counter off by one {w:.3g} x")
        assert w >= 10.0
    w = _miss(U.clip_adam_steps(c["p"], c["m"], c["v"], 0, c["grads"][:1], 0.5, 1.0, norm_eps=0.0)[0], U.adam_case(n, 0, 0.5)[0])
    print(f"n={n}: the + 1e-6 left out {w:.3g} x")


@pytest.mark.parametrize("n", U.PROBE_N)
def test_a_spike_left_out_of_the_norm_is_far_outside_the_bars(n):
    """(d) the norm probes: without the spike the norm is 0.15 and the clip idle, with it 3.0: exp_avg[k], exp_avg_sq[k] miss by 10 x"""
    p, z = U.probe_params(n), torch.zeros(n)
    ks = U.probe_positions(n)
    assert ks[:5] == [0, 3, 4, 1023, 1024] and ks[-(n % 4) - 1:] == list(range(4 * (n // 4) - 1, n)) and n % 4
    worst = np.inf
    for k in ks:
        b = U.probe_bucket(n, k)
        r = U.clip_adam_steps(p, z, z, 0, [b], 0.5, 1.0)[0]
        wrong = U.clip_adam_steps(p, z, z, 0, [b], 0.5, 1.0, norm_skip=k)[0]
        am, av = U.moment_allowances(r["grad_clipped"])
        assert 3.0 < r["norm"] < 3.01
        worst = min(worst, abs(wrong["exp_avg"][k] - r["exp_avg"][k]) / am[k], abs(wrong["exp_avg_sq"][k] - r["exp_avg_sq"][k]) / av[k])
    print(f"n={n}: the spike left out of the norm misses exp_avg[k] / exp_avg_sq[k] by {worst:.3g} x at the least")
    assert worst >= 10.0


# ---- the cases of pc_ppo_minibatch the GPU file adds ----------------------------------------------------------------------------------
LEARNER = [(2, 23, 9), (65, 25, 2), (1024, 40, 16), (9, 39, 9), (256, 23, 9)]


@pytest.mark.parametrize("shape", LEARNER, ids=lambda s: f"B{s[0]}-D{s[1]}-A{s[2]}")
@pytest.mark.parametrize("max_norm", [0.5, 1e9])
def test_the_learner_cases_hold_the_conditions(shape, max_norm):
    """four steps: no ratio within 1e-5 of a clip edge along the float64 trajectory, and the norm clip acts at 0.5 alone"""
    c = R.case(*shape, 1.0, 4, max_norm)
    d = min(float(np.minimum(np.abs(r["ratio"] - 0.8), np.abs(r["ratio"] - 1.2)).min()) for r in c["ref"])
    print(f"smallest distance of a ratio from a clip edge {d:.3e}; norms {[round(r['norm'], 3) for r in c['ref']]}")
    assert d >= 1e-5
    for r in c["ref"]:
        assert (r["norm"] > max_norm) == (max_norm == 0.5)


@pytest.mark.parametrize("W", [2, 8])
def test_the_summed_ranks_case_holds_the_conditions(W):
    c = R.case(*U_RANKS, 1.0, W)
    grads = [R.gradient_of(dict(c, idx=[ix])) for ix in c["idx"]]
    a = R._agent_as(c, torch.float64)
    with torch.no_grad():
        for ix in c["idx"]:
            lp = torch.log_softmax(a.actor(c["obs"][ix].double()), -1).gather(1, c["act"][ix].long().view(-1, 1)).view(-1)
            ratio = torch.exp(lp - c["old_lp"][ix].double()).numpy()
            assert np.minimum(np.abs(ratio - 0.8), np.abs(ratio - 1.2)).min() >= 1e-5
    norm = float(np.linalg.norm(np.mean(grads, 0)))
    print(f"W={W}: norm of the mean gradient {norm:.3f}")
    assert norm > 0.5 and not np.array_equal(grads[0], grads[1])


U_RANKS = (256, 23, 9)


# ---- refusals before any device call --------------------------------------------------------------------------------------------------
def _gather(device=0, B=64, D=23, ptrs=None):
    return lib.pc_ppo_gather(device, (ptrs or [P] * 11)[0], B, D, *(ptrs or [P] * 11)[1:], None)


def _loss(device=0, B=64, A=9, ptrs=None):
    p = ptrs or [P] * 9
    return lib.pc_ppo_loss(device, *p[:6], B, A, U.CLIP, U.VF, U.EC, *p[6:], None)


def _adam(fn, device=0, n=1000, ptrs=None):
    return fn(device, *(ptrs or [P] * 6), n, 0.5, 1.0, U.BETA1, U.BETA2, U.EPS, None)


def test_null_pointers_are_refused():
    for call, count in ((_gather, 11), (_loss, 9), (lambda **kw: _adam(lib.pc_clip_adam, **kw), 6),
                        (lambda **kw: _adam(lib.pc_clip_adam_advanced, **kw), 6)):
        for i in range(count):
            ptrs = [P] * count
            ptrs[i] = None
            for device in (0, -1):
                assert call(device=device, ptrs=ptrs) == INV, (count, i, device)


def test_shapes_outside_the_limits_are_refused():
    for device in (0, -1):      # (the shape is looked at before the device)
        for kw in (dict(B=1), dict(B=1025), dict(A=0), dict(A=17)):
            assert _loss(device=device, **kw) == UNS, kw
        for fn in (lib.pc_clip_adam, lib.pc_clip_adam_advanced):
            assert _adam(fn, device=device, n=0) == INV and _adam(fn, device=device, n=(1 << 26) + 1) == INV
        assert _gather(device=device, B=0) == INV and _gather(device=device, D=0) == INV


def test_device_minus_one_is_no_device():
    """valid arguments at the limits of the shapes, device -1: PC_ERR_NO_DEVICE with or without a GPU in the machine"""
    assert _gather(device=-1) == NODEV and _gather(device=-1, B=1, D=1) == NODEV
    assert _loss(device=-1, B=2, A=1) == NODEV and _loss(device=-1, B=1024, A=16) == NODEV
    for fn in (lib.pc_clip_adam, lib.pc_clip_adam_advanced):
        assert _adam(fn, device=-1, n=1) == NODEV and _adam(fn, device=-1, n=1 << 26) == NODEV
