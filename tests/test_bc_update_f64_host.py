"""The inputs of tests/test_bc_update_f64_gpu.py held to their conditions on the CPU, and the refusals of pc_bc_minibatch that
tests/test_imitation_host.py does not have.  The conditions are what makes the GPU file's tolerances mean something: torch's own float32
keeps half the allowance (the kernel gets a factor of two over it), each of four wrong heads -- the last sample lost, the divisor the
number of labelled samples, an unlabelled sample taken as label 0, a label off by one -- is more than 20 x the allowance away (the
tolerance cannot hide one), the first minibatch holds the labels and rows it is said to hold, the norm clip acts in one setting and
rests in the other, and every label value at an edge of "labelled" gives float64 bc_loss exactly what its stated whole label gives.  No
case is skipped or excluded: a seed that breaks a condition is changed in bc_update_reference's case table.  No GPU needed."""
import numpy as np
import pytest
import torch

import bc_update_reference as Q
from ppo_car_amd import _capi
from ppo_car_amd.imitation import bc_loss

INV, UNS = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_UNSUPPORTED
P = 4096      # a non-NULL, 16-byte aligned address, never dereferenced: every refusal below comes before any device call
ONE_STEP, SATURATED_CASES, AGREEING, MULTI = Q.ONE_STEP, Q.SATURATED_CASES, Q.AGREEING, Q.MULTI
EVERY = ONE_STEP + SATURATED_CASES + AGREEING + MULTI


def test_the_case_lists_are_the_gpu_files():
    """both files take their cases from the reference module: the same objects, not equal copies"""
    import test_bc_update_f64_gpu as G
    for name in ("ONE_STEP", "SATURATED_CASES", "AGREEING", "MULTI"):
        assert getattr(G, name) is getattr(Q, name) is globals()[name], name
    for name in ("ONE_ACTION", "EDGE_SHAPES", "IGNORE_SHAPES", "SINGLE_LABEL", "SHARED", "LEARNER_B", "LABEL_EDGES"):
        assert getattr(G, name) is getattr(Q, name), name
    assert G.R.SHAPES is Q.SHAPES and G.R.ROBUST is Q.ROBUST and G.R.APPLIED is Q.APPLIED and G.R.SATURATED is Q.SATURATED
    assert [c[0] for c in ONE_STEP] == Q.SHAPES * 2 and len(Q.SHAPES) == 17
    assert all(s in Q.SHAPES for s in Q.EDGE_SHAPES + Q.IGNORE_SHAPES + Q.SINGLE_LABEL + Q.SHARED + Q.ONE_ACTION)


def _ref32(shape, scale, steps, mn, agree):
    return Q.case(*shape, scale, steps, mn, agree)["ref"], Q.restated32(*shape, scale, steps, mn, agree)


# ---- torch's own float32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale,steps,max_norm,agree", ONE_STEP + AGREEING, ids=Q.ids(ONE_STEP + AGREEING))
def test_float32_torch_keeps_half_the_allowance(shape, scale, steps, max_norm, agree):
    """Scales 1 and 40, and the agreeing-labels cases (the GPU file holds those to the standard allowance too): gradient rtol 2e-4 /
    atol 2e-7, metric sums rel 1e-5 / abs 1e-6."""
    (r64,), (r32,) = _ref32(shape, scale, steps, max_norm, agree)
    wg, wm = Q.worst(r32["grad"], r64["grad"]), Q.metric_worst(r32["metrics"], r64["metrics"])
    print(f"float32 torch: gradient worst error / allowance {wg:.3f}, metrics {wm:.3f}; by slice "
          f"{ {k: round(v, 3) for k, v in Q.worst_by_slice(r32['grad'], r64['grad'], shape[1], shape[2]).items()} }")
    assert wg <= 0.5 and wm <= 0.5


@pytest.mark.parametrize("shape,scale,steps,max_norm,agree", SATURATED_CASES, ids=Q.ids(SATURATED_CASES))
def test_float32_torch_at_the_saturated_softmax(shape, scale, steps, max_norm, agree):
    """Scale 4000: torch's float32 does not keep half of the standard gradient allowance (printed), so the GPU file holds the gradient to
    saturated_allowance(g32, g64) = 2e-4 |g64| + 4 max|g32 - g64|, a margin of four over torch's own worst element, as the PPO files do.
    The metric sums keep the project's bar and torch half of it."""
    (r64,), (r32,) = _ref32(shape, scale, steps, max_norm, agree)
    wg, wm = Q.worst(r32["grad"], r64["grad"]), Q.metric_worst(r32["metrics"], r64["metrics"])
    print(f"float32 torch: gradient worst error / the standard allowance {wg:.3f}, max|g32 - g64| {np.abs(r32['grad'] - r64['grad']).max():.3e}; metrics {wm:.3f}")
    assert wm <= 0.5


@pytest.mark.parametrize("shape,scale,steps,max_norm,agree", MULTI, ids=Q.ids(MULTI))
def test_float32_torch_over_four_steps(shape, scale, steps, max_norm, agree):
    """every step: half the parameter bar, half the clipped gradient's allowance, half the metric bars"""
    r64s, r32s = _ref32(shape, scale, steps, max_norm, agree)
    assert len(r64s) == 4
    for t, (r64, r32) in enumerate(zip(r64s, r32s)):
        wp = float(np.abs(r32["param"] - r64["param"]).max() / Q.PARAM_ATOL)
        wg, wm = Q.worst(r32["grad_clipped"], r64["grad_clipped"]), Q.metric_worst(r32["metrics"], r64["metrics"])
        print(f"step {t + 1}: float32 torch parameters {wp:.4f} of the bar, clipped gradient {wg:.3f}, metrics {wm:.3f}; norm {r64['norm']:.3f}")
        assert wp <= 0.5 and wg <= 0.5 and wm <= 0.5


@pytest.mark.parametrize("B", Q.LEARNER_B)
def test_float32_torch_on_the_learners_steps(B):
    c = Q.learner_case(B)
    n = 5 if B == 2 else 3
    assert [len(ix) for ix in c["idx"]] == [B] * n and len(set(torch.cat(c["idx"]).tolist())) == n * B and c["pool"] == 3 * B + 5 < (n + 1) * B
    for t, (r64, r32) in enumerate(zip(c["ref"], c["ref32"])):
        wp = float(np.abs(r32["param"] - r64["param"]).max() / Q.PARAM_ATOL)
        print(f"step {t + 1}: float32 torch parameters {wp:.4f} of the bar; norm {r64['norm']:.3f}")
        assert wp <= 0.5
    lab = torch.cat([c["label"][ix] for ix in c["idx"]])
    assert bool((lab == -1).any()) and bool((lab >= 0).any())


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------------
def _slices_moved(wrong, g, allow, D, A):
    """{actor, critic}: whether `wrong` is more than 20 x the allowance from g in at least one element of such a slice"""
    by = Q.worst_by_slice(wrong, g, D, A, allow)
    return max(v for k, v in by.items() if k.startswith("actor")), max(v for k, v in by.items() if k.startswith("critic"))


@pytest.mark.parametrize("shape,scale,steps,max_norm,agree", ONE_STEP + SATURATED_CASES, ids=Q.ids(ONE_STEP + SATURATED_CASES))
def test_each_wrong_head_is_far_outside_the_allowance(shape, scale, steps, max_norm, agree):
    """(a) the last sample dropped: an actor slice AND a critic slice; (b) the labelled divisor, (c) an unlabelled sample as label 0,
    (d) a label off by one: an actor slice -- each more than 20 x the case's allowance in at least one element.  One action: (b), (c),
    (d) cannot move anything (log-softmax of one logit is the constant 0) and are asserted to change nothing; (a) moves the critic."""
    c = Q.case(*shape, scale)
    g = c["ref"][0]["grad"]
    D, A = shape[1:]
    own = Q.gradient_of(c)
    assert np.abs(own - g).max() <= 1e-12 * max(1.0, np.abs(g).max())      # the per-sample restatement is bc_loss
    allow = Q.allowance(g) if scale < 4000.0 else Q.saturated_allowance(Q.restated32(*shape, scale)[0]["grad"], g) * np.ones_like(g)
    wrong = Q.wrong_gradients(c)
    moved = {k: _slices_moved(w, g, allow, D, A) for k, w in wrong.items()}
    print("worst error / allowance (actor slices, critic slices): " + "; ".join(f"({k}) {a:.0f}, {v:.0f}" for k, (a, v) in moved.items()))
    o = Q.actor_end(D, A)
    assert moved["a"][1] > 20.0
    for k in "bcd":
        assert np.array_equal(wrong[k][o:], g[o:]), k      # (none of these touches the critic)
    if A == 1:
        assert not g[:o].any()
        for k in "abcd":
            assert np.array_equal(wrong[k][:o], g[:o]), k
    else:
        for k in "abcd":
            assert moved[k][0] > 20.0, k


# ---- composition -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale,steps,max_norm,agree", ONE_STEP + SATURATED_CASES + MULTI, ids=Q.ids(ONE_STEP + SATURATED_CASES + MULTI))
def test_the_first_minibatch_holds_what_it_is_said_to_hold(shape, scale, steps, max_norm, agree):
    c = Q.case(*shape, scale, steps, max_norm)
    B, D, A = shape
    ix, lab = c["idx"][0].tolist(), Q.first_labels(c)
    assert all(len(i) == B and int(i.min()) >= 0 and int(i.max()) < c["pool"] == B + 7 for i in c["idx"]) and len(c["idx"]) == steps
    assert bool(((c["label"] >= -1) & (c["label"] <= A - 1) & (c["label"] == c["label"].round())).all())
    assert bool((lab == -1).any()) and bool((lab == A - 1).any()) and 0 in ix and B + 6 in ix
    if B >= 4:
        assert ix[:4] == [0, B + 6, 2, 2] and lab[:4].tolist() == [-1.0, A - 1.0, 0.0, 0.0] and len(set(ix)) < B
    else:
        assert ix[:2] == [0, B + 6] and lab[:2].tolist() == [-1.0, A - 1.0]
    if B % 8:
        group = lab[B - B % 8:]
        last = int(lab[B - 1])
        assert last >= 0 and bool((group >= 0).any())
        if B % 8 >= 2:                 # (one live sample: the labelled one; the other seven lanes are dead)
            assert bool((group == -1).any())
        if A > 1:                      # losing the last sample moves the actor: its label is not where its probability already is
            assert last != int(Q.logits64(c, c["idx"][0][B - 1:]).argmax(-1))


@pytest.mark.parametrize("shape,scale,steps,max_norm,agree", AGREEING, ids=Q.ids(AGREEING))
def test_agreeing_labels_and_the_two_orders_of_the_log_softmax(shape, scale, steps, max_norm, agree):
    """Every label is its row's float64 argmax, so ce is small and its rounding shows: K27 forms l_a - (max + log(sum)), torch
    (l_a - max) - log(sum).  Both are emulated in float32 here and recorded against the ce bar (rel 1e-5, abs 1e-6); torch's order keeps
    half of it.  The kernel's order rounds max + log(sum) to an ulp of the largest logit, 1.5e-5 at 160: at (8, 23, 9) x 24000 it is
    at 0.46 of the bar, torch's at 0.001."""
    c = Q.case(*shape, scale, 1, max_norm, True)
    lab = Q.first_labels(c)
    assert torch.equal(lab.long(), Q.logits64(c, c["idx"][0]).argmax(-1)) and bool(Q.is_labelled(lab, shape[2]).all())
    ce = c["ref"][0]["metrics"][0]
    bar = Q.MET_ABS + Q.MET_REL * abs(ce)
    k, t = abs(Q.ce_emulated(c, "kernel") - ce) / bar, abs(Q.ce_emulated(c, "torch") - ce) / bar
    print(f"ce {ce:.6e}: the kernel's order {k:.4f} of the bar, torch's order {t:.4f}")
    assert t <= 0.5 and k <= 1.0


# ---- the norm clip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", Q.APPLIED)
def test_the_norm_clip_acts_in_one_setting_only(shape):
    acting, idle = Q.case(*shape, 1.0, 4, Q.BC_MAX_NORM)["ref"], Q.case(*shape, 1.0, 4, Q.BC_IDLE_NORM)["ref"]
    print("float64 gradient norms: clipped run " + ", ".join(f"{r['norm']:.3f}" for r in acting) + "; idle run " + ", ".join(f"{r['norm']:.3f}" for r in idle))
    for r in acting:
        assert r["norm"] >= 1.05 * Q.BC_MAX_NORM and not np.array_equal(r["grad"], r["grad_clipped"])
    for r in idle:
        assert np.array_equal(r["grad"], r["grad_clipped"])
    for r in acting + idle:
        assert abs(r["norm"] / Q.BC_MAX_NORM - 1.0) > 0.01
    # (Adam divides the clip's factor out again but for eps: the two runs part by up to lr per step, where |g| is of eps' size)
    assert np.abs(acting[-1]["param"] - idle[-1]["param"]).max() > 100.0 * Q.PARAM_ATOL


def test_reference_is_bc_loss_clip_and_adam():
    """run_steps' first step written out: bc_loss's gradient, clip_grad_norm_'s coefficient, Adam's first step from zero moments"""
    c = Q.case(9, 39, 9, 1.0, 4, Q.BC_MAX_NORM)
    r = c["ref"][0]
    a = Q._agent_as(c, torch.float64)
    ix = c["idx"][0]
    total, ce, vl, ent = bc_loss(a, c["obs"][ix].double(), c["label"][ix].double(), c["target"][ix].double(), Q.VF, Q.EC)
    total.backward()
    g = torch.cat([p.grad.reshape(-1) for p in a.parameters()]).numpy()
    assert np.array_equal(g, r["grad"]) and np.array_equal(r["metrics"], [float(t.detach()) for t in (ce, vl, ent, total)])
    gc = g * min(1.0, Q.BC_MAX_NORM / (np.sqrt((g ** 2).sum()) + 1e-6))
    assert np.allclose(gc, r["grad_clipped"], rtol=1e-12, atol=0)
    assert np.allclose(r["exp_avg"], 0.1 * gc, rtol=1e-12, atol=0) and np.allclose(r["exp_avg_sq"], 0.001 * gc * gc, rtol=1e-12, atol=0)
    p1 = c["p0"].double().numpy() - Q.LR * (0.1 * gc / (1 - 0.9)) / (np.sqrt(0.001 * gc * gc / (1 - 0.999)) + 1e-5)
    assert np.allclose(p1, r["param"], rtol=0, atol=1e-12)


# ---- the label edges -------------------------------------------------------------------------------------------------------------------
def _bc64(c, label):
    a = Q._agent_as(c, torch.float64)
    ix = c["idx"][0]
    total, ce, vl, ent = bc_loss(a, c["obs"][ix].double(), label[ix].double(), c["target"][ix].double(), Q.VF, Q.EC)
    total.backward()
    return torch.cat([p.grad.reshape(-1) for p in a.parameters()]).numpy(), [float(t.detach()) for t in (ce, vl, ent, total)]


@pytest.mark.parametrize("shape", Q.EDGE_SHAPES)
def test_label_edges_in_float64_bc_loss(shape):
    """each value gives exactly the gradient and metrics of its stated whole label, or of -1: the table says what bc_loss says.  The
    float32 value cast to float64 is the same number, so the predicate and the truncation see what the kernel sees."""
    c = Q.case(*shape)
    A = shape[2]
    names = [n for n, _, _ in Q.LABEL_EDGES[A]]
    assert len(names) == (15 if A > 2 else 14) and ("2.5" in names) == (A > 2)
    first, last = Q.edge_samples(c)
    assert int(c["idx"][0][first]) != int(c["idx"][0][last]) and first < 8 <= last - last % 8      # two rows, the first and the last group
    for j in (first, last):
        for name, value, whole in Q.LABEL_EDGES[A]:
            assert value.dtype == np.float32 and -1 <= whole < A
            g, m = _bc64(c, Q.with_label(c, j, value))
            gw, mw = _bc64(c, Q.with_label(c, j, float(whole)))
            assert np.array_equal(g, gw) and m == mw and np.isfinite(g).all() and np.isfinite(m).all(), (name, j)
    j = Q.edge_samples(c)[1]
    if A > 1:                          # (the table is not vacuous: label 0, label A - 1 and no label are three gradients)
        g = [_bc64(c, Q.with_label(c, j, v))[0] for v in (0.0, A - 1.0, -1.0)]
        assert not np.array_equal(g[0], g[1]) and not np.array_equal(g[0], g[2]) and not np.array_equal(g[1], g[2])
    e = dict((n, v) for n, v, _ in Q.LABEL_EDGES[A])
    assert np.signbit(e["-0.0"]) and e["-0.0"] == 0 and e["nextafter(A,0)"] < A and float(e["nextafter(A,0)"]) > A - 1e-5
    assert -1.5e-45 < float(e["nextafter(0,-1)"]) < 0.0 and e["2**32+1"] == 2.0 ** 32 and np.isnan(e["nan"])


@pytest.mark.parametrize("shape", Q.SINGLE_LABEL)
def test_the_single_label_minibatch(shape):
    """one labelled sample, the last (in a partly dead group), its row nowhere else; the actor's gradient is 1 / B of that sample's
    alone and more than 20 x the allowance from zero"""
    c = Q.case(*shape)
    B, D, A = shape
    ix, lab, j = Q.single_label(c)
    on = Q.is_labelled(lab[ix], A)
    assert int(on.sum()) == 1 and bool(on[j]) and j == B - 1 and B % 8 != 0
    one = dict(c, idx=[ix], label=lab)
    g = Q.run_steps(one)[0]["grad"]
    w = np.zeros(B)
    w[j] = 1.0
    o = Q.actor_end(D, A)
    alone = Q.gradient_of(one, weight=w)
    assert np.abs(alone[:o] - g[:o]).max() <= 1e-12 * np.abs(g[:o]).max()
    assert Q.worst(g[:o], np.zeros(o)) > 20.0
    r32 = Q.run_steps(one, dtype=torch.float32)[0]
    assert Q.worst(r32["grad"], g) <= 0.5 and Q.metric_worst(r32["metrics"], Q.run_steps(one)[0]["metrics"]) <= 0.5


@pytest.mark.parametrize("shape", Q.IGNORE_SHAPES)
def test_the_minibatch_without_an_unlabelled_sample(shape):
    """the unlabelled samples replaced by copies of a labelled row: every sample labelled, the same B; far from the case's own
    gradient, and float32 torch keeps half the bars"""
    c = Q.case(*shape)
    full = dict(c, idx=[Q.all_labelled(c)])
    assert bool(Q.is_labelled(Q.first_labels(full), shape[2]).all()) and int((c["label"] == -1).sum()) >= 2
    r, r32 = Q.run_steps(full)[0], Q.run_steps(full, dtype=torch.float32)[0]
    assert Q.worst(r32["grad"], r["grad"]) <= 0.5 and Q.metric_worst(r32["metrics"], r["metrics"]) <= 0.5
    assert Q.worst(c["ref"][0]["grad"], r["grad"]) > 20.0


# ---- refusals: the documented code before any device call ------------------------------------------------------------------------------
def _bc(device=0, B=64, D=23, H=256, A=9, target=P, param=P, ws=P, vf=0.5, apply=1):
    return _capi.lib.pc_bc_minibatch(device, P, B, D, H, A, P, P, target, param, P, *(P,) * 4, vf, 0.01, 0.5, 0.9, 0.999, 1e-5, P, ws, apply, None)


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-1), dict(D=0), dict(A=0), dict(A=-1), dict(H=0)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_degenerate_shapes_are_refused(kw):
    for device in (0, -1):
        for apply in (0, 1, 2):
            assert _bc(device=device, apply=apply, **kw) == UNS
    assert _bc(target=None, vf=0.0, **kw) == UNS
    a = dict(B=64, D=23, H=256, A=9)
    a.update(kw)
    assert _capi.lib.pc_ppo_workspace_floats(a["B"], a["D"], a["H"], a["A"]) == UNS      # (the size BCLearner asks for)


@pytest.mark.parametrize("off", [4, 8, 12])
def test_param_and_workspace_off_16_byte_alignment_are_refused(off):
    for device in (0, -1):
        for apply in (0, 1, 2):
            assert _bc(device=device, apply=apply, param=P + off) == INV and _bc(device=device, apply=apply, ws=P + off) == INV
    assert _bc(param=P + off, B=0) == INV and _bc(ws=P + off, A=0) == INV      # (with the NULL checks: before the shape)
    assert _bc(device=-1, param=P + 16, ws=P + 32) == _capi.PC_ERR_NO_DEVICE


def test_no_targets_with_a_nan_value_coefficient_is_refused():
    """include/ppocar.h: target == NULL needs vf_coef == 0 -- NaN is not 0"""
    for device in (0, -1):
        for apply in (0, 1, 2):
            assert _bc(device=device, apply=apply, target=None, vf=float("nan")) == INV
    assert _bc(device=-1, target=None, vf=-0.0) == _capi.PC_ERR_NO_DEVICE      # (-0.0 is 0)


@pytest.mark.parametrize("apply", [-2, -1, 3, 4, 2 ** 31 - 1, -2 ** 31])
def test_apply_outside_0_1_2_is_refused(apply):
    """ppocar.hip's check_apply_args: PC_ERR_INVALID_ARG, before shape and device"""
    assert _bc(apply=apply) == INV and _bc(device=-1, apply=apply) == INV and _bc(apply=apply, B=0) == INV
