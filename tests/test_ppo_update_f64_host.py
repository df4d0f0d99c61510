"""The inputs of tests/test_ppo_update_f64_gpu.py held to their conditions on the CPU, and the refusals of the small-minibatch entry
points.  The conditions are what makes the GPU file's tolerances mean something: no sample sits on a clip edge (kernel and reference
take the same branch), every branch is taken, torch's own float32 keeps half the allowance (the kernel gets a factor of two over it),
and a single dropped sample or a single wrong clip decision is more than 20 x the allowance away (the tolerance cannot hide one).  No
case is skipped or excluded: a seed that breaks a condition is changed in ppo_update_reference's case table.  No GPU needed."""
import numpy as np
import pytest
import torch

import ppo_update_reference as R
from ppo_car_amd import _capi
from ppo_car_amd.ppo import ppo_loss

UNS = _capi.PC_ERR_UNSUPPORTED
P = 4096      # a non-NULL address, never dereferenced: every refusal below comes before any device call
# (shape, scale, steps, max_norm) of every case the GPU file runs against float64
ONE_STEP = [(s, scale, 1, R.MAX_NORM) for scale in (1.0, 40.0) for s in R.SHAPES] + [(s, 4000.0, 1, R.MAX_NORM) for s in R.SATURATED]
MULTI = [(s, 1.0, 4, mn) for s in R.APPLIED for mn in (0.5, 1e9)] + [(s, 1.0, 3, R.MAX_NORM) for s in R.FORMS]
ids = lambda cases: [f"B{s[0]}-D{s[1]}-A{s[2]}-x{scale:g}-n{steps}-norm{mn:g}" for s, scale, steps, mn in cases]


def _edge_distance(r):
    return float(np.minimum(np.abs(r["ratio"] - (1.0 - R.CLIP)), np.abs(r["ratio"] - (1.0 + R.CLIP))).min())


def _combos(r):
    side = np.where(r["ratio"] < 1.0 - R.CLIP, 0, np.where(r["ratio"] > 1.0 + R.CLIP, 2, 1))
    return {(int(s), bool(a > 0)) for s, a in zip(side, r["adv_n"])}


@pytest.mark.parametrize("shape,scale,steps,max_norm", ONE_STEP + MULTI, ids=ids(ONE_STEP + MULTI))
def test_no_ratio_near_a_clip_edge(shape, scale, steps, max_norm):
    """In float64 every sample's ratio is at least 1e-5 from 1 - clip and 1 + clip (a float32 ratio here is off by less than 1e-6):
    along the reference's whole trajectory where several steps are applied."""
    c = R.case(*shape, scale, steps, max_norm)
    d = min(_edge_distance(r) for r in c["ref"])
    print(f"smallest distance of a ratio from a clip edge: {d:.3e}")
    assert d >= 1e-5


WIDE = [c for c in ONE_STEP if c[0][0] >= 64]      # (the cases below 64 samples are held together, in the next test)


@pytest.mark.parametrize("shape,scale,steps,max_norm", WIDE, ids=ids(WIDE))
def test_every_branch_is_taken(shape, scale, steps, max_norm):
    """ratio below, inside and above the clip range x normalised advantage negative and positive: all six in every case from B = 64"""
    assert len(_combos(R.case(*shape, scale)["ref"][0])) == 6


@pytest.mark.parametrize("scale", [1.0, 40.0, 4000.0])
def test_the_small_hand_made_cases_take_every_branch_together(scale):
    shapes = [s for s in R.SHAPES if s[0] in (7, 8, 9) and s in R.HAND and (scale < 4000.0 or s in R.SATURATED)]
    assert len(shapes) == (3 if scale < 4000.0 else 1)
    got = set()
    for s in shapes:
        got |= _combos(R.case(*s, scale)["ref"][0])
    if scale < 4000.0:
        assert len(got) == 6, got
    else:
        assert len(got) >= 5, got      # (B = 8 alone: eight samples, rows 2 and 3 the same)


@pytest.mark.parametrize("shape,scale,steps,max_norm", ONE_STEP, ids=ids(ONE_STEP))
def test_float32_torch_against_float64(shape, scale, steps, max_norm):
    """torch's own float32 on the CPU keeps half the allowance at scale 1 and 40 (gradient: rtol 2e-4, atol 2e-7; metric sums: rel 1e-5,
    abs 1e-6).  At scale 4000 it does not hold the gradient's (printed), which is why the GPU file has another allowance there; it
    holds 0.75 of the metric sums'."""
    r64, r32 = R.case(*shape, scale)["ref"][0], R.restated32(*shape, scale)[0]
    wg = R.worst(r32["grad"], r64["grad"])
    wm = float((np.abs(r32["metrics"] - r64["metrics"]) / (R.MET_ABS + R.MET_REL * np.abs(r64["metrics"]))).max())
    print(f"float32 torch: gradient worst error / allowance {wg:.3f}, metrics {wm:.3f}; by slice {R.worst_by_slice(r32['grad'], r64['grad'], shape[1], shape[2])}")
    if scale < 4000.0:
        assert wg <= 0.5 and wm <= 0.5
    else:
        assert wm <= 0.75


@pytest.mark.parametrize("shape,scale,steps,max_norm", ONE_STEP, ids=ids(ONE_STEP))
def test_a_single_wrong_sample_is_far_outside_the_allowance(shape, scale, steps, max_norm):
    """The float64 gradient with the last sample dropped, and with the clip decision of the first out-of-range sample inverted, each
    differ from the true one by more than 20 x the allowance in at least one element (at scale 4000: 20 x that scale's allowance)."""
    c = R.case(*shape, scale)
    g = c["ref"][0]["grad"]
    own = R.gradient_of(c)
    assert np.abs(own - g).max() <= 1e-12 * max(1.0, np.abs(g).max())      # the per-sample restatement is ppo_loss
    allow = R.allowance(g) if scale < 4000.0 else R.saturated_allowance(R.restated32(*shape, scale)[0]["grad"], g)
    dropped, flipped = R.wrong_gradients(c)
    wd, wf = R.worst(dropped, g, allow), R.worst(flipped, g, allow)
    print(f"one sample dropped: {wd:.1f} x the allowance; one clip decision inverted: {wf:.1f} x")
    assert wd > 20.0
    if shape[2] == 1:      # one action: the log-prob is the constant 0 and no clip decision reaches a gradient -- held exactly on the GPU
        assert np.array_equal(flipped, g)
    else:
        assert wf > 20.0


@pytest.mark.parametrize("shape", R.APPLIED)
def test_the_norm_clip_acts_in_one_setting_only(shape):
    for r in R.case(*shape, 1.0, 4, 0.5)["ref"]:
        assert r["norm"] > 0.5 and not np.array_equal(r["grad"], r["grad_clipped"])
    for r in R.case(*shape, 1.0, 4, 1e9)["ref"]:
        assert np.array_equal(r["grad"], r["grad_clipped"])


def test_indices_repeat_and_reach_both_ends_of_the_pool():
    for s in R.SHAPES:
        c = R.inputs(*s)
        ix = c["idx"][0].tolist()
        assert len(ix) == s[0] and min(ix) >= 0 and max(ix) < c["pool"] == s[0] + 7
        if s[0] >= 4:
            assert ix[:4] == [0, c["pool"] - 1, 2, 2]


def test_reference_is_ppo_loss_clip_and_adam():
    """run_steps' first step written out: ppo_loss's gradient, clip_grad_norm_'s coefficient, Adam's first step from zero moments"""
    c = R.case(9, 39, 9, 1.0, 4, 0.5)
    r = c["ref"][0]
    a = R._agent_as(c, torch.float64)
    ix = c["idx"][0]
    loss, pl, vl, en = ppo_loss(a, *(c[k][ix].double() for k in ("obs", "act", "old_lp", "adv", "ret")), R.CLIP, R.VF, R.EC)
    loss.backward()
    g = torch.cat([p.grad.reshape(-1) for p in a.parameters()]).numpy()
    assert np.array_equal(g, r["grad"]) and np.array_equal(r["metrics"], [float(t.detach()) for t in (pl, vl, en, loss)])
    gc = g * min(1.0, 0.5 / (np.sqrt((g ** 2).sum()) + 1e-6))
    assert np.allclose(gc, r["grad_clipped"], rtol=1e-12, atol=0)
    assert np.allclose(r["exp_avg"], 0.1 * gc, rtol=1e-12, atol=0) and np.allclose(r["exp_avg_sq"], 0.001 * gc * gc, rtol=1e-12, atol=0)
    p1 = c["p0"].double().numpy() - R.LR * (0.1 * gc / (1 - 0.9)) / (np.sqrt(0.001 * gc * gc / (1 - 0.999)) + 1e-5)
    assert np.allclose(p1, r["param"], rtol=0, atol=1e-12)


# ---- refusals: the documented code before any device call ------------------------------------------------------------------------
BAD = [dict(B=1), dict(B=1025), dict(A=0), dict(A=16), dict(D=0), dict(D=41), dict(H=255)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_shapes_outside_the_limits_are_refused(kw):
    a = dict(B=64, D=23, H=256, A=9)
    a.update(kw)
    lib = _capi.lib
    assert lib.pc_ppo_workspace_floats(a["B"], a["D"], a["H"], a["A"]) == UNS
    if "A" not in kw and "H" not in kw:      # (the prepared block depends on B and D alone)
        assert lib.pc_ppo_prepared_floats(a["B"], a["D"]) == UNS
    for device in (0, -1):                   # (the shape is looked at before the device)
        for apply in (0, 1, 2):
            assert lib.pc_ppo_minibatch(device, P, a["B"], a["D"], a["H"], a["A"], *(P,) * 5, *(P,) * 6, R.CLIP, R.VF, R.EC, R.MAX_NORM, 0.9,
                                        0.999, 1e-5, P, P, apply, None) == UNS


def test_shapes_at_the_limits_are_taken():
    lib = _capi.lib
    for B, D, A in ((2, 1, 1), (1024, 40, 15)):
        n = R.n_param(D, A)
        n_part = (B + 7) // 8
        assert lib.pc_ppo_workspace_floats(B, D, 256, A) == n_part * ((n + 3) // 4 * 4) + 4 * n_part + (n + 255) // 256
        assert lib.pc_ppo_prepared_floats(B, D) == B * (D + 4) + 4
