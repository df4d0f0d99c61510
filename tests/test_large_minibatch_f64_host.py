"""The inputs of tests/test_large_minibatch_f64_gpu.py held to their conditions on the CPU, and the refusals and limits of the
large-minibatch entry points that tests/test_large_minibatch_host.py does not have.  The conditions are
tests/test_ppo_update_f64_host.py's, at the same bars, for every case the GPU file runs: no sample on a clip edge, every branch taken,
torch's own float32 within half the allowance, a single dropped sample (the last one; from B = 2049 also the first sample of workgroup
0's second group) or a single wrong clip decision more than 20 x the allowance away, the norm clip biting at 0.05 and idle at 1e9.
No case is skipped or excluded: a seed that breaks a condition is changed in ppo_update_reference's case table.  No GPU needed."""
import numpy as np
import pytest
import torch

import ppo_update_reference as R
from ppo_car_amd import _capi

INV, UNS, NODEV = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_UNSUPPORTED, _capi.PC_ERR_NO_DEVICE
MAXB = _capi.PC_PPO_LARGE_MAX_B
P = 4096      # a non-NULL 16-byte aligned address, never dereferenced: every refusal below comes before any device call
ONE_STEP, MULTI = R.LARGE_ONE_STEP, R.LARGE_MULTI
ids = lambda cases: [f"B{s[0]}-D{s[1]}-A{s[2]}-x{scale:g}-n{steps}-norm{mn:g}" for s, scale, steps, mn in cases]


def _edge_distance(r):
    return float(np.minimum(np.abs(r["ratio"] - (1.0 - R.CLIP)), np.abs(r["ratio"] - (1.0 + R.CLIP))).min())


def _combos(r):
    side = np.where(r["ratio"] < 1.0 - R.CLIP, 0, np.where(r["ratio"] > 1.0 + R.CLIP, 2, 1))
    return {(int(s), bool(a > 0)) for s, a in zip(side, r["adv_n"])}


def test_the_gpu_file_runs_these_cases_and_no_others():
    """The GPU file's parameter lists are the reference module's tables, which the tests below walk in full."""
    import test_large_minibatch_f64_gpu as G
    assert len(R.LARGE_SHAPES) == 15 == len(set(R.LARGE_SHAPES)) and not set(R.LARGE_SHAPES) & set(R.SHAPES)
    for sub in (R.LARGE_SATURATED, R.LARGE_APPLIED, R.LARGE_ROBUST, R.LARGE_CONST_ADV):
        assert set(sub) <= set(R.LARGE_SHAPES)
    assert G.ONE_STEP_CASES == [(s, scale) for s, scale, _, _ in ONE_STEP if scale < 4000.0]
    assert G.SATURATED_CASES == [s for s, scale, _, _ in ONE_STEP if scale == 4000.0] == R.LARGE_SATURATED
    assert G.APPLIED_CASES == [(s, mn) for s, _, _, mn in MULTI]
    assert G.ROBUST_CASES == R.LARGE_ROBUST and G.CONST_ADV_CASES == R.LARGE_CONST_ADV
    assert {s for s, _, _, _ in ONE_STEP} == set(R.LARGE_SHAPES)
    assert {s[0] % 8 for s in R.LARGE_SHAPES} == set(range(8))
    assert {(s[0] + 7) // 8 for s in R.LARGE_SHAPES} == {129, 257, 513, 769}
    assert {s for s, _, steps, _ in MULTI if steps == 4} == set(R.LARGE_APPLIED)


@pytest.mark.parametrize("shape,scale,steps,max_norm", ONE_STEP + MULTI, ids=ids(ONE_STEP + MULTI))
def test_no_ratio_near_a_clip_edge(shape, scale, steps, max_norm):
    """In float64 every sample's ratio is at least 1e-5 from 1 - clip and 1 + clip (a float32 ratio here is off by less than 1e-6):
    along the reference's whole trajectory where several steps are applied."""
    c = R.case(*shape, scale, steps, max_norm)
    d = min(_edge_distance(r) for r in c["ref"])
    print(f"smallest distance of a ratio from a clip edge: {d:.3e}")
    assert d >= 1e-5


@pytest.mark.parametrize("shape,scale,steps,max_norm", ONE_STEP + MULTI, ids=ids(ONE_STEP + MULTI))
def test_every_branch_is_taken(shape, scale, steps, max_norm):
    """ratio below, inside and above the clip range x normalised advantage negative and positive: all six, at every step"""
    for r in R.case(*shape, scale, steps, max_norm)["ref"]:
        assert len(_combos(r)) == 6


@pytest.mark.parametrize("shape,scale,steps,max_norm", ONE_STEP, ids=ids(ONE_STEP))
def test_float32_torch_against_float64(shape, scale, steps, max_norm):
    """torch's own float32 on the CPU keeps half the allowance at scale 1 and 40 (gradient: rtol 2e-4, atol 2e-7; metric sums: rel 1e-5,
    abs 1e-6).  At scale 4000 it does not hold the gradient's (printed), which is why the GPU file has another allowance there; it
    holds 0.75 of the metric sums'."""
    r64, r32 = R.case(*shape, scale, steps, max_norm)["ref"][0], R.restated32(*shape, scale, steps, max_norm)[0]
    wg = R.worst(r32["grad"], r64["grad"])
    wm = float((np.abs(r32["metrics"] - r64["metrics"]) / (R.MET_ABS + R.MET_REL * np.abs(r64["metrics"]))).max())
    print(f"float32 torch: gradient worst error / allowance {wg:.3f}, metrics {wm:.3f}; by slice {R.worst_by_slice(r32['grad'], r64['grad'], shape[1], shape[2])}")
    if scale < 4000.0:
        assert wg <= 0.5 and wm <= 0.5
    else:
        assert wm <= 0.75


@pytest.mark.parametrize("shape,scale,steps,max_norm", ONE_STEP, ids=ids(ONE_STEP))
def test_a_single_wrong_sample_is_far_outside_the_allowance(shape, scale, steps, max_norm):
    """The float64 gradient with the last sample dropped, with sample 8 * 256 dropped (B > 2048) and with the clip decision of the
    first out-of-range sample inverted each differ from the true one by more than 20 x the allowance in at least one element (at
    scale 4000: 20 x that scale's allowance)."""
    c = R.case(*shape, scale, steps, max_norm)
    g = c["ref"][0]["grad"]
    own = R.gradient_of(c)
    assert np.abs(own - g).max() <= 1e-12 * max(1.0, np.abs(g).max())      # the per-sample restatement is ppo_loss
    allow = R.allowance(g) if scale < 4000.0 else R.saturated_allowance(R.restated32(*shape, scale, steps, max_norm)[0]["grad"], g)
    dropped, flipped = R.wrong_gradients(c)
    wd, wf = R.worst(dropped, g, allow), R.worst(flipped, g, allow)
    print(f"one sample dropped: {wd:.1f} x the allowance; one clip decision inverted: {wf:.1f} x")
    assert wd > 20.0
    if shape[0] > R.WALK_SAMPLE:
        ww = R.worst(R.walk_wrong_gradient(c), g, allow)
        print(f"sample {R.WALK_SAMPLE} dropped: {ww:.1f} x")
        assert ww > 20.0
    if shape[2] == 1:      # one action: the log-prob is the constant 0 and no clip decision reaches a gradient -- held exactly on the GPU
        assert np.array_equal(flipped, g)
    else:
        assert wf > 20.0


@pytest.mark.parametrize("shape", R.LARGE_APPLIED)
def test_the_norm_clip_acts_in_one_setting_only(shape):
    for r in R.case(*shape, 1.0, 4, R.LARGE_MAX_NORM)["ref"]:
        assert r["norm"] > R.LARGE_MAX_NORM and not np.array_equal(r["grad"], r["grad_clipped"])
    for r in R.case(*shape, 1.0, 4, R.LARGE_IDLE_NORM)["ref"]:
        assert np.array_equal(r["grad"], r["grad_clipped"])


def test_indices_repeat_and_reach_both_ends_of_the_pool():
    for s in R.LARGE_SHAPES:
        for steps in (1, 4):
            c = R.inputs(*s, 1.0, steps)
            for ix in c["idx"]:
                ix = ix.tolist()
                assert len(ix) == s[0] and min(ix) == 0 and max(ix) == c["pool"] - 1 == s[0] + 6
                assert ix[:4] == [0, c["pool"] - 1, 2, 2] and len(set(ix)) < s[0]


def test_constant_advantage_cases_are_what_the_gpu_file_says():
    """every adv = 0.5: the float64 normalised advantage and policy-loss sum are exactly 0, the actor's gradient is the entropy term's"""
    for B, D, A in R.LARGE_CONST_ADV:
        c = R.case(B, D, A, 1.0, 1, R.LARGE_MAX_NORM, 0.5)
        r = c["ref"][0]
        assert not r["adv_n"].any() and r["metrics"][0] == 0.0
        ent_only = R.gradient_of(c, entropy_only=True)
        o = R.slice_bounds(D, A)[4][1]
        assert np.abs(ent_only[:o] - r["grad"][:o]).max() <= 1e-15 and not ent_only[o:].any() and np.abs(ent_only[:o]).max() > 1e-6


def test_the_small_cases_keep_their_draws():
    """The large tables were added beside the small ones: the draws of the small cases are what they were before -- a digest of the
    tensors that come out of the seeded generator alone (obs, act, adv, ret, the indices of every step)."""
    import hashlib
    want = {((9, 39, 9), 1.0, 1): "835d0f5d33a3a04b", ((256, 23, 9), 1.0, 4): "c9c113d0a0be9260", ((1023, 40, 15), 40.0, 1): "214e7f52814eaa82",
            ((65, 25, 2), 1.0, 3): "aa6674d71e10f03d"}
    for (s, scale, steps), digest in want.items():
        c = R.inputs(*s, scale, steps)
        h = hashlib.sha256()
        for t in [c["obs"], c["act"], c["adv"], c["ret"]] + c["idx"]:
            h.update(t.numpy().tobytes())
        assert h.hexdigest()[:16] == digest, s
    assert all(k[0] <= 1024 for k in R.HAND) and not R.ADV_RAISED


# ---- limits and refusals: the documented code before any device call --------------------------------------------------------------
def test_adv_stats_workspace_at_its_boundaries():
    """P = ceil(B / 2048) workgroups per minibatch, clamped at 64: two doubles each"""
    ws = _capi.lib.pc_ppo_adv_stats_workspace_doubles
    for B, parts in ((1025, 1), (2048, 1), (2049, 2), (131072, 64), (131073, 64), (MAXB, 64)):
        assert ws(1, B) == 2 * parts, B
        assert ws(7, B) == 7 * 2 * parts, B
    assert ws(1, 63 * 2048) == 2 * 63 and ws(1, 63 * 2048 + 1) == 2 * 64      # (64 is reached before it clamps)


def test_large_workspace_at_the_limits():
    lib = _capi.lib
    for B, D, A in ((1025, 1, 1), (MAXB, 40, 15)):
        if not torch.cuda.is_available():
            assert lib.pc_ppo_large_workspace_floats(0, B, D, 256, A) == NODEV
            continue
        parts = lib.pc_ppo_large_parts(0, B)
        assert 0 < parts <= (B + 7) // 8
        n = R.n_param(D, A)
        assert lib.pc_ppo_large_workspace_floats(0, B, D, 256, A) == parts * ((n + 3) // 4 * 4) + 4 * parts + (n + 255) // 256
    assert lib.pc_ppo_large_workspace_floats(-1, MAXB, 40, 256, 15) == NODEV
    assert lib.pc_ppo_large_workspace_floats(0, MAXB + 1, 40, 256, 15) == UNS and lib.pc_ppo_large_workspace_floats(0, 1025, 0, 256, 1) == UNS


def _small(param=P, ws=P, B=64, device=-1, apply=1):
    return _capi.lib.pc_ppo_minibatch(device, P, B, 23, 256, 9, *(P,) * 5, param, P, *(P,) * 4, R.CLIP, R.VF, R.EC, R.MAX_NORM, 0.9, 0.999, 1e-5,
                                      P, ws, apply, None)


def _large(param=P, ws=P, B=2056, device=-1, apply=1, others=P):
    return _capi.lib.pc_ppo_minibatch_large(device, others, B, 23, 256, 9, *(others,) * 5, others, param, others, *(others,) * 4, R.CLIP, R.VF,
                                            R.EC, R.MAX_NORM, 0.9, 0.999, 1e-5, others, ws, apply, None)


def _bc(param=P, ws=P, B=64, device=-1, apply=1):
    return _capi.lib.pc_bc_minibatch(device, P, B, 23, 256, 9, P, P, P, param, P, *(P,) * 4, R.VF, R.EC, R.MAX_NORM, 0.9, 0.999, 1e-5, P, ws, apply,
                                     None)


@pytest.mark.parametrize("call", [_small, _large, _bc], ids=["pc_ppo_minibatch", "pc_ppo_minibatch_large", "pc_bc_minibatch"])
def test_param_and_workspace_must_be_16_byte_aligned(call):
    """include/ppocar.h: the forward / backward launch loads `param` and stores the workspace's partials as 16-byte vectors.  A
    misaligned one is PC_ERR_INVALID_ARG with the NULL checks: before the shape (UNSUPPORTED) and the device (NO_DEVICE) are looked at."""
    for off in (4, 8, 12):
        for apply in (0, 1, 2):
            assert call(param=P + off, apply=apply) == INV and call(ws=P + off, apply=apply) == INV
            assert call(param=P + off, device=0, apply=apply) == INV and call(ws=P + off, device=0, apply=apply) == INV
        assert call(param=P + off, B=1) == INV and call(ws=P + off, B=1) == INV      # (before the shape)
    # aligned addresses pass that check: the next refusal is the shape's
    assert call(B=1) == UNS and call(param=P + 16, B=1) == UNS and call(ws=P + 16, B=1) == UNS
    if call is not _small:                                        # (these two refuse device -1 themselves, before any device call)
        assert call() == NODEV and call(param=P + 16, ws=P + 32) == NODEV


def test_nothing_else_needs_more_than_its_elements_alignment():
    """every other pointer of pc_ppo_minibatch_large 4 bytes past a 16-byte boundary (idx: 8): accepted up to the device check"""
    assert _large(others=P + 4) == NODEV
    assert _capi.lib.pc_ppo_minibatch_large(-1, P + 8, 2056, 23, 256, 9, *(P + 4,) * 5, P + 4, P, P + 4, *(P + 4,) * 4, R.CLIP, R.VF, R.EC, R.MAX_NORM,
                                            0.9, 0.999, 1e-5, P + 4, P, 1, None) == NODEV
