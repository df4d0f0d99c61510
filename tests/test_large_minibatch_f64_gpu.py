"""The large-minibatch PPO step on the GPU at its edge shapes: pc_ppo_adv_stats (KLs) + pc_ppo_minibatch_large (K10L forward / loss /
backward around a walk loop, K11 reduce, K12 clip + Adam) through the C-ABI against the float64 restatement of
tests/ppo_update_reference.py (ppo.ppo_loss on a .double() copy of the agent, clip_grad_norm_, torch.optim.Adam(lr 3e-4, eps 1e-5),
computed on the CPU once per case).  The structure and the assertions are tests/test_ppo_update_f64_gpu.py's, the bars
tests/test_ppo_golden.py's: gradient rtol 2e-4 / atol 2e-7, metric sums rel 1e-5 / abs 1e-6, parameters 3e-6.
tests/test_large_minibatch_f64_host.py holds the inputs of every case below to the conditions these bars rest on.

Shapes (B, D, A).  B is laid out for K10L's fixed grid on the 256 compute units of an MI355X: 129 groups of eight samples (129
workgroups, one group each), 257 (workgroup 0 walks a second group), 513 (a third: the first whose indices were requested two groups
ahead), 769 (a fourth), the last group holding 1 .. 8 live samples (every residue of B mod 8); 4097: workgroup 0's third group is the
one-sample tail; 4104 with D = 39 and 4097 with D = 40: full extra groups in the rolled 40-wide form.  (D, A): the three compiled shapes,
and the generic forms at the ends of their ranges, D = 1, 7, 24 | 25, 40 with A = 1, 2, 3, 8, 15 (layer 2 cut into 4, 4, 4, 3, 2 parts).
Indices are drawn with replacement from a pool of B + 7 rows and start (0, pool - 1, 2, 2): the clamped dead-slot loads (idx[B - 1],
feature D - 1) have nothing behind them but the allocation's end.  What was measured on an MI355X is tabulated in DESIGN 4.7."""
import numpy as np
import pytest
import torch

import ppo_update_reference as R
from ppo_car_amd import _capi
from ppo_update_reference import Call

pytestmark = pytest.mark.gpu
lib = _capi.lib

DATA = ("obs", "act", "old_lp", "adv", "ret")
STATE = ("param", "grad", "m", "v", "step", "metrics")
MAXB = _capi.PC_PPO_LARGE_MAX_B
sid = lambda s: f"B{s[0]}-D{s[1]}-A{s[2]}"
# the cases, from the reference module's tables (tests/test_large_minibatch_f64_host.py checks that these are the ones it holds)
ONE_STEP_CASES = [(s, scale) for scale in (1.0, 40.0) for s in R.LARGE_SHAPES]
SATURATED_CASES = R.LARGE_SATURATED
APPLIED_CASES = [(s, mn) for s in R.LARGE_APPLIED for mn in (R.LARGE_MAX_NORM, R.LARGE_IDLE_NORM)]
ROBUST_CASES = R.LARGE_ROBUST
CONST_ADV_CASES = R.LARGE_CONST_ADV


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
    stats = R.adv_stats(idx[0].view(1, -1), c["B"], data[3])
    kw.setdefault("max_norm", c["max_norm"])
    return Call(c["p0"].cuda(), c["B"], c["D"], c["A"], large=True, **kw).large(idx[0], *data, stats[0], apply=apply)


def _untouched(call, c):
    assert torch.equal(call.param.cpu(), c["p0"]) and float(call.step) == 0.0 and not call.m.any() and not call.v.any()


def test_the_walk_each_case_was_laid_out_for():
    """pc_ppo_large_parts: G = 129 workgroups for the 129-group cases, else 256, and workgroup 0 walks ceil(groups / G) = 1, 2, 3, 4
    groups.  On a device with another compute-unit count this fails: the cases below then do not reach the groups their names say."""
    cus = lib.pc_ppo_large_parts(0, MAXB)
    assert cus == 256, (f"this device runs the large step on {cus} workgroups at most: the cases of this file are laid out for the 256 compute "
                        "units of an MI355X and do not walk the second, third and fourth groups they were chosen for")
    depth_of = {129: 1, 257: 2, 513: 3, 769: 4}
    seen = set()
    for B, D, A in R.LARGE_SHAPES + [(1025, 39, 9)]:
        groups = (B + 7) // 8
        G = lib.pc_ppo_large_parts(0, B)
        assert G == (129 if groups == 129 else 256), (B, G)
        assert -(-groups // G) == depth_of[groups], (B, G)
        seen.add((depth_of[groups], D > 24))
    assert {d for d, _ in seen} == {1, 2, 3, 4} and (2, True) in seen and (3, True) in seen      # (rolled form: full extra groups)
    assert 4097 - 8 * 2 * 256 == 1                                          # workgroup 0's third group at B = 4097: one live sample
    assert R.WALK_SAMPLE == 8 * cus


# ---- a. the gradient and the metric sums ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale", ONE_STEP_CASES, ids=[f"{sid(s)}-x{x:g}" for s, x in ONE_STEP_CASES])
def test_gradient_and_metrics_against_float64(shape, scale):
    """apply = 0 against ppo_loss in float64.  Worst error / allowance per case as measured on an MI355X, with its slice and torch's
    own float32 on the CPU next to it: DESIGN 4.7's table."""
    c = R.case(*shape, scale, 1, R.LARGE_MAX_NORM)
    r = c["ref"][0]
    call = _one_step(c)
    g, m = _np(call.grad), _np(call.metrics)
    by = R.worst_by_slice(g, r["grad"], shape[1], shape[2])
    print(f"MEASURED a B={shape[0]} D={shape[1]} A={shape[2]} scale={scale:g}: worst error / allowance = {R.worst(g, r['grad']):.3f} in "
          f"{max(by, key=by.get)}; float32 torch {R.worst(R.restated32(*shape, scale, 1, R.LARGE_MAX_NORM)[0]['grad'], r['grad']):.3f}; by slice "
          f"{ {k: round(v, 3) for k, v in by.items()} }; metrics {m} reference {r['metrics']}")
    assert np.allclose(g, r["grad"], rtol=R.GRAD_RTOL, atol=R.GRAD_ATOL)
    _metrics_hold(m, r["metrics"])
    _untouched(call, c)


# ---- b. one action ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("shape", [s for s in R.LARGE_SHAPES if s[2] == 1], ids=sid)
def test_one_action_leaves_the_actor_exactly_at_rest(shape, scale):
    """A = 1: the log-prob is 0 whatever the weights, so the actor's four gradient slices are exactly zero (either sign) and so is the
    entropy sum; the critic's slices are held as above."""
    c = R.case(*shape, scale, 1, R.LARGE_MAX_NORM)
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
@pytest.mark.parametrize("shape", SATURATED_CASES, ids=sid)
def test_saturated_softmax_against_float64(shape):
    """actor[2] x 4000: logits of tens, probabilities of 1 and e-20.  torch's own float32 misses the gradient's bar here (the host
    test prints by how much; the figure moves with the CPU), so the gradient is held per element to  2e-4 |g64| + 4 max_i |g32_i - g64_i|,
    g32 = the float32 CPU restatement of the same case, as tests/test_ppo_update_f64_gpu.py does and for its reason: the kernel sums the
    same ill-conditioned terms in another order (k-parts, groups of eight in walking order, partials).  The metric sums keep the
    project's bar.  Measured max|g - g64| / max|g32 - g64| on an MI355X: DESIGN 4.7."""
    c = R.case(*shape, 4000.0, 1, R.LARGE_MAX_NORM)
    r, r32 = c["ref"][0], R.restated32(*shape, 4000.0, 1, R.LARGE_MAX_NORM)[0]
    call = _one_step(c)
    g, m = _np(call.grad), _np(call.metrics)
    e32 = float(np.abs(r32["grad"] - r["grad"]).max())
    allow = R.saturated_allowance(r32["grad"], r["grad"])
    print(f"MEASURED c B={shape[0]} D={shape[1]} A={shape[2]} scale=4000: max|g - g64| {np.abs(g - r['grad']).max():.3e}, max|g32 - g64| {e32:.3e}, ratio "
          f"{np.abs(g - r['grad']).max() / e32:.3f}; worst error / the project's allowance {R.worst(g, r['grad']):.3f} (float32 torch: "
          f"{R.worst(r32['grad'], r['grad']):.3f}); metrics {m} reference {r['metrics']}")
    assert (np.abs(g - r["grad"]) <= allow).all()
    _metrics_hold(m, r["metrics"])
    _untouched(call, c)


# ---- d. several applied steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,max_norm", APPLIED_CASES, ids=[f"{sid(s)}-norm{mn:g}" for s, mn in APPLIED_CASES])
def test_four_applied_steps_against_float64(shape, max_norm):
    """Four apply = 1 steps on four minibatches whose statistics come from ONE pc_ppo_adv_stats call (n_mb = 4): bias correction after
    the first step, non-zero moments, the norm clip acting (0.05) and idle (1e9).  The moments' bars after the first step follow from
    the gradient's: m = 0.1 gc, v = 0.001 gc^2.  Worst parameter error measured on an MI355X: DESIGN 4.7."""
    c = R.case(*shape, 1.0, 4, max_norm)
    for r in c["ref"]:      # (the host test has the same condition)
        assert (r["norm"] > max_norm) == (max_norm == R.LARGE_MAX_NORM)
    data, idx = _dev(c)
    stats = R.adv_stats(torch.stack(idx).contiguous(), shape[0], data[3])
    call = Call(c["p0"].cuda(), *shape, max_norm=max_norm, large=True)
    before = c["p0"].double().numpy()
    for t, r in enumerate(c["ref"]):
        call.large(idx[t], *data, stats[t], apply=1)
        p, g = _np(call.param), _np(call.grad)
        print(f"MEASURED d {sid(shape)} max_norm {max_norm:g} step {t + 1}: parameters max abs err {np.abs(p - r['param']).max():.3e}; clipped "
              f"gradient worst error / allowance {R.worst(g, r['grad_clipped']):.3f}")
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


# ---- e. apply = 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,max_norm", APPLIED_CASES, ids=[f"{sid(s)}-norm{mn:g}" for s, mn in APPLIED_CASES])
def test_apply_2_advances_the_counter_and_leaves_the_raw_gradient(shape, max_norm):
    """include/ppocar.h: apply == 2 stops after the gradient but advances the step counter: parameters and moments untouched, grad
    unclipped whatever max_norm and bit-equal to apply = 0's."""
    c = R.case(*shape, 1.0, 4, max_norm)
    r = c["ref"][0]
    zero, two = _one_step(c, 0), _one_step(c, 2)
    assert float(two.step) == 1.0 and float(zero.step) == 0.0
    assert torch.equal(two.param.cpu(), c["p0"]) and not two.m.any() and not two.v.any()
    assert np.allclose(_np(two.grad), r["grad"], rtol=R.GRAD_RTOL, atol=R.GRAD_ATOL)
    assert torch.equal(two.grad, zero.grad) and torch.equal(two.metrics, zero.metrics)


# ---- f. constant advantages -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CONST_ADV_CASES, ids=sid)
def test_constant_advantages(shape):
    """Every adv = 0.5 at B = 2048 + 8 and 4096 + 1: the shifted sums are exactly 0, KLs returns exactly (0.5, the floor 1e-5), the
    normalised advantage is exactly 0: the policy-loss sum is exactly 0 and the actor's gradient is the entropy term's alone."""
    B, D, A = shape
    c = R.case(B, D, A, 1.0, 1, R.LARGE_MAX_NORM, 0.5)
    r = c["ref"][0]
    assert not r["adv_n"].any() and r["metrics"][0] == 0.0
    ent_only = R.gradient_of(c, entropy_only=True)
    o = R.slice_bounds(D, A)[4][1]
    data, idx = _dev(c)
    stats = R.adv_stats(idx[0].view(1, B), B, data[3])
    assert stats.cpu().numpy().tolist() == [[0.5, float(np.float32(1e-5))]]
    call = Call(c["p0"].cuda(), B, D, A, max_norm=R.LARGE_MAX_NORM, large=True).large(idx[0], *data, stats[0], apply=0)
    g = _np(call.grad)
    print(f"B={B}: actor against the entropy term alone, worst error / allowance {R.worst(g[:o], ent_only[:o]):.3f}; whole gradient {R.worst(g, r['grad']):.3f}")
    assert float(call.metrics[0]) == 0.0
    assert np.allclose(g[:o], ent_only[:o], rtol=R.GRAD_RTOL, atol=R.GRAD_ATOL)
    assert np.allclose(g, r["grad"], rtol=R.GRAD_RTOL, atol=R.GRAD_ATOL)
    _metrics_hold(_np(call.metrics), r["metrics"])


# ---- g. robustness, on bits -------------------------------------------------------------------------------------------------------
def _one_element_in(t):
    """the same values as a view one element into a larger allocation: 4 bytes past a 16-byte boundary"""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = big[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("shape", ROBUST_CASES, ids=sid)
def test_the_same_bits_whatever_the_buffers(shape):
    """One applied step: twice; with both workspaces full of NaN (nothing is read that the step has not written; the statistics'
    workspace is NaN in every call); with grad, the moments, step, lr and metrics each 16 bytes into a larger allocation; with obs / act
    / old_lp / adv / ret and the statistics pair one element into a larger allocation, which no 16-byte load could take (include/ppocar.h
    asks 16-byte alignment of param and workspace alone); with the index row the middle one of a wider matrix (idx_ld = B + 5) for the
    statistics, whose other entries all point at row 1."""
    B = shape[0]
    c = R.case(*shape, 1.0, 1, R.LARGE_MAX_NORM)
    data, idx = _dev(c)
    p0 = c["p0"].cuda()
    stats = R.adv_stats(idx[0].view(1, B), B, data[3])

    def run(d=data, ix=idx[0], st=stats[0], **kw):
        return Call(p0, *shape, max_norm=R.LARGE_MAX_NORM, large=True, **kw).large(ix, *d, st, apply=1)

    base = run()
    wide = torch.ones((3, B + 5), dtype=torch.int64, device="cuda")
    wide[1, :B] = idx[0]
    wide_stats = R.adv_stats(wide[:, :B], B, data[3])
    assert wide[:, :B].stride(0) == B + 5 and torch.equal(wide_stats[1], stats[0]) and not torch.equal(wide_stats[0], stats[0])
    others = dict(again=run(), nan_workspace=run(ws_fill=float("nan")), shifted_state=run(shift=4),
                  unaligned_inputs=run(tuple(_one_element_in(t) for t in data), st=_one_element_in(stats[0])),
                  embedded_indices=run(ix=wide[1, :B], st=wide_stats[1]))
    assert others["shifted_state"].grad.data_ptr() % 16 == 0 and others["shifted_state"].grad.data_ptr() != others["shifted_state"].grad.untyped_storage().data_ptr()
    assert float(base.step) == 1.0 and bool(torch.isfinite(base.param).all()) and not torch.equal(base.param, p0)
    for name, o in others.items():
        for k in STATE:
            assert torch.equal(getattr(base, k), getattr(o, k)), (name, k)


# ---- h. the advantage statistics alone --------------------------------------------------------------------------------------------
def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


KLS = {                # n_mb, B, pool, with replacement, idx_ld - B, the first gathered advantage an outlier
    "B2048-one-workgroup": (3, 2048, 8192, False, 0, False),
    "B2049-two-workgroups": (3, 2049, 8192, False, 0, False),
    "B131073-P-clamped-at-64": (1, 131073, 1 << 18, False, 0, False),
    "B-the-limit": (1, MAXB, MAXB + 11, True, 0, False),
    "duplicates": (3, 2056, 600, True, 0, False),
    "idx_ld-above-B": (3, 4099, 3 * 4099, False, 5, False),
    "B1025-outlier-shift": (3, 1025, 8192, False, 0, True),
    "B4099-outlier-shift": (3, 4099, 3 * 4099, False, 0, True),
}


@pytest.mark.parametrize("name", list(KLS))
def test_advantage_statistics(name):
    """tests/test_large_minibatch_gpu.py's criterion: with a mean of 100 x the std, (mean, unbiased std) within one float32 ulp of
    float64 numpy rounded to float32, and a constant advantage gives exactly (the constant, 1e-5f).  At the 1 -> 2 workgroup boundary,
    from where P is clamped at 64, at PC_PPO_LARGE_MAX_B, with repeated indices, with the index rows inside a wider matrix, and with the
    shift K (the first gathered advantage) 100 standard deviations from the mean: the float64 shifted sums then lose at most about
    n 2^-53 10^4 = 5e-9 relative, far below half a float32 ulp, so the bar still follows."""
    n_mb, B, pool, replace, extra, outlier = KLS[name]
    g = torch.Generator().manual_seed(B + extra)
    adv = (100.0 + torch.randn(pool, generator=g)).float()
    if replace:
        rows = torch.randint(0, pool, (n_mb, B), generator=g)
    else:                                                       # (disjoint minibatches: one permutation cut into rows)
        rows = torch.randperm(pool, generator=g)[:n_mb * B].view(n_mb, B).contiguous()
    assert (len(set(rows[0].tolist())) < B) == replace
    if outlier:
        for m in range(n_mb):
            rest = adv[rows[m, 1:]].double()
            adv[rows[m, 0]] = float(rest.mean() + 100.0 * rest.std())
    wide = torch.ones((n_mb, B + extra), dtype=torch.int64)
    wide[:, :B] = rows
    dev = wide.cuda()[:, :B]
    assert dev.stride(0) == B + extra
    assert lib.pc_ppo_adv_stats_workspace_doubles(n_mb, B) == 2 * n_mb * min(64, -(-B // 2048))
    stats = R.adv_stats(dev, B, adv.cuda()).cpu().numpy()
    for m in range(n_mb):
        x = adv.numpy()[rows[m].numpy()].astype(np.float64)
        mean, sd = np.float32(x.mean()), np.float32(x.std(ddof=1))
        print(f"{name} minibatch {m}: mean {stats[m, 0]!r} ref {mean!r}, std {stats[m, 1]!r} ref {sd!r}")
        if outlier:
            assert abs(x[0] - x[1:].mean()) > 99.99 * x[1:].std(ddof=1)
        assert _ulps(stats[m, 0], mean) <= 1 and _ulps(stats[m, 1], sd) <= 1
    const = R.adv_stats(dev, B, torch.full((pool,), 2.5, device="cuda")).cpu().numpy()
    assert (const[:, 0] == np.float32(2.5)).all() and (const[:, 1] == np.float32(1e-5)).all()


# ---- i. row addresses beyond 2^31 elements, on bits -------------------------------------------------------------------------------
def test_rows_beyond_2_31_elements():
    """all row addresses are 64-bit.  D = 39; obs is an allocation of ceil(2^31 / 39) + 16 rows (8.6 GB, never filled but for
    NaN around the rows in use), act / old_lp / adv / ret to match; pool row p of a case lives in big row p (p even) or last - p (p odd),
    the indices are mapped the same way: rows at both ends, those with odd p <= 15 starting beyond 2^31 elements -- where a 32-bit
    idx * D has wrapped -- and all the odd ones beyond 2^32 bytes.  pc_ppo_adv_stats + pc_ppo_minibatch_large at (1025, 39, 9),
    pc_ppo_minibatch and pc_ppo_prepare + pc_ppo_minibatch_prepared at (9, 39, 9) give the bits of the same calls on the compact pool.
    Nothing outside the written rows is read (their neighbours are NaN) but the clamped dead-slot re-reads of live rows."""
    D, A = 39, 9
    n_rows = -(-2 ** 31 // D) + 16
    last = n_rows - 1
    big = [torch.empty((n_rows, D), device="cuda")] + [torch.empty(n_rows, device="cuda") for _ in range(4)]
    try:
        for B in (1025, 9):
            c = R.inputs(B, D, A)
            data, idx = _dev(c)
            pool = c["pool"]
            p = torch.arange(pool, device="cuda")
            where = torch.where(p % 2 == 0, p, last - p)
            for t, small in zip(big, data):
                t[:pool + 8] = float("nan")
                t[last - pool - 8:] = float("nan")
                t[where] = small
            big_idx = where[idx[0]].contiguous()
            assert int((big_idx * D >= 2 ** 31).sum()) >= 1 and int((big_idx * D * 4 >= 2 ** 32).sum()) >= 1 and int((big_idx < pool).sum()) >= 3
            p0 = c["p0"].cuda()
            if B > 1024:
                s_small, s_big = R.adv_stats(idx[0].view(1, B), B, data[3]), R.adv_stats(big_idx.view(1, B), B, big[3])
                assert torch.equal(s_small, s_big) and bool(torch.isfinite(s_big).all())
                pairs = [(Call(p0, B, D, A, max_norm=R.LARGE_MAX_NORM, large=True).large(idx[0], *data, s_small[0], apply=1),
                          Call(p0, B, D, A, max_norm=R.LARGE_MAX_NORM, large=True).large(big_idx, *big, s_big[0], apply=1))]
            else:
                prep_small, prep_big = R.prepare(idx[0].view(1, B), B, D, *data), R.prepare(big_idx.view(1, B), B, D, *big)
                assert torch.equal(prep_small, prep_big) and bool(torch.isfinite(prep_big).all())
                pairs = [(Call(p0, B, D, A).ppo(idx[0], *data, apply=1), Call(p0, B, D, A).ppo(big_idx, *big, apply=1)),
                         (Call(p0, B, D, A).prepared(prep_small[0], apply=1), Call(p0, B, D, A).prepared(prep_big[0], apply=1))]
            for small_call, big_call in pairs:
                assert float(big_call.step) == 1.0 and bool(torch.isfinite(big_call.param).all()) and not torch.equal(big_call.param, p0)
                for k in STATE:
                    assert torch.equal(getattr(small_call, k), getattr(big_call, k)), (B, k)
    finally:
        del big
        torch.cuda.empty_cache()
