"""The update kernels outside pc_ppo_minibatch on the GPU at their edge shapes: K6 ppo_gather_kernel on bits, K7 ppo_loss_kernel<16, .>
(pc_ppo_loss, pc_ppo_loss_diag), K8 clip_adam_kernel (pc_clip_adam) and K12m clip_adam_mb_kernel (pc_clip_adam_advanced, the clip + Adam
step of every multi-rank minibatch) against the float64 restatements of tests/update_tail_reference.py; the bit-level invariants that
follow from one adam_elem / adam_coef compiled with -ffp-contract=off and K8's same operation order; and the learner's two paths that
run them (custom_mlp = False; force_collective) over four steps against tests/ppo_update_reference.py's float64 trajectory.  The bars
are the project's: outputs of the loss GRAD_ATOL / B + GRAD_RTOL |ref| (s = 30: `saturated_allowance`), metric sums rel 1e-5 / abs 1e-6,
parameters 3e-6, exp_avg 0.1 allowance(gc), exp_avg_sq 0.002 |gc| allowance(gc) + 1e-15 with gc the float64 clipped gradient of the step.
tests/test_update_tail_f64_host.py holds the inputs to the conditions these bars rest on.  Every test prints its worst error / bar;
DESIGN 4.3 has the figures measured on an MI355X."""
import contextlib
import functools
import hashlib

import numpy as np
import pytest
import torch

import ppo_update_reference as R
import update_tail_reference as U
from ppo_car_amd import _capi
from ppo_update_reference import Call
from update_tail_reference import Tail

pytestmark = pytest.mark.gpu
lib = _capi.lib

LOSS_ALL = ([(B, A, 1.0, None) for B, A in U.LOSS_CASES] + [(B, A, U.SAT, None) for B, A in U.LOSS_SATURATED]
            + [(B, A, 1.0, 0.5) for B, A in U.LOSS_CONST_ADV])
lid = lambda c: f"B{c[0]}-A{c[1]}-s{c[2]:g}" + ("-const" if c[3] is not None else "")
sid = lambda s: f"B{s[0]}-D{s[1]}-A{s[2]}"
DATA = ("obs", "act", "old_lp", "adv", "ret")


def _np(t):
    return t.detach().cpu().double().numpy()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _metrics_hold(got, ref):
    for a, b, key in zip(got, ref, ("policy_loss", "value_loss", "entropy", "loss")):
        assert float(a) == pytest.approx(float(b), rel=R.MET_REL, abs=R.MET_ABS), key


# ---- K6 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("B,D", [(1, 1), (2, 23), (63, 39), (1024, 40), (1000, 61)])
def test_gather_is_indexing_bit_for_bit(B, D, shift):
    """tensor[idx] on bits -- a NaN, a -0.0 and a denormal among the rows -- with a duplicate, row 0 and the pool's last row among the
    indices; (1000, 61): B (D + 4) is no multiple of the 256 threads.  Nothing beyond [B][D] / [B] is written (the guard floats)."""
    g = torch.Generator().manual_seed(100 + B)
    M = B + 7
    obs, (act, lp, adv, ret) = torch.randn(M, D, generator=g), (torch.randn(M, generator=g) for _ in range(4))
    obs[0, 0], obs[M - 1, D - 1], obs[2, D // 2] = -0.0, float("nan"), 1e-41
    idx = torch.randint(0, M, (B,), generator=g)
    head = [0, M - 1, 2, 2] if B >= 4 else [M - 1, 0][:B]
    idx[:len(head)] = torch.tensor(head)
    t = Tail.gather(idx, obs, act, lp, adv, ret, shift=shift)
    for got, src in zip(t.dst, (obs, act, lp, adv, ret)):
        assert torch.equal(_bits(got), _bits(src[idx]))
    assert t.guards_hold()
    assert torch.equal(t.idx.cpu(), idx) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(t.src, (obs, act, lp, adv, ret)))


# ---- K7 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LOSS_ALL, ids=lid)
def test_loss_against_float64(case):
    """dlogits, dvalues and the metric increments against float64; a second call on the same state writes the same gradients and
    doubles the metric sums (the +=); pc_ppo_loss_diag with target_kl = 0 gives the same bits on all three outputs.
    Measured on an MI355X (DESIGN 4.3 has the table): dlogits 0.025 of the allowance at the most, the metric sums 0.029.  Before two
    changes in ppo_loss_kernel this test showed (1023, 9) at 1.39 x the dlogits allowance (a float32 mean of the advantages 3.0e-7 off,
    against a sample 0.003 from it: the deviations are now re-centred) and then (3, 9) x 30 at 1.004 x the policy-loss sum's (a
    log-prob good to an ulp of the largest logit: the log-ratio is now formed with l_a - max's rounding error)."""
    c = U.loss_case(*case)
    r, (al, av) = c["ref"], U.loss_allowances(c)
    t = Tail.for_loss(c).loss()
    dl, dv, m = _np(t.dlogits), _np(t.dvalues), _np(t.metrics)
    wm = float((np.abs(m - r["metrics"]) / (R.MET_ABS + R.MET_REL * np.abs(r["metrics"]))).max())
    print(f"{lid(case)}: worst error / allowance dlogits {float((np.abs(dl - r['dlogits']) / al).max()):.3f} dvalues "
          f"{float((np.abs(dv - r['dvalues']) / av).max()):.3f} metric sums {wm:.3f}; float32 torch on the CPU: dlogits "
          f"{float((np.abs(c['r32']['dlogits'] - r['dlogits']) / al).max()):.3f}; metrics {m} reference {r['metrics']}")
    assert (np.abs(dl - r["dlogits"]) <= al).all() and (np.abs(dv - r["dvalues"]) <= av).all()
    _metrics_hold(m, r["metrics"])
    d = Tail.for_loss(c).loss_diag(0.0)
    for k in ("dlogits", "dvalues", "metrics"):
        assert torch.equal(_bits(getattr(d, k)), _bits(getattr(t, k))), k
    assert float(d.diag[2]) == 1.0 and float(d.diag[3]) == 1.0 and float(d.diag[4]) == 0.0
    once = (t.dlogits.clone(), t.dvalues.clone())
    t.loss()
    assert torch.equal(t.dlogits, once[0]) and torch.equal(t.dvalues, once[1])
    _metrics_hold(_np(t.metrics), 2.0 * r["metrics"])
    assert t.guards_hold() and d.guards_hold()
    for x, k in zip(t.inp, ("logits", "values", "act", "old_lp", "adv", "ret")):
        assert torch.equal(x.cpu(), c[k]), k


@pytest.mark.parametrize("B", [2, 1024])
def test_one_action_leaves_dlogits_and_entropy_exactly_zero(B):
    """A = 1: the log-prob is 0 whatever the logit: dlogits exactly zero (either sign), an entropy sum of exactly 0"""
    c = U.loss_case(B, 1)
    assert not c["ref"]["dlogits"].any() and c["ref"]["metrics"][2] == 0.0
    t = Tail.for_loss(c).loss()
    assert bool((t.dlogits == 0.0).all()) and float(t.metrics[2]) == 0.0
    assert np.abs(_np(t.dvalues)).max() > 0


@pytest.mark.parametrize("B,A", U.LOSS_CONST_ADV)
def test_constant_advantages_leave_the_policy_terms_exactly_zero(B, A):
    """Every adv = 0.5 with B a power of two: the mean is exact, every deviation 0, the standard deviation at its floor: a policy-loss
    sum of exactly 0, and dlogits the entropy term's alone (float64's, at the allowance: test_loss_against_float64 has the case)"""
    c = U.loss_case(B, A, 1.0, 0.5)
    r = c["ref"]
    assert not r["adv_n"].any() and r["metrics"][0] == 0.0 and np.abs(r["dlogits"]).max() > 1e-8
    t = Tail.for_loss(c).loss().loss()
    assert float(t.metrics[0]) == 0.0
    assert (np.abs(_np(t.dlogits) - r["dlogits"]) <= U.loss_allowances(c)[0]).all()


@pytest.mark.parametrize("case", [(3, 9, 1.0, None), (65, 9, U.SAT, None), (1024, 16, 1.0, None)], ids=lid)
def test_the_loss_gives_the_same_bits_wherever_the_buffers_lie(case):
    """every buffer 4 bytes past a 16-byte boundary, dlogits / dvalues pre-filled with NaN instead of 7: the kernel writes all of both"""
    c = U.loss_case(*case)
    base, other = Tail.for_loss(c).loss(), Tail.for_loss(c, shift=1, fill=float("nan")).loss()
    assert other.dlogits.data_ptr() % 16 == 4
    for k in ("dlogits", "dvalues", "metrics"):
        assert torch.equal(_bits(getattr(base, k)), _bits(getattr(other, k))), k
    assert other.guards_hold()


# ---- K8 and K12m against float64 ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run(kernel, n, step0, max_norm, W, shift=0):
    """STEPS consecutive calls of one cell (tests/update_tail_reference.py: inputs and reference): the worst error / bar over the steps
    of (parameters, exp_avg, exp_avg_sq, K8: the clipped gradient written back), a digest per step of the bits of parameters and
    moments, and one of those with grad.  K12m: the test advances the counter itself, as the gradient kernels do under apply = 2."""
    c, ref = U.adam_inputs(n, step0), U.adam_case(n, step0, max_norm)
    t = Tail.for_adam(c["p"], c["m"], c["v"], step0, shift=shift)
    assert t.grad.data_ptr() % 16 == (4 * shift) % 16
    w, digests, with_grad = np.zeros(4), [], []
    for s, r in enumerate(ref):
        bucket = (c["grads"][s] * W).cuda()
        t.grad.copy_(bucket)
        if kernel == "k12m":
            t.step.fill_(step0 + s + 1)
            t.clip_adam_advanced(max_norm, 1.0 / W)
            assert torch.equal(_bits(t.grad), _bits(bucket)) and float(t.step) == step0 + s + 1      # both left as delivered
            wg = 0.0
        else:
            t.clip_adam(max_norm, 1.0 / W)
            assert float(t.step) == step0 + s + 1                                                    # advanced by exactly 1
            wg = U.worst(_np(t.grad), r["grad_clipped"])
        assert float(t.lr) == float(np.float32(U.LR))
        w = np.maximum(w, [*U.adam_worst(t.state(), r), wg])
        sha = lambda parts: hashlib.sha1(b"".join(x.cpu().numpy().tobytes() for x in parts)).hexdigest()
        digests.append(sha((t.param, t.m, t.v)))
        with_grad.append(sha((t.param, t.m, t.v, t.grad)))
    assert t.guards_hold()
    return w, tuple(digests), tuple(with_grad)


CELLS = [(step0, mn, W) for step0 in U.STARTS for mn in U.NORMS for W in U.WORLDS]


def _against_float64(kernel, n):
    w = np.zeros(4)
    for step0, mn, W in CELLS:
        w = np.maximum(w, _run(kernel, n, step0, mn, W)[0])
    print(f"{kernel} n={n}: worst error / bar over {len(CELLS)} cells x {U.STEPS} steps: parameters {w[0]:.4f} exp_avg {w[1]:.4f} exp_avg_sq {w[2]:.4f}"
          + (f" clipped gradient {w[3]:.4f}" if kernel == "k8" else ""))
    assert (w <= 1.0).all()


@pytest.mark.parametrize("n", U.K8_N)
def test_clip_adam_against_float64(n):
    """K8, every max_norm / start / grad_scale cell, four steps: parameters, both moments and the clipped, scaled gradient it writes
    into grad after every step; the counter advanced by exactly 1 per call"""
    _against_float64("k8", n)


@pytest.mark.parametrize("n", U.K12M_N)
def test_clip_adam_advanced_against_float64(n):
    """K12m likewise; grad and step_count are left bit-identical (include/ppocar.h)"""
    _against_float64("k12m", n)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", U.PROBE_N)
def test_every_element_is_counted_in_the_norm(n, shift):
    """K12m's norm pass: 1e-3 N(0, 1) with one spike of 3.0 at k -- the ends of the first float4, of a thread's first stride, of the
    first pass of 16 x 256 float4, of the vector part, and the scalar tail for n % 4.  Counted, the norm is 3.0 and the clip acts
    (coefficient 0.166); left out, 0.15 and idle: exp_avg[k], exp_avg_sq[k] are then 1e4 x their bars away (host test).  shift = 1: the
    bucket lies 4 bytes past a 16-byte boundary and the whole norm goes through the scalar loop."""
    p, z = U.probe_params(n), torch.zeros(n)
    worst = np.zeros(3)
    for k in U.probe_positions(n):
        b = U.probe_bucket(n, k)
        r = U.clip_adam_steps(p, z, z, 0, [b], 0.5, 1.0)[0]
        t = Tail.for_adam(p, z, z, 1, grad=b, shift=shift).clip_adam_advanced(0.5, 1.0)
        assert t.grad.data_ptr() % 16 == 4 * shift
        got = t.state()
        am, av = U.moment_allowances(r["grad_clipped"])
        assert abs(got[1][k] - r["exp_avg"][k]) <= am[k] and abs(got[2][k] - r["exp_avg_sq"][k]) <= av[k], k
        worst = np.maximum(worst, U.adam_worst(got, r))
        assert t.guards_hold()
    print(f"n={n} shift={shift}: worst error / bar over the spike's positions: parameters {worst[0]:.4f} exp_avg {worst[1]:.4f} exp_avg_sq {worst[2]:.4f}")
    assert (worst <= 1.0).all()


# ---- bit-level invariants -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(set(U.K8_N + U.K12M_N)))
def test_idle_clip_k8_and_k12m_give_the_same_bits(n):
    """max_norm 1e9: coef == 1.0f whatever the order of the norm's sum, and from there K8 (counter s, which it advances) and K12m
    (counter s + 1) run the same operations: parameters and moments bit for bit after every step, at every start and grad_scale"""
    for step0 in U.STARTS:
        for W in U.WORLDS:
            a, b = _run("k8", n, step0, 1e9, W)[1], _run("k12m", n, step0, 1e9, W)[1]
            assert len(a) == len(b) == U.STEPS and a == b, (step0, W)


@pytest.mark.parametrize("kernel,n", [("k8", n) for n in U.K8_N] + [("k12m", n) for n in U.K12M_N])
def test_a_power_of_two_scale_gives_the_same_bits(kernel, n):
    """bucket W with grad_scale 1 / W, W = 2, 8: the bits of the bucket with grad_scale 1 (no gradient element is a denormal: host test),
    clip acting and idle, from either start, after every step (K8: the gradient it writes back too)"""
    for step0 in U.STARTS:
        for mn in U.NORMS:
            one = _run(kernel, n, step0, mn, 1)[2 if kernel == "k8" else 1]      # (K12m leaves the bucket, which differs by W)
            for W in (2, 8):
                assert _run(kernel, n, step0, mn, W)[2 if kernel == "k8" else 1] == one, (step0, mn, W)


@pytest.mark.parametrize("kernel,n", [("k8", 1025), ("k8", 23050), ("k12m", 257), ("k12m", 16387), ("k12m", 23050)])
def test_clip_adam_gives_the_same_bits_wherever_the_buffers_lie(kernel, n):
    """Every buffer 16 bytes further into its allocation: the same bits.  4 bytes further: K8 walks the bucket element by element
    either way, the same bits; K12m sums the norm through its scalar loop instead of 16-byte vectors -- another order, so the same bits
    where coef == 1.0f (idle clip) and the float64 bars where the clip acts."""
    for mn in U.NORMS:
        base = _run(kernel, n, 7, mn, 2)[2]
        assert _run(kernel, n, 7, mn, 2, shift=4)[2] == base, mn
        w, _, off = _run(kernel, n, 7, mn, 2, shift=1)
        assert (w <= 1.0).all()
        if kernel == "k8" or mn == 1e9:
            assert off == base, mn


def _dev(c):
    return tuple(c[k].cuda().contiguous() for k in DATA), [ix.cuda() for ix in c["idx"]]


def _advanced(call, max_norm, grad_scale=1.0):
    _capi.check(lib.pc_clip_adam_advanced(0, call.param.data_ptr(), call.grad.data_ptr(), call.m.data_ptr(), call.v.data_ptr(),
                                          call.step.data_ptr(), call.lr.data_ptr(), call.param.numel(), max_norm, grad_scale, U.BETA1,
                                          U.BETA2, U.EPS, torch.cuda.current_stream().cuda_stream), "pc_clip_adam_advanced")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", R.APPLIED, ids=sid)
def test_apply_2_then_the_exchange_step_is_apply_1(shape):
    """pc_ppo_minibatch(apply = 1) against apply = 2 followed by pc_clip_adam_advanced(grad_scale = 1) over four steps.  Idle clip: K12
    and K12m share adam_coef / adam_elem and coef == 1.0f: parameters, moments, counter and metrics bit for bit.  max_norm 0.5: K12 sums
    the norm from K11's partials, K12m over the bucket -- the two-launch route is held to the float64 trajectory at the project's bars."""
    for mn in (1e9, 0.5):
        c = R.case(*shape, 1.0, 4, mn)
        data, idx = _dev(c)
        one, two = Call(c["p0"].cuda(), *shape, max_norm=mn), Call(c["p0"].cuda(), *shape, max_norm=mn)
        for s, r in enumerate(c["ref"]):
            one.ppo(idx[s], *data, apply=1)
            two.ppo(idx[s], *data, apply=2)
            raw = two.grad.clone()
            _advanced(two, mn)
            assert torch.equal(two.grad, raw) and float(two.step) == s + 1.0
            if mn == 1e9:
                for k in ("param", "m", "v", "step", "metrics"):
                    assert torch.equal(getattr(one, k), getattr(two, k)), (s, k)
            err = float(np.abs(_np(two.param) - r["param"]).max())
            print(f"{sid(shape)} max_norm {mn:g} step {s + 1}: apply = 2 + pc_clip_adam_advanced, parameters max abs err {err:.3e}")
            assert err <= R.PARAM_ATOL
            if s == 0:
                am, av = U.moment_allowances(r["grad_clipped"])
                assert (np.abs(_np(two.m) - r["exp_avg"]) <= am).all() and (np.abs(_np(two.v) - r["exp_avg_sq"]) <= av).all()


@pytest.mark.parametrize("W", [2, 8])
def test_summed_ranks_against_the_float64_mean(W):
    """W float32 gradients (apply = 0 on W minibatches of one case at the same parameters) added on the device in rank order, then
    pc_clip_adam_advanced(grad_scale = 1 / W), against the float64 mean of the float64 gradients, clipped and stepped"""
    shape = (256, 23, 9)
    c = R.case(*shape, 1.0, W)
    data, idx = _dev(c)
    bucket = torch.zeros(R.n_param(*shape[1:]), device="cuda")
    for ix in idx:
        bucket += Call(c["p0"].cuda(), *shape).ppo(ix, *data, apply=0).grad
    mean = np.mean([R.gradient_of(dict(c, idx=[ix])) for ix in c["idx"]], 0)
    z = torch.zeros_like(c["p0"])
    r = U.clip_adam_steps(c["p0"], z, z, 0, [mean], R.MAX_NORM, 1.0)[0]
    assert r["norm"] > R.MAX_NORM
    t = Tail.for_adam(c["p0"], z, z, 1, grad=bucket.cpu()).clip_adam_advanced(R.MAX_NORM, 1.0 / W)
    w = U.adam_worst(t.state(), r)
    print(f"W={W}: worst error / bar: parameters {w[0]:.4f} exp_avg {w[1]:.4f} exp_avg_sq {w[2]:.4f}; the summed bucket / W against the "
          f"float64 mean: {U.worst(_np(bucket) / W, mean):.3f} of the gradient's allowance")
    assert max(w) <= 1.0 and t.guards_hold()
    assert np.abs(r["param"] - c["p0"].double().numpy()).max() > 1e-4


# ---- the learner's two paths, end to end --------------------------------------------------------------------------------------------
def _learner(c, max_norm, **kw):
    from ppo_car_amd.ppo import PPOConfig, PPOLearner
    B = c["B"]
    cfg = PPOConfig(n_envs=8, n_steps=B, batch_size=B, train_iters=1, use_graphs=False, max_grad_norm=max_norm, clip_ratio=R.CLIP,
                    vf_coef=R.VF, ent_coef=R.EC, learning_rate=R.LR, **kw)
    return PPOLearner(R._agent_as(c, torch.float32).cuda(), cfg, "cuda")


def _four_steps(L, step, c, grad_key):
    data, idx = _dev(c)
    before = np.zeros(4)
    for s, r in enumerate(c["ref"]):
        step(idx[s], *data)
        torch.cuda.synchronize()
        p, g, m = _np(L.flat_param), _np(L.flat_grad), _np(L.metrics)
        print(f"step {s + 1}: parameters max abs err {np.abs(p - r['param']).max():.3e}; {grad_key} worst error / allowance "
              f"{R.worst(g, r[grad_key]):.3f}; metric increments {m - before} reference {r['metrics']}")
        assert np.abs(p - r["param"]).max() <= R.PARAM_ATOL
        assert np.allclose(g, r[grad_key], rtol=R.GRAD_RTOL, atol=R.GRAD_ATOL)
        assert float(L.step_count) == s + 1.0
        _metrics_hold(m - before, r["metrics"])
        before = m
        if s == 0:
            am, av = U.moment_allowances(r["grad_clipped"])
            assert (np.abs(_np(L.exp_avg) - r["exp_avg"]) <= am).all() and (np.abs(_np(L.exp_avg_sq) - r["exp_avg_sq"]) <= av).all()


@pytest.mark.parametrize("max_norm", [0.5, 1e9])
@pytest.mark.parametrize("shape", [(2, 23, 9), (65, 25, 2), (1024, 40, 16)], ids=sid)
def test_fused_path_four_steps_against_float64(shape, max_norm):
    """PPOLearner(custom_mlp = False).fused_minibatch_step: K6, torch's GEMMs, K7, autograd, K8 -- the update of every agent off the
    hand-written menu (A = 16 among them) -- against the float64 trajectory: parameters, the clipped gradient K8 leaves in flat_grad,
    the metric increments, the counter after every step, the moments after the first"""
    c = R.case(*shape, 1.0, 4, max_norm)
    L = _learner(c, max_norm, custom_mlp=False)
    assert L.path == "fused" and not L.collective
    L._fused_alloc(*shape[1:])
    _four_steps(L, L.fused_minibatch_step, c, "grad_clipped")


@contextlib.contextmanager
def _one_rank_group():
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("max_norm", [0.5, 1e9])
@pytest.mark.parametrize("shape", [(9, 39, 9), (256, 23, 9)], ids=sid)
def test_exchange_path_four_steps_against_float64(shape, max_norm):
    """PPOLearner(force_collective = True).custom_minibatch_step under a one-rank gloo group: pc_ppo_minibatch(apply = 2), the all-reduce
    (one rank: the identity), K12m -- the multi-rank step as far as one device shows it.  flat_grad keeps the raw gradient."""
    c = R.case(*shape, 1.0, 4, max_norm)
    with _one_rank_group():
        L = _learner(c, max_norm, force_collective=True)
        assert L.path == "custom" and L.collective
        _four_steps(L, L.custom_minibatch_step, c, "grad")
