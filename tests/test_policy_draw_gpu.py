"""GPU tests of the policy step and its draw, element by element: pc_sample (K4) and pc_policy_act (K5, all three draw tails, both
work decompositions, the three arithmetic forms) over the shapes include/ppocar.h declares, against tests/draw_reference.py.

THE EXACT-DRAW CHECK.  The uniform of every element comes from the reference (Philox-4x32-10, the counter layout and the float32
mapping the header states); the float64 CDF is built from the float32 logits the kernel itself reports (pc_sample: was given).  An
element is SAFE when its uniform is further than DELTA = 1e-5 from every inner bin boundary: the project holds its log-probs to
2e-6, so each p_i (<= 1) is within 2e-6 p_i and an inclusive sum of at most 16 of them within 2e-6 plus 16 x 2^-24 ~ 1e-6 of
summation rounding; DELTA leaves about 3 x over that -- a property of the float32 softmax chain, not of the code under test.  Every
safe element's action must equal the reference's.  How many elements are unsafe is a condition on the INPUTS: it is computed from
the reference before anything is launched (for pc_policy_act on the float64 MLP's logits with the margin widened to 2 DELTA, which
covers the 4e-6 the kernel's logits may differ by), must be at most floor(N / 1000) -- zero below 1000 elements; seeds are picked
from a fixed list so that it holds -- and is printed.

One more input condition, for rows whose LAST action has probability zero: the float32 CDF can end a few ulp below 1, and a uniform
in [cdf_last, 1) then lands in the last bin ("the last bin absorbs rounding", DESIGN.md section 5 has the exposure); such an element
has its uniform within DELTA of 1, is counted before the launch, and the inputs are chosen so that there is none."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import draw_reference as ref
import ppo_car_amd as pc
from ppo_car_amd._capi import PC_ERR_UNSUPPORTED, check, lib

pytestmark = pytest.mark.gpu

DELTA = 1e-5
GUARD = 64                    # elements of guard in front of and behind every output
SEEDS = (1, 2 ** 32 + 5, 2 ** 63 + 11)
OFFSETS = (0, 1, 2, 3, 4, 7, 2 ** 32 + 1, 2 ** 34 + 3)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Guarded:
    """an output of n elements with GUARD sentinel elements on each side"""

    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.ptr = self.full.data_ptr() + GUARD * self.full.element_size()

    def get(self, what):
        full = self.full.cpu().numpy()
        assert np.all(full[:GUARD] == self.fill) and np.all(full[GUARD + self.n:] == self.fill), f"{what}: written outside its {self.n} elements"
        return full[GUARD:GUARD + self.n]


def _categorical_f64(logits):
    d = torch.distributions.Categorical(logits=torch.from_numpy(np.asarray(logits, dtype=np.float64)))
    return d.logits.numpy(), d.entropy().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# pc_sample
# ---------------------------------------------------------------------------------------------------------------------------
def _logit_rows(n, A, rng_seed):
    """float32 rows: random (scale 3); by row index mod 32: 1 all equal, 2 one dominant (+100 / -100), 3 and 4 rows with -inf
    entries (3: anywhere, 4: a trailing run), the rest random"""
    rng = np.random.default_rng(rng_seed)
    L = (rng.standard_normal((n, A)) * 3.0).astype(np.float32)
    i = np.arange(n)
    L[i % 32 == 1] = np.float32(0.7)
    dom = np.flatnonzero(i % 32 == 2)
    L[dom] = -100.0
    L[dom, dom % A] = 100.0
    if A > 1:
        holes = rng.random((n, A)) < 0.3
        holes[i, rng.integers(0, A, n)] = False                 # a finite logit in every row
        holes[i % 32 != 3] = False
        L[holes] = -np.inf
        tail = np.flatnonzero(i % 32 == 4)
        keep = rng.integers(1, A, len(tail))                    # the first `keep` logits stay
        L[tail[:, None], np.arange(A)[None, :]] = np.where(np.arange(A)[None, :] < keep[:, None], L[tail], -np.inf)
    return L


def _plan_sample(L, seed, offset, what):
    """the reference's draw for logits L [n][A] (element i = row i of THIS call) and the input conditions, before any launch"""
    n, A = L.shape
    u = ref.uniform(seed, offset, np.arange(n, dtype=np.uint64))
    act, logp, ent, margin = ref.draw_f64(L, u)
    safe = margin > DELTA
    unsafe = int(n - safe.sum())
    exposed = int(((np.exp(logp[:, -1]) < 1e-30) & (u >= 1.0 - DELTA)).sum()) if A > 1 else 0
    print(f"{what}: N {n} A {A} seed {seed} offset {offset}: {unsafe} unsafe elements (allowed {n // 1000}), {exposed} exposed to the CDF's end")
    assert unsafe <= n // 1000 and exposed == 0, "a condition on the test's inputs: pick another seed"
    return {"L": L, "u": u, "act": act, "logp": logp, "ent": ent, "safe": safe}


def _run_sample(L_dev, n, A, seed, offset, row0=0, entropy=True):
    act, lp, ent = _Guarded(n, torch.int64, -7), _Guarded(n, torch.float32, 1234.5), _Guarded(n, torch.float32, 1234.5)
    check(lib.pc_sample(0, L_dev.data_ptr() + 4 * A * row0, n, A, seed, offset, act.ptr, lp.ptr, ent.ptr if entropy else None, _stream()),
          "pc_sample")
    torch.cuda.synchronize()
    return act.get("actions"), lp.get("logprob"), ent.get("entropy")


def _verify_sample(plan, act, lp, ent, what):
    L, safe = plan["L"], plan["safe"]
    n, A = L.shape
    i = np.arange(n)
    assert act.min() >= 0 and act.max() <= A - 1, what
    bad = np.flatnonzero(safe & (act != plan["act"]))
    assert len(bad) == 0, f"{what}: {len(bad)} safe elements drew another action than the reference, first {bad[:5]}: got {act[bad[:5]]}, want {plan['act'][bad[:5]]}"
    assert np.all(np.isfinite(L[i, act])), f"{what}: an action of probability 0 was drawn"
    cat_logp, cat_ent = _categorical_f64(L)
    special = (np.abs(L) >= 100.0).any(axis=1)                      # dominant and -inf rows: the extreme-logit tolerance
    err = np.abs(lp.astype(np.float64) - cat_logp[i, act])
    e_ord, e_spc = float(err[~special].max(initial=0.0)), float(err[special].max(initial=0.0))
    e_ent = float(np.abs(ent.astype(np.float64) - cat_ent).max()) if ent is not None else 0.0
    print(f"{what}: log-prob error {e_ord:.2e} (extreme rows {e_spc:.2e}), entropy error {e_ent:.2e}")
    assert e_ord < 2e-6 and e_spc < 5e-6, what
    if ent is not None:
        assert np.all(np.isfinite(ent)) and e_ent < 5e-6, what
        assert np.abs(plan["ent"] - cat_ent).max() < 1e-12


# every value of A, N, SEEDS and OFFSETS occurs, every A with a ragged N
SAMPLE_CASES = [(1, 63, 0, 0), (1, 100003, 1, 1), (2, 257, 2, 2), (2, 64, 0, 3), (3, 65, 1, 4), (3, 100003, 0, 6),
                (8, 1, 2, 5), (8, 100003, 1, 7), (9, 100003, 2, 6), (9, 63, 1, 0), (15, 257, 0, 7), (15, 64, 2, 1),
                (16, 65, 1, 3), (16, 100003, 0, 2), (16, 1, 0, 4), (9, 257, 0, 5)]


def test_sample_cases_cover_every_listed_value():
    assert {c[0] for c in SAMPLE_CASES} == {1, 2, 3, 8, 9, 15, 16} and {c[1] for c in SAMPLE_CASES} == {1, 63, 64, 65, 257, 100003}
    assert {c[2] for c in SAMPLE_CASES} == {0, 1, 2} and {c[3] for c in SAMPLE_CASES} == set(range(len(OFFSETS)))
    for A in (1, 2, 3, 8, 9, 15, 16):
        assert any(c[0] == A and c[1] % 64 for c in SAMPLE_CASES)


@pytest.mark.parametrize("A,N,si,oi", SAMPLE_CASES)
def test_sample_draws_the_reference_action_element_by_element(A, N, si, oi):
    seed, offset = SEEDS[si], OFFSETS[oi]
    L = _logit_rows(N, A, 100 * A + oi)
    plan = _plan_sample(L, seed, offset, "pc_sample")
    act, lp, ent = _run_sample(torch.from_numpy(L).cuda(), N, A, seed, offset)
    _verify_sample(plan, act, lp, ent, f"pc_sample A {A} N {N}")
    act2, lp2, _ = _run_sample(torch.from_numpy(L).cuda(), N, A, seed, offset, entropy=False)     # entropy = NULL
    assert np.array_equal(act, act2) and np.array_equal(lp, lp2)


def test_sample_rejects_more_than_16_actions():
    L = torch.zeros(4, 17, device="cuda")
    act, lp = _Guarded(4, torch.int64, -7), _Guarded(4, torch.float32, 1234.5)
    assert lib.pc_sample(0, L.data_ptr(), 4, 17, 1, 0, act.ptr, lp.ptr, None, _stream()) == PC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.all(act.get("actions") == -7) and np.all(lp.get("logprob") == 1234.5)


@pytest.mark.parametrize("A,seed,offset", [(9, 2 ** 32 + 5, 2 ** 32 + 1), (3, 1, 7), (16, 2 ** 63 + 11, 2)])
def test_sample_element_depends_on_seed_offset_and_its_index_only(A, seed, offset):
    """The draw of element i at offset o depends on nothing else: the same rows permuted, a truncated N and a call that starts at a
    base pointer inside the buffer each follow (seed, offset, index IN THAT CALL) -- which a chi-square over one row cannot see."""
    N = 100003
    L = _logit_rows(N, A, 7 * A)
    Ld = torch.from_numpy(L).cuda()
    plan = _plan_sample(L, seed, offset, "whole")
    act, lp, ent = _run_sample(Ld, N, A, seed, offset)
    _verify_sample(plan, act, lp, ent, "whole")
    # truncated: the same rows at the same indices -- every bit, safe or not
    for n in (1, 4097):
        a2, lp2, e2 = _run_sample(Ld, n, A, seed, offset)
        assert np.array_equal(a2, act[:n]) and np.array_equal(lp2, lp[:n]) and np.array_equal(e2, ent[:n])
    # permuted rows: element i now holds another row, and draws with ITS OWN uniform
    perm = np.random.default_rng(5).permutation(N)
    Lp = np.ascontiguousarray(L[perm])
    planp = _plan_sample(Lp, seed, offset, "permuted")
    ap, lpp, ep = _run_sample(torch.from_numpy(Lp).cuda(), N, A, seed, offset)
    _verify_sample(planp, ap, lpp, ep, "permuted")
    assert np.array_equal(planp["u"], plan["u"])
    # a slice that starts 4099 rows into the buffer: its first row is element 0 of that call
    row0, n = 4099, 50001
    plans = _plan_sample(L[row0:row0 + n], seed, offset, "slice")
    a3, lp3, e3 = _run_sample(Ld, n, A, seed, offset, row0=row0)
    _verify_sample(plans, a3, lp3, e3, "slice")
    # and the next offset is another draw altogether
    a4, _, _ = _run_sample(Ld, N, A, seed, offset + 1)
    assert (a4 != act).mean() > 0.2 if A > 1 else True


# ---------------------------------------------------------------------------------------------------------------------------
# pc_policy_act
# ---------------------------------------------------------------------------------------------------------------------------
KEYS = ("actor.0.weight", "actor.0.bias", "actor.2.weight", "actor.2.bias", "critic.0.weight", "critic.0.bias", "critic.2.weight", "critic.2.bias")
N_MAX = 3 * 65536 + 17


@functools.lru_cache(maxsize=None)
def _weights(D, A):
    """as test_fused_policy_kernel_matches_torch_mlp: the default init plus 0.1 randn, so biases and output weights are not trivial"""
    torch.manual_seed(1000 * D + A)
    agent = pc.Agent(D, A)
    with torch.no_grad():
        for p in agent.parameters():
            p.add_(torch.randn_like(p) * 0.1)
    return {k: v.detach().clone().contiguous() for k, v in agent.state_dict().items()}


@functools.lru_cache(maxsize=4)
def _inputs(D, A, n):
    """observations [n][D] and the float64 MLP's logits and values for them"""
    obs = (np.random.default_rng(D * 31 + A).random((n, D)) * 2.0 - 0.5).astype(np.float32)
    L64, V64 = ref.mlp_f64({k: v.numpy() for k, v in _weights(D, A).items()}, obs)
    return obs, L64, V64


class _Policy:
    """a pc_policy handle and its packed image, sized from what pc_policy_get reports and nothing larger"""

    def __init__(self, D, A, prec, split, weights):
        self.D, self.A = D, A
        self.h = C.c_void_p()
        check(lib.pc_policy_create(0, D, 256, A, prec, split, C.byref(self.h)), "pc_policy_create")
        pr, sp, n = C.c_int(), C.c_int(), C.c_int64()
        check(lib.pc_policy_get(self.h, C.byref(pr), C.byref(sp), C.byref(n)), "pc_policy_get")
        self.prec, self.split, self.image_floats = pr.value, sp.value, n.value
        self.image = torch.empty(self.image_floats, device="cuda")
        w = [weights[k].cuda() for k in KEYS]
        check(lib.pc_policy_pack(self.h, *[t.data_ptr() for t in w], self.image.data_ptr(), _stream()), "pc_policy_pack")
        torch.cuda.synchronize()

    def act(self, obs_dev, N, seed, offset, offset_dev=None, logits=True, action_f=True):
        A = self.A
        out = {"action": _Guarded(N, torch.int64, -7), "action_f32": _Guarded(N, torch.float32, 1234.5), "logprob": _Guarded(N, torch.float32, 1234.5),
               "value": _Guarded(N, torch.float32, 1234.5), "logits": _Guarded(N * A, torch.float32, 1234.5)}
        check(lib.pc_policy_act(self.h, obs_dev.data_ptr(), N, self.image.data_ptr(), seed, offset,
                                offset_dev.data_ptr() if offset_dev is not None else None, out["action"].ptr,
                                out["action_f32"].ptr if action_f else None, out["logprob"].ptr, out["value"].ptr,
                                out["logits"].ptr if logits else None, _stream()), "pc_policy_act")
        torch.cuda.synchronize()
        res = {k: g.get(k) for k, g in out.items()}
        res["logits"] = res["logits"].reshape(N, A)
        if not logits:
            assert np.all(res["logits"] == 1234.5)
        return res

    def close(self):
        lib.pc_policy_destroy(self.h)
        self.h = None


SEED_LIST = tuple(2 ** 32 + 5 + 1000 * k for k in range(16))


def _plan_policy(D, A, N, offset, what, n_inputs=None):
    """the first seed of SEED_LIST whose unsafe-element count -- on the float64 MLP's logits, margin 2 DELTA -- is within the bound:
    decided from the reference alone, before any launch"""
    obs, L64, V64 = _inputs(D, A, n_inputs or N)
    L64, V64 = L64[:N], V64[:N]
    idx = np.arange(N, dtype=np.uint64)
    for seed in SEED_LIST:
        u = ref.uniform(seed, offset, idx)
        _, _, _, margin = ref.draw_f64(L64, u)
        safe = margin > 2 * DELTA
        unsafe = int(N - safe.sum())
        if unsafe <= N // 1000:
            print(f"{what}: D {D} A {A} N {N} seed {seed} offset {offset}: {unsafe} unsafe elements (allowed {N // 1000})")
            return {"obs": obs[:N], "L64": L64, "V64": V64, "u": u, "safe": safe, "seed": seed, "offset": offset, "unsafe": unsafe}
    raise AssertionError(f"{what}: no seed of the list meets the input condition")


def _verify_policy(plan, res, A, what):
    L64, V64, u, safe = plan["L64"], plan["V64"], plan["u"], plan["safe"]
    N = len(u)
    i = np.arange(N)
    logits, act = res["logits"], res["action"]
    mag = max(1.0, float(np.abs(L64).max()))
    e_l = float(np.abs(logits.astype(np.float64) - L64).max()) / mag
    e_v = float(np.abs(res["value"].astype(np.float64) - V64).max()) / mag
    assert act.min() >= 0 and act.max() <= A - 1, what
    ref_act, logp, _, _ = ref.draw_f64(logits, u)              # the CDF of the float32 logits the kernel reports
    e_lp = float(np.abs(res["logprob"].astype(np.float64) - logp[i, act]).max())
    print(f"{what}: logit error {e_l:.2e}, value error {e_v:.2e} (relative to {mag:.2f}), log-prob error {e_lp:.2e}")
    assert e_l < 4e-6 and e_v < 4e-6, what
    assert e_lp < 2e-6, what
    bad = np.flatnonzero(safe & (act != ref_act))
    assert len(bad) == 0, f"{what}: {len(bad)} safe elements drew another action than the reference, first {bad[:5]}: got {act[bad[:5]]}, want {ref_act[bad[:5]]}"
    assert np.array_equal(res["action_f32"], act.astype(np.float32)), what


@pytest.mark.parametrize("A", [1, 2, 4, 5, 8, 9, 10, 12, 15])
@pytest.mark.parametrize("D", [1, 4, 8, 20, 21, 24, 25, 32, 33, 40])
def test_policy_act_shapes(D, A):
    """Every (D, A) of the lists x requested precision {0, 1, 2} x split {0, 1} at N = 257: the three draw tails (pair: A = 9 unsplit;
    generic: every other A unsplit; row: split), the value's place in output row A (A & 3 and A >> 2 take every value), the K-step
    boundaries of D, and the demotion of A > 9 to precision 0."""
    N = 257
    plan = _plan_policy(D, A, N, 2 ** 32 + 1 + (A & 3), "shapes")
    obs_dev = torch.from_numpy(plan["obs"]).cuda()
    for prec in (0, 1, 2):
        for split in (0, 1):
            pol = _Policy(D, A, prec, split, _weights(D, A))
            try:
                assert pol.prec == (0 if A > 9 else prec) and pol.split == split
                what = f"D {D} A {A} precision {prec} split {split}"
                res = pol.act(obs_dev, N, plan["seed"], plan["offset"])
                _verify_policy(plan, res, A, what)
                res2 = pol.act(obs_dev, N, plan["seed"], plan["offset"], logits=False)          # logits_out = NULL: the same bits
                for k in ("action", "action_f32", "logprob", "value"):
                    assert np.array_equal(res[k], res2[k]), (what, k)
            finally:
                pol.close()


SIZES = [(1, -1), (15, -1), (31, -1), (33, -1), (255, -1), (8192, -1), (8193, -1),
         (8192 + 40, 1),            # 258 chunks of 32 on 256 workgroups: the chunk loop iterates, the last chunk is ragged
         (65536 + 300, 0),          # 258 chunks of 256
         (3 * 65536 + 17, 0)]


@pytest.mark.parametrize("D,A", [(23, 9), (23, 5), (40, 15), (1, 1)])
def test_policy_act_sizes(D, A):
    """N below one tile, next to the automatic-split bound, and sizes at which the grid-stride loop of policy_kernel makes a second and
    a third trip (sOut reused behind the barrier, ragged last chunk), in each precision the shape can get; outputs past N untouched."""
    for N, split in SIZES:
        plan = _plan_policy(D, A, N, 5, "sizes", n_inputs=N_MAX)
        obs_dev = torch.from_numpy(np.ascontiguousarray(plan["obs"])).cuda()
        for prec in ((0,) if A > 9 else (0, 1, 2)):
            pol = _Policy(D, A, prec, split, _weights(D, A))
            try:
                assert pol.prec == prec
                res = pol.act(obs_dev, N, plan["seed"], plan["offset"])
                _verify_policy(plan, res, A, f"D {D} A {A} precision {prec} N {N} split {split}")
            finally:
                pol.close()


@pytest.mark.parametrize("D,A", [(23, 9), (23, 5)])
def test_policy_act_split_and_unsplit_both_draw_the_reference(D, A):
    """the two work decompositions differ in the last bits of the logits (include/ppocar.h), so each is held to the reference on its
    own logits, not to the other"""
    N = 8192 + 40
    plan = _plan_policy(D, A, N, 3, "split 0 / 1", n_inputs=N_MAX)
    obs_dev = torch.from_numpy(np.ascontiguousarray(plan["obs"])).cuda()
    for prec in (0, 1, 2):
        for split in (0, 1):
            pol = _Policy(D, A, prec, split, _weights(D, A))
            try:
                _verify_policy(plan, pol.act(obs_dev, N, plan["seed"], plan["offset"]), A, f"D {D} A {A} precision {prec} split {split}")
            finally:
                pol.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the stream
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(1, 2), (3, 1), (2 ** 32, 2), (2, 2 ** 32)])
@pytest.mark.parametrize("split", [0, 1])
def test_policy_act_offset_and_offset_dev_add(a, b, split):
    """(offset = a, *offset_dev = b) is (a + b, NULL), bit for bit: a + b in {3, 4, 2^32 + 2}"""
    D, A, N = 23, 9, 1000
    obs, _, _ = _inputs(D, A, N_MAX)
    obs_dev = torch.from_numpy(np.ascontiguousarray(obs[:N])).cuda()
    dev = torch.tensor([b], dtype=torch.int64, device="cuda")          # (the 64 bits of a uint64 below 2^63)
    pol = _Policy(D, A, 2, split, _weights(D, A))
    try:
        r1 = pol.act(obs_dev, N, 2 ** 63 + 11, a, offset_dev=dev)
        r2 = pol.act(obs_dev, N, 2 ** 63 + 11, a + b)
        r3 = pol.act(obs_dev, N, 2 ** 63 + 11, a)
    finally:
        pol.close()
    for k in r1:
        assert np.array_equal(r1[k], r2[k]), k
    assert int(dev.item()) == b and (r3["action"] != r1["action"]).mean() > 0.2


@pytest.mark.parametrize("prec,split", [(0, 0), (2, 0), (2, 1), (1, 1)])
@pytest.mark.parametrize("D,A,offset", [(23, 9, 6), (23, 5, 2 ** 32 + 1)])
def test_policy_act_and_sample_share_one_stream(D, A, offset, prec, split):
    """pc_policy_act(offset = o), then pc_sample on its own logits_out with the same (seed, o): the same action on EVERY safe element
    (the fused step's three tails and K4 sum their float32 CDFs in different orders, nothing else)"""
    N = 8192 + 40
    plan = _plan_policy(D, A, N, offset, "one stream", n_inputs=N_MAX)
    obs_dev = torch.from_numpy(np.ascontiguousarray(plan["obs"])).cuda()
    pol = _Policy(D, A, prec, split, _weights(D, A))
    try:
        res = pol.act(obs_dev, N, plan["seed"], offset)
    finally:
        pol.close()
    _verify_policy(plan, res, A, f"D {D} A {A} precision {prec} split {split}")
    act, lp, _ = _run_sample(torch.from_numpy(np.ascontiguousarray(res["logits"])).cuda(), N, A, plan["seed"], offset)
    differ = np.flatnonzero(act != res["action"])
    print(f"pc_policy_act vs pc_sample: {len(differ)} of {N} elements differ, {int(plan['safe'][differ].sum())} of them safe")
    assert not plan["safe"][differ].any()
    same = act == res["action"]
    assert np.abs(lp[same] - res["logprob"][same]).max() < 2e-6


# ---------------------------------------------------------------------------------------------------------------------------
# the element whose word has all its top 24 bits set
# ---------------------------------------------------------------------------------------------------------------------------
# (seed 9; tests/test_policy_draw_host.py::test_the_stream_has_all_ones_words_at_the_known_elements).  ((float)k + 0.5f) * 2^-24 is 1.0f
# for k = 2^24 - 1: unclamped, `u < cdf` is false for every bin and the last action comes back whatever its probability -- here
# action 1 of logits [0, -200], log-prob -200.
@pytest.mark.parametrize("offset,N,hot", [(0, 3677981, 3677980), (2, 9871915, 9871914)])
def test_all_ones_word_never_draws_the_impossible_action_sample(offset, N, hot):
    L = torch.zeros(N, 2, device="cuda")
    L[:, 1] = -200.0
    act = torch.full((N,), -7, dtype=torch.int64, device="cuda")
    lp = torch.full((N,), 1234.5, device="cuda")
    check(lib.pc_sample(0, L.data_ptr(), N, 2, 9, offset, act.data_ptr(), lp.data_ptr(), None, _stream()), "pc_sample")
    torch.cuda.synchronize()
    ones = torch.nonzero(act != 0).view(-1).cpu().numpy()
    print(f"pc_sample seed 9 offset {offset}: element {hot}: action {int(act[hot])}, log-prob {float(lp[hot])}; elements with another action than 0: {ones[:8]}")
    assert len(ones) == 0 and float(lp.abs().max()) == 0.0


@pytest.mark.parametrize("prec", [0, 1, 2])
def test_all_ones_word_never_draws_the_impossible_action_policy_act(prec):
    """the same logits through pc_policy_act: zero output weights, output bias [0, -200] (D = 4, A = 2, unsplit: the generic tail)"""
    N, hot = 3677981, 3677980
    torch.manual_seed(0)
    w = {k: v.clone() for k, v in _weights(4, 2).items()}
    w["actor.2.weight"].zero_()
    w["actor.2.bias"].copy_(torch.tensor([0.0, -200.0]))
    obs = torch.rand(N, 4, device="cuda")
    pol = _Policy(4, 2, prec, 0, w)
    act = torch.full((N,), -7, dtype=torch.int64, device="cuda")
    lp = torch.full((N,), 1234.5, device="cuda")
    val = torch.empty(N, device="cuda")
    try:
        check(lib.pc_policy_act(pol.h, obs.data_ptr(), N, pol.image.data_ptr(), 9, 0, None, act.data_ptr(), None, lp.data_ptr(), val.data_ptr(),
                                None, _stream()), "pc_policy_act")
        torch.cuda.synchronize()
    finally:
        pol.close()
    ones = torch.nonzero(act != 0).view(-1).cpu().numpy()
    print(f"pc_policy_act precision {prec} seed 9 offset 0: element {hot}: action {int(act[hot])}, log-prob {float(lp[hot])}; elements with another action than 0: {ones[:8]}")
    assert len(ones) == 0 and float(lp.abs().max()) == 0.0
