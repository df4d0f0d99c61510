"""The cross-entropy planner, the parts that need no GPU: the C-ABI's symbols and argument checks, the plain reference
(cem_reference.py) held to its own rules on hand-made inputs, the input conditions of the driven rows on the CPU oracle with their
stored counts, CEMPlanner's constructor and evaluate.py's --planner cem options."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ppo_car_amd import _capi
from conftest import ROOT
import cem_reference as X
import draw_reference as D
from test_sequences_host import OLD_NAMESPACE

INV = _capi.PC_ERR_INVALID_ARG
P = 4096      # a non-NULL address: every refused call below is refused before any device call, so it is never dereferenced
NO_DEVICE = 12345      # a device index no machine has

SAMPLE_ARGS = ("device", "weights", "M", "H", "K", "seed", "offset", "const_columns", "keep", "active", "table", "stream")
REFIT_ARGS = ("device", "weights", "ret", "table", "M", "H", "K", "E", "shift", "w_min", "active", "best_seq", "stream")


def test_symbols_exported_with_signatures():
    lib = C.CDLL(_capi.lib_path())
    for name in ("pc_cem_sample", "pc_cem_refit"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.EXPORTS
    vp, i, i64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
    f = _capi.lib.pc_cem_sample
    assert f.restype is i and list(f.argtypes) == [i, vp, i64, i, i, u64, u64, i, vp, vp, vp, vp] and len(f.argtypes) == len(SAMPLE_ARGS)
    g = _capi.lib.pc_cem_refit
    assert g.restype is i and list(g.argtypes) == [i, vp, vp, vp, i64, i, i, i, i, i, vp, vp, vp] and len(g.argtypes) == len(REFIT_ARGS)
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    assert re.search(r"int pc_cem_sample\(int device, const uint32_t\* weights, int64_t M, int H, int K, uint64_t seed, uint64_t offset, "
                     r"int const_columns,\s*const uint8_t\* keep, const uint8_t\* active, uint8_t\* table, void\* stream\);", hdr)
    assert re.search(r"int pc_cem_refit\(int device, uint32_t\* weights, const double\* ret, const uint8_t\* table, int64_t M, int H, int K, "
                     r"int E, int shift,\s*int w_min, const uint8_t\* active, uint8_t\* best_seq, void\* stream\);", hdr)
    assert re.search(r"#define PC_CEM_MAX_HORIZON 256\b", hdr) and _capi.PC_CEM_MAX_HORIZON == 256 and _capi.PC_CEM_W_MAX == X.W_MAX
    # the documented rules, and the order of the checks
    for text in ("r = ((uint64_t)x * S) >> 32", "the least a with", "f = (c << 16) / E", "w - (w >> shift) + (f >> shift)",
                 "Checked before any device call, in this order: NULL weights / table", "-0.0 == 0.0"):
        assert text in hdr, text


def _sample(**kw):
    a = {k: P for k in SAMPLE_ARGS}
    a.update(device=NO_DEVICE, M=8, H=12, K=64, seed=1, offset=2, const_columns=1, stream=None)
    a.update(kw)
    return _capi.lib.pc_cem_sample(*[a[k] for k in SAMPLE_ARGS])


def _refit(**kw):
    a = {k: P for k in REFIT_ARGS}
    a.update(device=NO_DEVICE, M=8, H=12, K=64, E=8, shift=1, w_min=64, stream=None)
    a.update(kw)
    return _capi.lib.pc_cem_refit(*[a[k] for k in REFIT_ARGS])


# the documented order: NULL required arrays; M; H; K; (refit) E; shift; w_min.  Alone, and with everything after it wrong as well.
SHAPE_BAD = [dict(M=0), dict(M=-3), dict(H=0), dict(H=-1), dict(H=257), dict(H=1 << 30), dict(K=0), dict(K=-1), dict(K=4097), dict(K=1 << 30),
             dict(M=0, H=0, K=0), dict(H=0, K=0)]


@pytest.mark.parametrize("kw", [dict(weights=None), dict(table=None), dict(weights=None, table=None, M=0, H=0, K=0),
                                dict(table=None, keep=None, active=None)] + SHAPE_BAD + [dict(K=0, keep=None, active=None)])
def test_sample_argument_errors_before_any_device_call(kw):
    assert _sample(**kw) == INV
    assert _sample(device=0, **kw) == INV      # (whatever the device)


@pytest.mark.parametrize("kw", [dict(weights=None), dict(ret=None), dict(table=None), dict(weights=None, ret=None, table=None, M=0, E=0)]
                         + SHAPE_BAD + [dict(E=0), dict(E=-1), dict(E=65), dict(K=10, E=11), dict(shift=-1), dict(shift=17), dict(w_min=-1),
                                        dict(w_min=65537), dict(E=0, shift=17, w_min=-1), dict(shift=17, w_min=-1),
                                        dict(K=0, E=0, active=None, best_seq=None)])
def test_refit_argument_errors_before_any_device_call(kw):
    assert _refit(**kw) == INV
    assert _refit(device=0, **kw) == INV


def test_a_valid_call_reaches_the_device_check():
    """Every argument fine, the optional ones NULL or not, the limits of every number: the call gets as far as the device -- an index no
    machine has -- and answers PC_ERR_NO_DEVICE, not INVALID_ARG.  Still no made-up address is read."""
    for kw in (dict(), dict(keep=None, active=None), dict(M=1, H=1, K=1), dict(H=256, K=4096), dict(const_columns=0), dict(offset=2 ** 64 - 1)):
        assert _sample(**kw) == _capi.PC_ERR_NO_DEVICE, kw
    for kw in (dict(), dict(active=None, best_seq=None), dict(M=1, H=1, K=1, E=1), dict(H=256, K=4096, E=4096), dict(shift=0, w_min=0),
               dict(shift=16, w_min=65536), dict(E=64)):
        assert _refit(**kw) == _capi.PC_ERR_NO_DEVICE, kw
    assert _sample(device=-1) == _capi.PC_ERR_NO_DEVICE and _refit(device=-1) == _capi.PC_ERR_NO_DEVICE


# ---- the reference's own properties ---------------------------------------------------------------------------------------------------
def test_sampled_frequencies_follow_the_weights():
    w = np.zeros((2, 3, 9), np.uint32)
    w[0, 0] = (1, 2, 3, 4, 5, 6, 7, 8, 9)
    w[0, 1] = (0, 0, 30000, 0, 10000, 0, 0, 0, 20000)      # zeros are never drawn
    w[0, 2] = 0                                            # read as nine ones
    w[1, 0] = 70000                                        # read as 65536 each: uniform
    w[1, 1] = (65536, 0, 0, 0, 0, 0, 0, 0, 200000)         # the second one clamped: half and half
    w[1, 2] = (0, 0, 0, 0, 0, 0, 0, 5, 0)                  # one-hot
    K = 4096
    t = X.sample(w, K, seed=9, offset=6, const_columns=False)
    assert t.shape == (2, 3, K) and t.dtype == np.uint8
    want = X.read_weights(w).astype(np.float64)
    want /= want.sum(-1, keepdims=True)
    freq = np.stack([(t == a).mean(-1) for a in range(9)], -1)
    # a bin of probability p over K draws: standard deviation sqrt(p (1 - p) / K) <= 0.0079; five of them
    assert np.abs(freq - want).max() < 5 * np.sqrt(0.25 / K), np.abs(freq - want).max()
    assert (freq[want == 0] == 0).all() and (t[1, 2] == 7).all()
    # the draw is the raw word's: element idx of (seed, offset), whatever lies around it
    idx = (1 * 3 + 1) * K + 77
    x = int(D.philox_words(9, 6, idx)[6 & 3][0])
    assert t[1, 1, 77] == (0 if (x * (2 * 65536)) >> 32 < 65536 else 8)
    # four consecutive offsets share a block; another seed or offset is another table
    assert not np.array_equal(t, X.sample(w, K, 9, 7, False)) and not np.array_equal(t, X.sample(w, K, 10, 6, False))


def test_one_hot_rows_constant_columns_keep_and_inactive_rows():
    H, K = 4, 12
    w = np.zeros((3, H, 9), np.uint32)
    hot = np.array([[3, 0, 8, 5], [1, 1, 2, 7], [6, 4, 4, 0]])
    np.put_along_axis(w, hot[..., None], 123, -1)
    t = X.sample(w, K, 1, 0, const_columns=False)
    assert (t == hot[..., None]).all()
    keep = np.array([[9, 200, 0, 8]] * 3, np.uint8)
    t = X.sample(w, K, 1, 0, const_columns=True, keep=keep)
    assert (t[:, :, :9] == np.arange(9)).all() and (t[:, :, 9] == keep).all() and (t[:, :, 10:] == hot[..., None]).all()
    t9 = X.sample(w, 9, 1, 0, const_columns=True, keep=keep[:, :])      # K <= 9: no kept column
    assert (t9 == np.arange(9)).all()
    t5 = X.sample(w, 5, 1, 0, const_columns=True)
    assert (t5 == np.arange(5)).all()
    out = np.full((3, H, K), 77, np.uint8)
    part = X.sample(w, K, 1, 0, True, keep, active=np.array([1, 0, 1]), out=out)
    assert (part[1] == 77).all() and np.array_equal(part[[0, 2]], t[[0, 2]])


def test_refit_on_hand_made_returns():
    # one state, H = 2, K = 6; returns with a tie at the threshold and -0.0 beside 0.0
    table = np.array([[[0, 1, 2, 3, 4, 200], [8, 8, 7, 7, 6, 6]]], np.uint8)
    ret = np.array([[1.0, -0.0, 5.0, 0.0, -2.0, 0.0]])
    assert X.order(ret).tolist() == [[2, 0, 1, 3, 5, 4]]      # 5 > 1 > (-0.0 == 0.0 == 0.0 in k order) > -2
    w = np.full((1, 2, 9), 1000, np.uint32)
    w[0, 1, 7] = 70000      # read as 65536
    # E = 3: elites 2, 0, 1 (k = 1 wins the tie over k = 3 and 5).  step 0: actions 2, 0, 1; step 1: 7, 8, 8
    new, best = X.refit(w, ret, table, E=3, shift=1, w_min=64)
    third, two_thirds = (1 << 16) // 3, (2 << 16) // 3      # 21845, 43690
    want0 = [500 + (third >> 1)] * 3 + [500] * 6
    want1 = [500] * 7 + [32768 + (third >> 1), 500 + (two_thirds >> 1)]
    assert new.dtype == np.uint32 and new[0, 0].tolist() == want0 and new[0, 1].tolist() == want1
    assert best.tolist() == [[2, 7]]
    # shift 0: the elites' frequencies alone, floored at w_min; E = K: entry 200 counts as 8
    new, _ = X.refit(w, ret, table, E=6, shift=0, w_min=64)
    sixth = (1 << 16) // 6
    assert new[0, 0].tolist() == [sixth] * 5 + [64] * 3 + [sixth]
    assert new[0, 1].tolist() == [64] * 6 + [(2 << 16) // 6] * 3
    new, _ = X.refit(w, ret, table, E=6, shift=0, w_min=0)
    assert new[0, 0, 5] == 0 and new.sum(-1).tolist() == [[6 * sixth, 3 * ((2 << 16) // 6)]]
    # E = 1 and every elite on one action: the weight saturates at 65536; an all-zero row is read as nine ones
    z = np.zeros((1, 2, 9), np.uint32)
    new, best = X.refit(z, ret, table, E=1, shift=0, w_min=0)
    assert new[0, 0].tolist() == [0, 0, 65536, 0, 0, 0, 0, 0, 0]
    new, _ = X.refit(z, ret, table, E=1, shift=16, w_min=0)
    assert new[0, 0].tolist() == [1, 1, 2, 1, 1, 1, 1, 1, 1]      # 1 - (1 >> 16) + (65536 >> 16)
    # all returns equal: the first E in k order; an inactive row is left alone
    new, best = X.refit(w, np.zeros((1, 6)), table, E=2, shift=0, w_min=0)
    assert new[0, 0].tolist() == [32768, 32768] + [0] * 7 and best.tolist() == [[0, 8]]
    same, b = X.refit(w, ret, table, 3, 1, 64, active=np.array([0]), best_seq=np.full((1, 2), 77, np.uint8))
    assert np.array_equal(same, w) and (b == 77).all()


def test_plan_keeps_the_best_sequence():
    """The kept column: with a scorer that likes one particular sequence, no state's best return ever falls from round to round."""
    H, K, M = 5, 16, 4
    target = np.array([2, 2, 7, 7, 1])

    def score(tables):
        ret = (np.minimum(tables, 8) == target[None, :, None]).sum(1).astype(np.float64)
        k = ret.argmax(1)
        return dict(ret=ret, best_k=k.astype(np.int32), best_action=tables[np.arange(M), 0, k].astype(np.int64), best_ret=ret.max(1))

    out = X.plan(X.uniform_weights(M, H), score, K, E=4, iterations=12, seed=5, offset0=40)
    assert (np.diff(out["iter_best_ret"], axis=0) >= 0).all()
    assert (out["iter_best_ret"][-1] >= out["iter_best_ret"][0]).all() and (out["iter_best_ret"][-1] > out["iter_best_ret"][0]).any()
    # what the last refit keeps for the next round's column 9 is the sequence that earned the last best return
    assert np.array_equal((out["best_seq"] == target).sum(1), out["iter_best_ret"][-1])
    assert np.array_equal(out["best_seq"], out["tables"][np.arange(M), :, out["best_k"]])
    assert out["weights"].min() >= 64 and out["weights"].max() <= X.W_MAX


# ---- the input conditions, on the CPU oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track,n", X.CONFIGS)
def test_driven_rows_meet_the_input_conditions(track, n):
    s, ref = X.reference(track, n)
    assert len(s["px"]) == X.DRIVEN_ROWS == 256
    assert ref["iter_best_ret"].shape == (X.ITERATIONS_REF, 256)
    assert (np.diff(ref["iter_best_ret"], axis=0) >= 0).all()      # the best return never falls
    c = X.counts(ref)
    print(track, n, c)
    assert c == X.COUNTS[(track, n)]
    for k in X.COUNT_KEYS:
        assert X.COUNTS[(track, n)][k] >= X.NEED[k], (k, X.COUNTS[(track, n)][k])
    assert X.NEED == dict(improved=50, action_changed=40, drawn_best=20)


# ---- the planner and evaluate.py ------------------------------------------------------------------------------------------------------
def test_cem_planner_constructor_refuses_what_it_cannot_run():
    import ppo_car_amd as pc
    from ppo_car_amd.planner import CEMPlanner, PlannerEvaluator
    for bad in (dict(horizon=0), dict(horizon=257), dict(candidates=9), dict(candidates=4097), dict(elites=0), dict(elites=65),
                dict(candidates=10, elites=11), dict(iterations=0), dict(smoothing_shift=-1), dict(smoothing_shift=17), dict(min_weight=-1),
                dict(min_weight=65537), dict(init_weight=-1), dict(init_weight=65537)):
        with pytest.raises(ValueError, match="CEMPlanner"):
            CEMPlanner(None, **bad)      # (refused before the envs are looked at)
    assert pc.CEMPlanner is CEMPlanner
    with pytest.raises(ValueError, match="kind"):
        PlannerEvaluator("tracks/big_track.json", kind="mppi")


def test_evaluate_cem_options():
    import evaluate
    assert vars(evaluate.parse_args(["--checkpoint", "model.dat"])) == OLD_NAMESPACE
    a = evaluate.parse_args(["--planner", "cem", "--plan-iterations", "4", "--plan-elites", "8", "--envs", "1024"])
    assert a.planner == "cem" and a.plan_iterations == 4 and a.plan_elites == 8 and a.envs == 1024 and a.checkpoint is None
    assert not hasattr(a, "plan_horizon") and not hasattr(a, "plan_candidates")
    a = evaluate.parse_args(["--planner", "cem", "--plan-iterations", "2", "--plan-elites", "16", "--plan-horizon", "12", "--plan-candidates", "128",
                             "--envs", "64"])
    assert (a.plan_iterations, a.plan_elites, a.plan_horizon, a.plan_candidates) == (2, 16, 12, 128)
    a = evaluate.parse_args(["--planner", "shooting", "--envs", "64"])      # as before: nothing of the new options in the namespace
    assert not hasattr(a, "plan_iterations") and not hasattr(a, "plan_elites")
    for argv in (["--checkpoint", "m", "--plan-iterations", "4"], ["--checkpoint", "m", "--plan-elites", "4"],
                 ["--planner", "shooting", "--plan-iterations", "4", "--envs", "8"], ["--planner", "cem", "--plan-iterations", "4", "--envs", "8"],
                 ["--planner", "cem", "--plan-elites", "8", "--envs", "8"], ["--planner", "mppi", "--envs", "8"]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(argv)
    with pytest.raises(ValueError, match="--envs"):
        evaluate.parse_args(["--planner", "cem", "--plan-iterations", "4", "--plan-elites", "8"])
