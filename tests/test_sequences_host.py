"""Scoring action sequences, the parts that need no GPU: the C-ABI's symbols and argument checks, the plain reference
(sequences_reference.py) against step_poses_reference.step and its stored input counts, the Planner's constructor and candidate
table, and evaluate.py's --planner options."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from ppo_car_amd import _capi
from conftest import ROOT
import step_poses_reference as R
import sequences_reference as Q

INV = _capi.PC_ERR_INVALID_ARG
P = 4096      # a non-NULL address: every refused call below is refused before any device call, so it is never dereferenced

POSES_ARGS = ("e", "px", "py", "vx", "vy", "turns", "next_gate", "time_step", "track_id", "active", "M", "actions", "stride", "K", "H", "scale",
              "ret", "steps", "status", "gates", "laps", "best_k", "best_action", "best_ret", "stream")
STATE_ARGS = ("e",) + POSES_ARGS[11:]


def test_symbols_exported_with_signatures():
    lib = C.CDLL(_capi.lib_path())
    for name in ("pc_env_rollout_sequences", "pc_env_rollout_sequences_state"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.EXPORTS
    vp = C.c_void_p
    tail = [vp, C.c_int64, C.c_int, C.c_int, C.c_double] + [vp] * 9      # actions .. stream
    f = _capi.lib.pc_env_rollout_sequences
    assert f.restype is C.c_int and list(f.argtypes) == [vp] * 10 + [C.c_int64] + tail and len(f.argtypes) == len(POSES_ARGS)
    g = _capi.lib.pc_env_rollout_sequences_state
    assert g.restype is C.c_int and list(g.argtypes) == [vp] + tail and len(g.argtypes) == len(STATE_ARGS)
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    outs = (r"double\* ret,\s*int32_t\* steps, uint8_t\* status, int32_t\* gates, int32_t\* laps,\s*int32_t\* best_k,\s*int64_t\* best_action,\s*"
            r"double\* best_ret, void\* stream\);")
    assert re.search(r"int pc_env_rollout_sequences\(const pc_env\* e, const double\* px, const double\* py, const double\* vx, const double\* vy,\s*"
                     r"const int32_t\* turns, const int32_t\* next_gate, const int32_t\* time_step, const uint8_t\* track_id,\s*"
                     r"const uint8_t\* active, int64_t M, const uint8_t\* actions, int64_t actions_state_stride, int K, int H,\s*"
                     r"double reward_scale, " + outs, hdr)
    assert re.search(r"int pc_env_rollout_sequences_state\(pc_env\* e, const uint8_t\* actions, int64_t actions_state_stride, int K, int H, "
                     r"double reward_scale,\s*" + outs, hdr)
    assert re.search(r"#define PC_SEQ_MAX_CANDIDATES 4096\b", hdr) and _capi.PC_SEQ_MAX_CANDIDATES == 4096


def _poses(**kw):
    a = {k: P for k in POSES_ARGS}
    a.update(M=8, stride=0, K=64, H=12, scale=0.1, stream=None)
    a.update(kw)
    return _capi.lib.pc_env_rollout_sequences(*[a[k] for k in POSES_ARGS])


def _state(**kw):
    a = {k: P for k in STATE_ARGS}
    a.update(stride=0, K=64, H=12, scale=0.1, stream=None)
    a.update(kw)
    return _capi.lib.pc_env_rollout_sequences_state(*[a[k] for k in STATE_ARGS])


# the documented order: NULL handle; NULL required arrays; M; K; H; the stride; reward_scale.  Every later argument is fine in each case
# and, in the combined ones, wrong as well: the refusal is the same code either way, and no made-up address is ever read.
SHARED_BAD = [dict(e=None)] + [dict([(k, None)]) for k in ("actions", "ret", "steps", "status")] + [
    dict(K=0), dict(K=-1), dict(K=4097), dict(K=1 << 30), dict(H=0), dict(H=-2), dict(H=1001), dict(stride=1), dict(stride=-768),
    dict(stride=767), dict(stride=769), dict(stride=12), dict(stride=64), dict(K=70, H=3, stride=768), dict(scale=math.nan), dict(scale=math.inf),
    dict(scale=-math.inf), dict(e=None, actions=None, K=0, H=0, stride=5, scale=math.nan), dict(K=0, H=0, stride=5, scale=math.nan),
    dict(H=0, stride=5, scale=math.nan), dict(stride=5, scale=math.nan),
    dict(K=0, gates=None, laps=None, best_k=None, best_action=None, best_ret=None)]


@pytest.mark.parametrize("kw", SHARED_BAD + [dict([(k, None)]) for k in ("px", "py", "vx", "vy", "turns")]
                         + [dict(M=0), dict(M=-5), dict(px=None, M=0, K=0), dict(M=0, K=0, H=0, stride=3, scale=math.nan),
                            dict(M=0, next_gate=None, time_step=None, track_id=None, active=None)])
def test_argument_errors_before_any_device_call(kw):
    # (the handle is a made-up address too: the refusal comes before the handle is looked at)
    assert _poses(**kw) == INV


@pytest.mark.parametrize("kw", SHARED_BAD)
def test_state_form_argument_errors_before_any_device_call(kw):
    assert _state(**kw) == INV


def test_a_valid_call_reaches_the_device_check():
    """Every argument fine, the optional ones NULL or not, both strides, the limits of K and H: the call gets as far as the handle's
    device -- here a handle-sized block of zeros that names a device no machine has -- and answers PC_ERR_NO_DEVICE, not INVALID_ARG."""
    fake = (C.c_int * 4096)()
    fake[0] = 12345      # pc_env's first member is its device index
    h = C.addressof(fake)
    opt = dict(next_gate=None, time_step=None, track_id=None, active=None, gates=None, laps=None, best_k=None, best_action=None, best_ret=None)
    for kw in (dict(), opt, dict(stride=768), dict(K=4096, H=1000), dict(K=1, H=1, M=1), dict(K=4096, H=1000, stride=4096000), dict(scale=0.0),
               dict(scale=-2.5)):
        assert _poses(e=h, **kw) == _capi.PC_ERR_NO_DEVICE, kw
        kw = {k: v for k, v in kw.items() if k in STATE_ARGS}
        assert _state(e=h, **kw) == _capi.PC_ERR_NO_DEVICE, kw


# ---- the reference and its inputs ----------------------------------------------------------------------------------------------------
def test_table_layout():
    t = Q.table(12, 64)
    assert t.dtype == np.uint8 and t.shape == (12, 64) and t.max() == 8
    assert (t[:, :9] == np.arange(9)).all() and len({tuple(c) for c in t.T}) > 60
    assert np.array_equal(Q.table(12, 70)[:, :9], t[:, :9]) and np.array_equal(Q.table(12, 1), np.zeros((12, 1), np.uint8))


@pytest.mark.parametrize("track,n", Q.CONFIGS)
def test_reference_at_one_step_is_step_poses_reference(track, n):
    """H = 1, the nine constant columns: every row under every action is one step_poses_reference.step"""
    for recipe in Q.RECIPES:
        s = Q.states(track, n, recipe)
        M = len(s["px"])
        got = Q.rollout(track, n, s, Q.table(1, 9))
        rows, acts = R.all_actions({k: s[k] for k in Q.STATE_KEYS})      # action a in rows a * M ..
        ref = R.step(track, n, rows, acts)
        fold = lambda a: np.asarray(a).reshape(9, M).T
        assert np.array_equal(got["ret"].view(np.uint64), fold(ref["reward"].astype(np.float64)).view(np.uint64)), recipe
        assert (got["steps"] == 1).all()
        want = np.where(fold(ref["terminated"]), Q.TERMINATED, np.where(fold(ref["truncated"]), Q.TRUNCATED, Q.RUNNING))
        assert np.array_equal(got["status"], want), recipe
        assert np.array_equal(got["gates"], fold(ref["gate"]).astype(np.int32)), recipe
        assert np.array_equal(got["laps"], fold(ref["gate"] & (ref["next_gate"] == 0)).astype(np.int32)), recipe
        for k in Q.STATE_KEYS:
            assert np.array_equal(got["state"][k].reshape(M, 9), fold(ref[k])), (recipe, k)
        assert np.array_equal(got["best_k"], got["ret"].argmax(1)) and np.array_equal(got["best_action"], got["best_k"])


@pytest.mark.parametrize("track,n", Q.CONFIGS)
def test_reference_reproduces_the_stored_counts(track, n):
    c, pairs, lap_pairs = Q.counts(track, n)
    assert pairs == 796 * Q.K_REF and lap_pairs == 540 * Q.K_REF
    assert c == Q.COUNTS[(track, n)]
    Q.meets(c, pairs, lap_pairs)      # the input conditions, from the oracle alone
    for recipe in Q.RECIPES:
        s, ref = Q.reference(track, n, recipe)
        assert ref["steps"].min() >= 1 and ref["steps"].max() == Q.H_REF
        assert ((ref["status"] == Q.RUNNING) == (ref["steps"] == Q.H_REF))[ref["status"] == Q.RUNNING].all()
        assert (ref["laps"] <= ref["gates"]).all() and (ref["gates"] <= ref["steps"]).all()
        # a frozen copy: a step count below H means the episode ended there
        assert (ref["status"][ref["steps"] < Q.H_REF] != Q.RUNNING).all()
        # ties: the best index is the lowest of the row's maxima
        is_max = ref["ret"] == ref["ret"].max(1, keepdims=True)
        assert np.array_equal(ref["best_k"], is_max.argmax(1))
        assert np.array_equal(ref["best_ret"].view(np.uint64), ref["ret"].max(1).view(np.uint64))
    # nearly every row without a unique maximum has a tie: that is what exercises the lowest-k rule
    assert 796 - c["unique_max_rows"] > 600


def test_per_state_tables_in_the_reference():
    track, n = "big_track", 16
    s = {k: v[:6] for k, v in Q.states(track, n, "near_gate").items()}
    tabs = np.stack([Q.table(5, 12, seed=20 + m) for m in range(6)])
    both = Q.rollout(track, n, s, tabs)
    for m in range(6):
        one = Q.rollout(track, n, {k: v[m:m + 1] for k, v in s.items()}, tabs[m])
        for k in Q.OUT_KEYS + Q.BEST_KEYS:
            assert np.array_equal(both[k][m:m + 1], one[k]), (m, k)


# ---- the planner -----------------------------------------------------------------------------------------------------------------------
def test_planner_constructor_refuses_what_it_cannot_run():
    from ppo_car_amd.planner import Planner
    for bad in (dict(candidates=8), dict(candidates=0), dict(candidates=4097), dict(horizon=0), dict(horizon=1001), dict(horizon=-3)):
        with pytest.raises(ValueError):
            Planner(None, **bad)      # (refused before the envs are looked at)
    import ppo_car_amd as pc
    assert pc.Planner is Planner and hasattr(pc, "PlannerEvaluator")


PLAN_H, PLAN_K, PLAN_SEED, PLAN_ROUNDS = 12, 64, 3, 20      # what the GPU test plans with


def test_candidate_table_regenerated_on_the_host():
    seen = set()
    for step in range(PLAN_ROUNDS):
        t, margin = Q.planner_draw(PLAN_H, PLAN_K, PLAN_SEED, step)
        assert t.dtype == np.uint8 and t.shape == (PLAN_H, PLAN_K) and t.max() <= 8
        assert (t[:, :9] == np.arange(9)).all()
        assert len(np.unique(t[:, 9:])) == 9      # every action is drawn
        # no drawn element sits where a float32 CDF of nine equal bins (boundaries good to ~1e-7) could decide otherwise
        assert margin > 1e-6, (step, margin)
        seen.add(t.tobytes())
    assert len(seen) == PLAN_ROUNDS      # every step its own table
    again, _ = Q.planner_draw(PLAN_H, PLAN_K, PLAN_SEED, 7)
    assert np.array_equal(again, Q.planner_draw(PLAN_H, PLAN_K, PLAN_SEED, 7)[0])
    assert not np.array_equal(again, Q.planner_draw(PLAN_H, PLAN_K, PLAN_SEED + 1, 7)[0])
    # the element index is t * K + k: the table is a plain reshape of the call's draws
    import draw_reference as D
    u = D.uniform(PLAN_SEED, 7, np.arange(PLAN_H * PLAN_K))
    a = D.draw_f64(np.zeros((PLAN_H * PLAN_K, 9)), u)[0]
    assert again[5, 40] == a[5 * PLAN_K + 40] and np.array_equal(again[:, 9:], a.reshape(PLAN_H, PLAN_K)[:, 9:])
    assert Q.planner_draw(4, 9, 0, 0)[0].shape == (4, 9)      # nothing drawn: the constant sequences alone


# ---- evaluate.py ---------------------------------------------------------------------------------------------------------------------
OLD_NAMESPACE = dict(checkpoint="model.dat", track="tracks/big_track.json", num_rays=12, episodes=5, greedy=False, seed=0, frames=None,
                     frame_every=5, envs=None, rollout_kernel="auto", shield=0, maps=None, landscape=None, landscape_cell=8, landscape_speed=0.5,
                     landscape_horizon=0, landscape_lookahead=False, video=None, video_envs=4, video_scale=4, video_fps=30)


def test_evaluate_planner_options():
    import evaluate
    # without --planner: the namespace evaluate.py always had, attribute for attribute, and the checkpoint still required
    assert vars(evaluate.parse_args(["--checkpoint", "model.dat"])) == OLD_NAMESPACE
    assert vars(evaluate.parse_args(["--checkpoint", "model.dat", "--envs", "32", "--greedy"])) == dict(OLD_NAMESPACE, envs=32, greedy=True)
    for argv in ([], ["--envs", "8"], ["--checkpoint", "m", "--plan-horizon", "4"], ["--planner", "cem", "--envs", "8"]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(argv)
    a = evaluate.parse_args(["--planner", "shooting", "--plan-horizon", "16", "--plan-candidates", "256", "--envs", "1024"])
    assert a.planner == "shooting" and a.plan_horizon == 16 and a.plan_candidates == 256 and a.envs == 1024 and a.checkpoint is None
    a = evaluate.parse_args(["--planner", "shooting", "--envs", "64", "--track", "tracks/track.json"])
    assert a.planner == "shooting" and not hasattr(a, "plan_horizon") and a.track == "tracks/track.json"
    with pytest.raises(ValueError, match="--envs"):
        evaluate.parse_args(["--planner", "shooting"])
