"""Scoring action sequences with a discount and the critic's value, the parts that need no GPU: the C-ABI's symbols, prototypes and
argument checks, the reference's recurrence on hand-made rewards, how often the critic changes the best sequence of the test inputs,
the planners' constructors and evaluate.py's options."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from ppo_car_amd import _capi
from conftest import ROOT
import sequences_reference as Q
import sequences_value_reference as V
from test_sequences_host import OLD_NAMESPACE, POSES_ARGS as K22_POSES

INV = _capi.PC_ERR_INVALID_ARG
P = 4096      # a non-NULL address: every refused call below is refused before any device call, so it is never dereferenced

NEW_IN = ("gamma", "bootstrap", "p", "image", "workspace")
NEW_OUT = ("end_obs", "end_value", "end_discount", "ret_env")
POSES_ARGS = K22_POSES[:16] + NEW_IN + K22_POSES[16:-1] + NEW_OUT + ("stream",)
STATE_ARGS = ("e",) + POSES_ARGS[11:]


def test_symbols_prototypes_and_header_text():
    lib = C.CDLL(_capi.lib_path())
    names = ("pc_env_rollout_sequences_value", "pc_env_rollout_sequences_value_state", "pc_env_rollout_sequences_value_workspace")
    for name in names:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.EXPORTS
    vp = C.c_void_p
    tail = [vp, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, vp, vp, vp] + [vp] * 13      # actions .. stream
    f = _capi.lib.pc_env_rollout_sequences_value
    assert f.restype is C.c_int and list(f.argtypes) == [vp] * 10 + [C.c_int64] + tail and len(f.argtypes) == len(POSES_ARGS)
    g = _capi.lib.pc_env_rollout_sequences_value_state
    assert g.restype is C.c_int and list(g.argtypes) == [vp] + tail and len(g.argtypes) == len(STATE_ARGS)
    w = _capi.lib.pc_env_rollout_sequences_value_workspace
    assert w.restype is C.c_int64 and list(w.argtypes) == [C.c_int64, C.c_int]
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    ins = (r"double reward_scale, double gamma,\s*int bootstrap, const pc_policy\* p, const float\* image,\s*void\* workspace, ")
    outs = (r"double\* ret,\s*int32_t\* steps,\s*uint8_t\* status, int32_t\* gates, int32_t\* laps,\s*int32_t\* best_k,\s*int64_t\* best_action,\s*"
            r"double\* best_ret,\s*float\* end_obs,\s*float\* end_value,\s*double\* end_discount,\s*double\* ret_env,\s*void\* stream\);")
    assert re.search(r"int pc_env_rollout_sequences_value\(const pc_env\* e, const double\* px, [^;]*const uint8_t\* active, int64_t M, "
                     r"const uint8_t\* actions, int64_t actions_state_stride, int K, int H,\s*" + ins + outs, hdr)
    assert re.search(r"int pc_env_rollout_sequences_value_state\(pc_env\* e, const uint8_t\* actions, int64_t actions_state_stride, int K, int H,\s*"
                     + ins + outs, hdr)
    assert re.search(r"int64_t pc_env_rollout_sequences_value_workspace\(int64_t M, int K\);", hdr)
    for name, value in (("NONE", 0), ("RUNNING", 1), ("RUNNING_TRUNCATED", 2)):
        assert re.search(rf"#define PC_SEQ_BOOTSTRAP_{name} {value}\b", hdr) and getattr(_capi, f"PC_SEQ_BOOTSTRAP_{name}") == value
    assert _capi.SEQ_BOOTSTRAP == V.MODES
    # the definitions are part of the header: the recurrence, the end observation, the single policy call, the combination
    text = " ".join(hdr.split())
    for phrase in ("ret = ret + disc * (double)r", "disc = disc * gamma", "ret_env = ret; end_discount = disc", "ONE pc_policy_act_greedy call",
                   "ret_env + end_discount * (double)end_value", "never contracted into an fma", "A terminated lane is never bootstrapped"):
        assert phrase in text, phrase


def test_workspace_query():
    w = _capi.lib.pc_env_rollout_sequences_value_workspace
    assert w(0, 64) == 0 and w(-1, 64) == 0 and w(8, 0) == 0 and w(8, 4097) == 0
    for M, K in ((1, 1), (8, 64), (796, 70), (1 << 20, 4096)):
        assert w(M, K) >= 12 * M * K and w(M, K) % 16 == 0, (M, K)      # int64 actions and float32 log-probabilities


def _policy(D=23):
    h = C.c_void_p()
    assert _capi.lib.pc_policy_create(0, D, 256, 9, -1, -1, C.byref(h)) == 0      # (touches no device)
    return h


def _call(args, fn, kw):
    a = {k: P for k in args}
    a.update(M=8, stride=0, K=64, H=12, scale=0.1, gamma=0.99, bootstrap=0, p=None, image=None, workspace=None, stream=None)
    a.update(kw)
    return fn(*[a[k] for k in args])


def _poses(**kw):
    return _call(POSES_ARGS, _capi.lib.pc_env_rollout_sequences_value, kw)


def _state(**kw):
    return _call(STATE_ARGS, _capi.lib.pc_env_rollout_sequences_value_state, kw)


# K22's refusals, in K22's order, then the new ones: gamma; the mode; p / image; a bootstrap without a policy; a policy without its arrays
SHARED_BAD = [dict(e=None)] + [dict([(k, None)]) for k in ("actions", "ret", "steps", "status")] + [
    dict(K=0), dict(K=4097), dict(H=0), dict(H=1001), dict(stride=1), dict(stride=767), dict(K=70, H=3, stride=768), dict(scale=math.nan),
    dict(scale=math.inf), dict(gamma=math.nan), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=math.inf), dict(gamma=-math.inf),
    dict(gamma=1.0000000000000002), dict(bootstrap=3), dict(bootstrap=-1), dict(bootstrap=1), dict(bootstrap=2),
    dict(p=P), dict(image=P), dict(bootstrap=1, image=P), dict(bootstrap=1, p=P),
    dict(p=P, image=P, workspace=P, end_obs=None), dict(p=P, image=P, workspace=P, end_value=None), dict(p=P, image=P, workspace=None),
    dict(p=P, image=P, workspace=P, bootstrap=2, end_obs=None, end_value=None),
    dict(K=0, gamma=math.nan, bootstrap=9), dict(gamma=math.nan, bootstrap=9, p=P), dict(bootstrap=9, p=P)]


@pytest.mark.parametrize("kw", SHARED_BAD + [dict([(k, None)]) for k in ("px", "py", "vx", "vy", "turns")] + [dict(M=0), dict(M=-5, gamma=2.0)])
def test_argument_errors_before_any_device_call(kw):
    assert _poses(**kw) == INV      # (the handles are made-up addresses: the refusal comes before they are looked at)


@pytest.mark.parametrize("kw", SHARED_BAD)
def test_state_form_argument_errors_before_any_device_call(kw):
    assert _state(**kw) == INV


def test_policy_dimension_is_checked_before_the_device_and_a_valid_call_reaches_it():
    """A handle-sized block of zeros that names a device no machine has: obs dim 0.  Every policy's D differs from it -- refused; without
    a policy, every argument fine, the call gets as far as the device and answers PC_ERR_NO_DEVICE."""
    fake = (C.c_int * 4096)()
    fake[0] = 12345      # pc_env's first member is its device index
    h = C.addressof(fake)
    opt = dict(next_gate=None, time_step=None, track_id=None, active=None, gates=None, laps=None, best_k=None, best_action=None, best_ret=None,
               end_obs=None, end_value=None, end_discount=None, ret_env=None)
    for kw in (dict(), opt, dict(gamma=0.0), dict(gamma=1.0), dict(K=4096, H=1000, stride=4096000), dict(K=1, H=1, M=1)):
        assert _poses(e=h, **kw) == _capi.PC_ERR_NO_DEVICE, kw
        assert _state(e=h, **{k: v for k, v in kw.items() if k in STATE_ARGS}) == _capi.PC_ERR_NO_DEVICE, kw
    for D in (18, 23):
        p = _policy(D)
        for mode in (0, 1, 2):
            assert _poses(e=h, p=p, image=P, workspace=P, bootstrap=mode) == INV
            assert _state(e=h, p=p, image=P, workspace=P, bootstrap=mode) == INV
        _capi.lib.pc_policy_destroy(p)


# ---- the reference's recurrence ------------------------------------------------------------------------------------------------------------
def test_recurrence_on_hand_made_rewards():
    rng = np.random.default_rng(0)
    H, L = 12, 500
    rew = rng.standard_normal((H, L)).astype(np.float32).astype(np.float64)
    steps = rng.integers(1, H + 1, L)
    live = np.arange(H)[:, None] < steps[None, :]
    # gamma 1: the plain sum in step order, the discount stays 1
    ret, disc = V.discount(rew, live, 1.0)
    plain = np.zeros(L)
    for t in range(H):
        plain = np.where(live[t], plain + rew[t], plain)
    assert np.array_equal(ret.view(np.uint64), plain.view(np.uint64)) and (disc == 1.0).all()
    # gamma 0: the first reward alone, the discount 0 after the first step
    ret, disc = V.discount(rew, live, 0.0)
    assert np.array_equal(ret.view(np.uint64), (0.0 + rew[0]).view(np.uint64)) and (disc == 0.0).all()
    # the discount is the chained product, not the closed form: they differ somewhere at gamma 0.99
    ret, disc = V.discount(rew, live, 0.99)
    chain = np.ones(L)
    for t in range(H):
        chain = np.where(live[t], chain * 0.99, chain)
    assert np.array_equal(disc.view(np.uint64), chain.view(np.uint64))
    closed = 0.99 ** steps.astype(np.float64)
    assert (disc != closed).any() and np.allclose(disc, closed, rtol=1e-14, atol=0)
    closed_ret = (rew * live * (0.99 ** np.arange(H, dtype=np.float64))[:, None]).sum(0)
    assert (ret != closed_ret).any() and np.allclose(ret, closed_ret, rtol=1e-12, atol=1e-14)
    # frozen lanes add nothing
    one = V.discount(rew[:, :1], live[:, :1], 0.5)
    short = V.discount(rew[:steps[0], :1], live[:steps[0], :1], 0.5)
    assert one[0][0] == short[0][0] and one[1][0] == short[1][0] == 0.5 ** steps[0]


def test_combine_and_best():
    status = np.array([[V.RUNNING, V.TERMINATED, V.TRUNCATED, V.RUNNING]], np.uint8)
    ret_env = np.array([[1.0, 5.0, 2.0, 1.0]])
    disc = np.array([[0.5, 0.5, 0.25, 0.5]])
    value = np.array([[4.0, 100.0, 20.0, 4.0]], np.float32)
    acts = np.array([[[3, 200 // 100, 7, 1]]])
    assert np.array_equal(V.combine(ret_env, disc, value, status, V.NONE), ret_env)
    assert np.array_equal(V.combine(ret_env, disc, value, status, V.BOOT_RUNNING), [[3.0, 5.0, 2.0, 3.0]])
    assert np.array_equal(V.combine(ret_env, disc, value, status, V.BOOT_RUNNING_TRUNCATED), [[3.0, 5.0, 7.0, 3.0]])
    k, a, r = V.best(V.combine(ret_env, disc, value, status, V.BOOT_RUNNING_TRUNCATED), acts)
    assert (k[0], a[0], r[0]) == (2, 7, 7.0)
    k, a, r = V.best(np.array([[3.0, 1.0, 2.0, 3.0]]), acts)      # a tie: the lowest k
    assert (k[0], a[0], r[0]) == (0, 3, 3.0)


# ---- the inputs: the critic changes the choice often enough --------------------------------------------------------------------------------
@pytest.mark.parametrize("track,n", Q.CONFIGS)
def test_the_critic_changes_the_best_sequence_of_enough_rows(track, n):
    got = {H: V.richness(track, n, H) for H in (4, 12)}
    print(f"{track} {n}: rows of 796 whose best_k differs between bootstrap none and running at gamma {V.RICH_GAMMA}: {got}")
    assert got == V.RICH_COUNTS[(track, n)]
    assert max(got.values()) >= V.RICH_FLOOR
    assert V.FRESH_CRITIC_SCALE == 1.0      # no config needed its test critic scaled up
    # the status mix the modes split on, from sequences_reference's stored counts
    c = Q.COUNTS[(track, n)]
    total = 796 * Q.K_REF
    assert c["running"] >= 0.27 * total and c["truncated"] >= 0.34 * total and c["terminated"] >= 0.36 * total
    _, tr = V.pooled_trace(track, n, 12, Q.K_REF)
    assert (int((tr["status"] == V.RUNNING).sum()), int((tr["status"] == V.TRUNCATED).sum()), int((tr["status"] == V.TERMINATED).sum())) == \
        (c["running"], c["truncated"], c["terminated"])
    assert tr["end_obs"].shape == (796, Q.K_REF, V.obs_dim(n)) and np.isfinite(tr["end_obs"]).all()


def test_trace_at_gamma_one_is_the_plain_reference():
    track, n = "track", 12
    for recipe in ("near_gate",):
        s, ref = Q.reference(track, n, recipe)
        tr = V.trace(track, n, s, Q.table(Q.H_REF, Q.K_REF))
        ret, disc = V.discounted(tr, 1.0)
        assert np.array_equal(ret.view(np.uint64), ref["ret"].view(np.uint64)) and (disc == 1.0).all()
        for k in ("steps", "status", "gates", "laps"):
            assert np.array_equal(tr[k], ref[k]), k
        k, a, r = V.best(ret, tr["actions"])
        assert np.array_equal(k, ref["best_k"]) and np.array_equal(a, ref["best_action"]) and np.array_equal(r, ref["best_ret"])


# ---- the planners and the CLI ---------------------------------------------------------------------------------------------------------------
def test_planners_refuse_a_critic_they_cannot_use():
    from ppo_car_amd.planner import CEMPlanner, Planner, PlannerEvaluator
    import inspect
    for cls in (Planner, CEMPlanner, PlannerEvaluator):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["agent"].default is None and sig["gamma"].default == 1.0 and sig["bootstrap"].default == "none", cls
    for cls in (Planner, CEMPlanner):
        for bad in (dict(bootstrap="running"), dict(bootstrap="running_truncated"), dict(bootstrap="always"), dict(gamma=1.5), dict(gamma=-0.1),
                    dict(gamma=math.nan)):
            with pytest.raises(ValueError):
                cls(None, candidates=16, **bad)      # (refused before the envs are looked at)
    from ppo_car_amd.env import VecCarEnv
    for name in ("rollout_sequences", "score_sequences"):
        sig = inspect.signature(getattr(VecCarEnv, name)).parameters
        assert all(sig[k].default is None for k in ("gamma", "bootstrap", "agent")) and sig["repack"].default is True


def test_evaluate_critic_options():
    import evaluate
    assert vars(evaluate.parse_args(["--checkpoint", "model.dat"])) == OLD_NAMESPACE      # without the new flags: the namespace it was
    a = evaluate.parse_args(["--planner", "shooting", "--envs", "64"])
    assert not hasattr(a, "plan_gamma") and not hasattr(a, "plan_bootstrap")
    cem = ["--planner", "cem", "--plan-iterations", "2", "--plan-elites", "4", "--envs", "64"]
    a = evaluate.parse_args(cem + ["--checkpoint", "model.dat", "--plan-gamma", "0.99", "--plan-bootstrap", "running"])
    assert a.plan_gamma == 0.99 and a.plan_bootstrap == "running" and a.checkpoint == "model.dat"
    a = evaluate.parse_args(cem + ["--plan-gamma", "0.9"])      # a discount alone needs no critic
    assert a.plan_gamma == 0.9 and a.checkpoint is None
    assert evaluate.parse_args(cem + ["--plan-bootstrap", "none"]).plan_bootstrap == "none"
    for argv in (cem + ["--plan-bootstrap", "running"], cem + ["--plan-bootstrap", "running_truncated", "--plan-gamma", "0.99"],
                 cem + ["--plan-bootstrap", "sometimes", "--checkpoint", "m"], ["--checkpoint", "m", "--plan-gamma", "0.9"],
                 ["--checkpoint", "m", "--plan-bootstrap", "running"]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(argv)
