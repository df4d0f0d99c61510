"""Truncation bootstrap (pc_gae_bootstrap, pc_rollout_final_obs, PPOConfig.truncation_bootstrap): the C-ABI surface and its argument
checks, the config / CLI switches, and this file's float64 numpy restatement of the new GAE (gae_bootstrap_ref, which the GPU tests
compare the kernel with).  No GPU needed."""
import os
import re

import numpy as np
import pytest

from ppo_car_amd import _capi
from ppo_car_amd.ppo import PPOConfig
from conftest import ROOT

INV = _capi.PC_ERR_INVALID_ARG
P = 4096      # a non-NULL address: the checks run before any device call, nothing is dereferenced


def gae_ref(rew, val, term, trunc, last_val, last_term, last_trunc, gamma, lam):
    """The reference's GAE (buffer.py:36-64) in float64: step t's flags in row t + 1, step T - 1's in last_*."""
    T, N = rew.shape
    adv = np.zeros((T, N))
    last = np.zeros(N)
    for t in reversed(range(T)):
        nv, tm, tr = (last_val, last_term, last_trunc) if t == T - 1 else (val[t + 1], term[t + 1], trunc[t + 1])
        delta = rew[t] + gamma * nv * (1.0 - tm) - val[t]
        last = delta + gamma * lam * (1.0 - tm) * (1.0 - tr) * last
        adv[t] = last
    return adv, adv + val


def gae_bootstrap_ref(rew, val, term, trunc, last_val, last_term, last_trunc, final_val, gamma, lam, limit=_capi.PC_TIME_LIMIT):
    """include/ppocar.h pc_gae_bootstrap in float64: a truncated step t bootstraps from final_val[t // limit] instead of the next row."""
    T, N = rew.shape
    adv = np.zeros((T, N))
    last = np.zeros(N)
    for t in reversed(range(T)):
        nv, tm, tr = (last_val, last_term, last_trunc) if t == T - 1 else (val[t + 1], term[t + 1], trunc[t + 1])
        nv = np.where(tr != 0, final_val[t // limit], nv)
        delta = rew[t] + gamma * nv * (1.0 - tm) - val[t]
        last = delta + gamma * lam * (1.0 - tm) * (1.0 - tr) * last
        adv[t] = last
    return adv, adv + val


def _case(T, N, seed, limit=_capi.PC_TIME_LIMIT):
    rng = np.random.default_rng(seed)
    rew = rng.normal(size=(T, N))
    val = rng.normal(size=(T, N))
    term = (rng.random((T, N)) < 0.03).astype(np.float64)
    trunc = np.zeros((T, N))
    last_term = (rng.random(N) < 0.03).astype(np.float64)
    last_trunc = np.zeros(N)
    # at most one truncation per (slot, env), never together with a termination (CarEnv's `elif`, car_env.py:746-750)
    K = -(-T // limit)
    for n in range(N):
        for k in range(K):
            t = int(rng.integers(k * limit, min(T, (k + 1) * limit)))
            if t == T - 1:
                last_trunc[n], last_term[n] = 1.0, 0.0
            else:
                trunc[t + 1, n], term[t + 1, n] = 1.0, 0.0
    return rew, val, term, trunc, rng.normal(size=N), last_term, last_trunc, K


@pytest.mark.parametrize("T,limit", [(1, 1000), (7, 3), (12, 5), (25, 10)])
def test_reference_reduces_to_gae_when_final_values_are_the_next_rows(T, limit):
    rew, val, term, trunc, lv, lt, ltr, K = _case(T, 9, T, limit)
    fv = np.zeros((K, 9))
    nxt = np.concatenate([val[1:], lv[None]], axis=0)
    flags = np.concatenate([trunc[1:], ltr[None]], axis=0)
    for t in range(T):
        fv[t // limit] = np.where(flags[t] != 0, nxt[t], fv[t // limit])
    a0, r0 = gae_ref(rew, val, term, trunc, lv, lt, ltr, 0.99, 0.95)
    a1, r1 = gae_bootstrap_ref(rew, val, term, trunc, lv, lt, ltr, fv, 0.99, 0.95, limit)
    assert np.array_equal(a0, a1) and np.array_equal(r0, r1)


def test_reference_changes_only_segments_that_end_in_a_truncation():
    T, N, limit = 30, 16, 10
    rew, val, term, trunc, lv, lt, ltr, K = _case(T, N, 5, limit)
    fv = np.random.default_rng(1).normal(size=(K, N)) + 100.0
    a0, _ = gae_ref(rew, val, term, trunc, lv, lt, ltr, 0.99, 0.95)
    a1, _ = gae_bootstrap_ref(rew, val, term, trunc, lv, lt, ltr, fv, 0.99, 0.95, limit)
    done = np.concatenate([(term[1:] != 0) | (trunc[1:] != 0), ((lt != 0) | (ltr != 0))[None]], axis=0)
    tr_end = np.concatenate([trunc[1:] != 0, (ltr != 0)[None]], axis=0)
    for n in range(N):
        ends_trunc = False      # the segment of step t ends at the first done at or after t
        for t in reversed(range(T)):
            if done[t, n]:
                ends_trunc = bool(tr_end[t, n])
            if not ends_trunc or not done[t:, n].any():
                assert a0[t, n] == a1[t, n], (t, n)
    assert not np.array_equal(a0, a1)
    # a truncated step t: delta uses gamma * V(final) -- the trace is still cut there
    t, n = np.argwhere(tr_end[:-1])[0]
    assert np.isclose(a1[t, n], rew[t, n] + 0.99 * fv[t // limit, n] * (1.0 - term[t + 1, n]) - val[t, n])


def test_symbols_in_header_exports_and_library():
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    assert re.search(r"#define PC_TIME_LIMIT 1000\b", hdr) and _capi.PC_TIME_LIMIT == 1000
    for name in ("pc_gae_bootstrap", "pc_rollout_final_obs"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _capi.EXPORTS
        assert getattr(_capi.lib, name) is not None


def _boot(device=0, T=4, N=8, slots=1, ptrs=(P,) * 10, carry=None, out=None, s=0.1):
    rew, val, term, trunc, lv, lt, ltr, fv, adv, ret = ptrs
    return _capi.lib.pc_gae_bootstrap(device, rew, val, term, trunc, lv, lt, ltr, fv, slots, 0.99, 0.95, T, N, adv, ret, s, carry, out,
                                      None)


@pytest.mark.parametrize("which", list(range(10)))
def test_gae_bootstrap_null_arguments(which):
    assert _boot(ptrs=tuple(None if i == which else P for i in range(10))) == INV


@pytest.mark.parametrize("T,slots", [(1, 0), (1000, 0), (1001, 1), (2500, 2), (4, -1)])
def test_gae_bootstrap_slots_too_small(T, slots):
    assert _boot(T=T, slots=slots) == INV


@pytest.mark.parametrize("kw", [dict(T=0), dict(T=-3), dict(N=0), dict(carry=P), dict(out=P), dict(carry=P, out=P, s=0.0),
                                dict(carry=P, out=P, s=float("nan"))])
def test_gae_bootstrap_other_argument_checks(kw):
    assert _boot(**kw) == INV


def test_gae_bootstrap_valid_arguments_reach_the_device_check():
    # every argument fine: the call gets as far as the device (an impossible device id: PC_ERR_NO_DEVICE, not INVALID_ARG)
    assert _boot(device=-1, T=2500, slots=3) == _capi.PC_ERR_NO_DEVICE
    assert _boot(device=-1, carry=P, out=P) == _capi.PC_ERR_NO_DEVICE


def _roll(T=8, slots=1, final_obs=P):
    return _capi.lib.pc_rollout_final_obs(None, None, P, T, 0.1, 0, 0, None, *([P] * 12), final_obs, slots, None)


@pytest.mark.parametrize("kw", [dict(final_obs=None), dict(slots=0), dict(T=1001, slots=1), dict(T=0), dict(T=-1)])
def test_rollout_final_obs_argument_checks(kw):
    assert _roll(**kw) == INV


def test_config_validation():
    assert PPOConfig().truncation_bootstrap == "reference"
    assert PPOConfig(truncation_bootstrap="final_obs").truncation_bootstrap == "final_obs"
    for bad in ("final", "", None, "FINAL_OBS"):
        with pytest.raises(ValueError, match="truncation_bootstrap"):
            PPOConfig(truncation_bootstrap=bad)


def test_cli_flag():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_cli", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["--run-name", "x"]).truncation_bootstrap == "reference"
    assert mod.parse_args(["--run-name", "x", "--truncation-bootstrap", "final_obs"]).truncation_bootstrap == "final_obs"
    with pytest.raises(SystemExit):
        mod.parse_args(["--run-name", "x", "--truncation-bootstrap", "nope"])
