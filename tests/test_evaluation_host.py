"""Batched evaluation (pc_first_episodes, pc_greedy, ppo_car_amd.Evaluator): the numpy reference of the first-episode state
(first_episode_reference.py, which the GPU tests hold the kernel to) on hand-built cases, the C-ABI surface and its argument checks,
the trainer / CLI switches and the scalars.  No GPU needed."""
import math
import os
import re

import numpy as np
import pytest
import torch

from ppo_car_amd import _capi
from conftest import ROOT
from first_episode_reference import RUNNING, TERMINATED, TRUNCATED, buffer_flags, first_episodes_ref, new_state

INV, UNS, NODEV = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_UNSUPPORTED, _capi.PC_ERR_NO_DEVICE
INF = math.inf


def f32(x):
    return float(np.float32(x))


def _one(rews, terms, truncs=None, scale=1.0, state=None):
    r = (np.array(rews, np.float64) * scale).astype(np.float32).reshape(-1, 1)
    te = np.array(terms, np.float32).reshape(-1, 1)
    tr = np.zeros_like(te) if truncs is None else np.array(truncs, np.float32).reshape(-1, 1)
    st = None if state is None else np.array(state, np.float64).reshape(8, 1)
    return first_episodes_ref(r, te, tr, scale, st)[:, 0]


# ---- the reference on hand-built one-env cases ----------------------------------------------------------------------------------
def test_new_state():
    s = new_state(3)
    assert s.shape == (8, 3) and s.dtype == np.float64 and not s[:6].any() and np.all(s[6:] == INF)


def test_reference_no_done():
    s = _one([0.01, 1.01, 0.0], [0, 0, 0])
    assert s.tolist() == [f32(0.01) + f32(1.01), 3, 1, 0, RUNNING, 0, INF, INF]


def test_reference_done_in_row_0():
    s = _one([-3.0, 1.0, 11.0], [1, 0, 0])
    assert s.tolist() == [-3.0, 1, 0, 0, TERMINATED, 0, INF, INF]
    s = _one([0.01, 1.0], [0, 0], truncs=[1, 0])
    assert s.tolist() == [f32(0.01), 1, 0, 0, TRUNCATED, 0, INF, INF]


def test_reference_done_in_the_last_row_of_the_buffer_layout():
    """Buffer layout: step t's flags in row t + 1, step T - 1's in last_*; row 0's flags belong to the step before the window."""
    rew = np.array([[0.01], [1.0], [0.01]], np.float32)
    term = np.array([[1.0], [0.0], [0.0]], np.float32)          # row 0: not this window's
    trunc = np.zeros_like(term)
    te, tr = buffer_flags(term, trunc, np.array([0.0], np.float32), np.array([1.0], np.float32))
    assert te[:, 0].tolist() == [0, 0, 0] and tr[:, 0].tolist() == [0, 0, 1]
    s = first_episodes_ref(rew, te, tr, 1.0)[:, 0]
    assert s.tolist() == [f32(0.01) + 1.0 + f32(0.01), 3, 1, 0, TRUNCATED, 0, INF, INF]


def test_reference_both_flags_count_as_terminated():
    assert _one([0.01, -3.0], [0, 1], truncs=[0, 1])[4] == TERMINATED


def test_reference_rows_after_the_done_are_ignored():
    s = _one([1.0, -3.0, 11.0, 1.0, -3.0], [0, 1, 0, 0, 1])
    assert s.tolist() == [-2.0, 2, 1, 0, TERMINATED, 0, INF, INF]


def test_reference_two_laps_with_different_lap_times():
    #           t: 1     2     3     4      5     6     7      8
    s = _one([0.01, 1.0, 0.01, 11.0, 0.01, 1.01, 11.01, 0.01], [0] * 8)
    assert s[1] == 8 and s[2] == 4 and s[3] == 2 and s[4] == RUNNING
    assert s[5] == 7 and s[7] == 4 and s[6] == 3          # laps of 4 and 3 steps: best != first, their sum = the last close


def test_reference_lap_on_the_closing_step():
    s = _one([1.0, 0.01, 8.0, 1.0], [0, 0, 1, 0])         # k = 8: lap + crash in one step
    assert s.tolist() == [1.0 + f32(0.01) + 8.0, 3, 2, 1, TERMINATED, 3, 3, 3]


def test_reference_episode_spanning_three_windows():
    r = [1.01, 0.01, 11.01, 0.01, 11.0, -2.99, 1.0]
    te = [0, 0, 0, 0, 0, 1, 0]
    s1 = _one(r[:2], te[:2])
    s2 = _one(r[2:4], te[2:4], state=s1)
    s3 = _one(r[4:], te[4:], state=s2)
    one = _one(r, te)
    assert np.array_equal(s3.view(np.int64), one.view(np.int64))
    assert one[1] == 6 and one[3] == 2 and one[5] == 5 and one[7] == 3 and one[6] == 2 and one[4] == TERMINATED
    assert one[0] == sum(f32(x) for x in r[:6])
    assert np.array_equal(_one(r, te, state=one), one)     # a closed env is left alone


@pytest.mark.parametrize("scale", [1.0, 0.1, 0.37])
def test_reference_scales(scale):
    r = [0.01, 1.0, 1.01, 11.0, -2.0, 11.01, -1.99, -3.0]
    s = _one(r, [0] * 7 + [1], scale=scale)
    assert s[1] == 8 and s[2] == 6 and s[3] == 2 and s[4] == TERMINATED and s[5] == 6 and s[7] == 4 and s[6] == 2
    assert s[0] == sum(float(np.float32(x * scale)) for x in r)


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_exports_and_library():
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    for name in ("pc_first_episodes", "pc_greedy"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _capi.EXPORTS
        assert getattr(_capi.lib, name) is not None
    for name, value in (("PC_FIRST_ROWS", 8), ("PC_FIRST_RUNNING", 0), ("PC_FIRST_TERMINATED", 1), ("PC_FIRST_TRUNCATED", 2)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
        assert getattr(_capi, name) == value


P = 4096      # a non-NULL address: every call below is refused before any device call, so it is never dereferenced


def _first(device=0, rew=P, term=P, trunc=P, lt=P, ltr=P, T=8, N=8, layout=0, s=0.1, state=P):
    return _capi.lib.pc_first_episodes(device, rew, term, trunc, lt, ltr, T, N, layout, s, state, None)


def _greedy(device=0, logits=P, N=8, A=9, actions=P, af=P, lp=P):
    return _capi.lib.pc_greedy(device, logits, N, A, actions, af, lp, None)


@pytest.mark.parametrize("bad", [dict(rew=None), dict(term=None), dict(trunc=None), dict(state=None), dict(lt=None), dict(ltr=None),
                                 dict(T=0), dict(T=-3), dict(N=0), dict(N=-1), dict(layout=2), dict(layout=-1),
                                 dict(s=0.0), dict(s=-0.1), dict(s=math.nan), dict(s=math.inf), dict(s=5e-324)])
def test_first_episodes_argument_checks(bad):
    assert _first(**bad) == INV
    assert _first(device=-1, **bad) == INV          # the arguments are looked at before the device


def test_first_episodes_steps_layout_needs_no_last_flags():
    assert _first(device=-1, lt=None, ltr=None, layout=1) == NODEV


@pytest.mark.parametrize("bad,code", [(dict(logits=None), INV), (dict(actions=None), INV), (dict(N=0), INV), (dict(N=-5), INV),
                                      (dict(A=0), UNS), (dict(A=-1), UNS), (dict(A=17), UNS)])
def test_greedy_argument_checks(bad, code):
    assert _greedy(**bad) == code
    assert _greedy(device=-1, **bad) == code


def test_no_device():
    assert _first(device=-1) == NODEV and _greedy(device=-1) == NODEV
    assert _greedy(device=-1, af=None, lp=None) == NODEV and _greedy(device=-1, A=1) == NODEV and _greedy(device=-1, A=16) == NODEV
    if not torch.cuda.is_available():      # a box without a GPU: every device index
        assert _first() == NODEV and _greedy() == NODEV


# ---- the switches ----------------------------------------------------------------------------------------------------------------
def test_config_and_cli_default_off():
    import train
    from ppo_car_amd.ppo import PPOConfig
    cfg = PPOConfig()
    assert cfg.eval_every == 0 and cfg.eval_envs == 1024 and cfg.eval_greedy is False and cfg.eval_track is None
    a = train.parse_args(["--run-name", "x"])
    assert a.eval_every == 0 and a.eval_envs == 1024 and a.eval_greedy is False and a.eval_track is None
    a = train.parse_args(["--run-name", "x", "--eval-every", "5", "--eval-envs", "64", "--eval-greedy", "--eval-track", "t.json"])
    assert a.eval_every == 5 and a.eval_envs == 64 and a.eval_greedy is True and a.eval_track == "t.json"


def test_config_value_errors():
    from ppo_car_amd.ppo import PPOConfig
    with pytest.raises(ValueError):
        PPOConfig(eval_every=-1)
    with pytest.raises(ValueError):
        PPOConfig(eval_every=1, eval_envs=0)
    with pytest.raises(ValueError):
        PPOConfig(eval_envs=-4)
    PPOConfig(eval_every=3, eval_envs=1)


# ---- the scalars -----------------------------------------------------------------------------------------------------------------
def test_scalars():
    from ppo_car_amd.evaluation import EVAL_KEYS, EVAL_MEAN_KEYS, EVAL_TOTALS, evaluation_scalars
    from ppo_car_amd.model import PolicyRangeError
    #      N  ret   min  max   len   gates laps term lapsum best lapped firstsum range
    tot = [4, 8.0, 1.0, 3.0, 2000.0, 120.0, 6.0, 1.0, 1800.0, 250.0, 3.0, 960.0, 0.0]
    assert len(tot) == EVAL_TOTALS
    d = evaluation_scalars(tot, 0.1)
    assert set(d) == set(EVAL_KEYS)
    assert d["eval/episodes"] == 4 and d["eval/episodic_length"] == 500.0 and d["eval/gates_per_episode"] == 30.0
    assert d["eval/laps_per_episode"] == 1.5 and d["eval/crash_rate"] == 0.25
    assert math.isclose(d["eval/episodic_return"], 20.0) and math.isclose(d["eval/episodic_return_min"], 10.0)
    assert math.isclose(d["eval/episodic_return_max"], 30.0)
    assert d["eval/best_lap_steps"] == 250.0 and d["eval/mean_lap_steps"] == 300.0 and d["eval/first_lap_steps"] == 320.0
    # no env lapped: the lap keys are None, the rest stands
    none = [4, 8.0, 1.0, 3.0, 2000.0, 12.0, 0.0, 4.0, 0.0, INF, 0.0, 0.0, 0.0]
    d = evaluation_scalars(none, 0.1)
    assert d["eval/best_lap_steps"] is None and d["eval/mean_lap_steps"] is None and d["eval/first_lap_steps"] is None
    assert d["eval/crash_rate"] == 1.0 and d["eval/laps_per_episode"] == 0.0 and d["eval/episodic_length"] == 500.0
    # a non-zero range status: the episodes were not the policy's
    bad = tot[:12] + [4.0]
    d = evaluation_scalars(bad, 0.1)
    assert d["eval/episodes"] == 4 and all(d[k] is None for k in EVAL_MEAN_KEYS)
    with pytest.raises(PolicyRangeError):
        evaluation_scalars(bad, 0.1, policy_range="raise")
