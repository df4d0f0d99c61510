"""Episode statistics (K3e, pc_episode_stats / pc_gae_episodes): the C-ABI surface and its argument checks, the trainer / CLI
switches, and this file's forward numpy reference (episodes_ref, which the GPU tests compare the kernels with) on hand-built cases.
No GPU needed."""
import math
import os
import re

import numpy as np
import pytest
import torch

from ppo_car_amd import _capi
from conftest import ROOT

INV = _capi.PC_ERR_INVALID_ARG
ALPHABET = np.array([0.0, 0.01, 1.0, 1.01, 11.0, 11.01, -3.0, -2.99, -2.0, -1.99, 8.0, 8.01])   # the reference's reward sums


def init_out(N):
    out = np.zeros((7, N))
    out[5], out[6] = np.inf, -np.inf
    return out


def buffer_dones(term, trunc, last_term, last_trunc):
    """Buffer layout -> done[t] = step t ended an episode (its flags sit in row t + 1; step T - 1's in last_*; row 0 is not read)."""
    d = (term != 0) | (trunc != 0)
    return np.concatenate([d[1:], ((last_term != 0) | (last_trunc != 0))[None]], axis=0)


def episodes_ref(rew, done, scale, carry=None, out=None):
    """Forward numpy reference: rew [T, N] float32, done [T, N] bool -> (out [7, N], carry [4, N]), float64, both accumulated /
    carried exactly as include/ppocar.h describes.  Returns are summed in float64 from the float32 rewards (exact in any order)."""
    T, N = rew.shape
    carry = np.zeros((4, N)) if carry is None else np.array(carry, np.float64)
    out = init_out(N) if out is None else np.array(out, np.float64)
    valid = carry[1] >= 0
    cur = np.where(valid, carry, 0.0)
    for t in range(T):
        r = rew[t].astype(np.float64)
        k = np.rint(r / scale)
        cur[0] = cur[0] + r
        cur[1] += 1
        lap = (k == 11) | (k == 8)
        cur[2] += lap | (k == 1) | (k == -2)
        cur[3] += lap
        fin = done[t] & valid
        out[0] += fin
        out[1] += np.where(fin, cur[0], 0.0)
        out[2] += np.where(fin, cur[1], 0.0)
        out[3] += np.where(fin, cur[2], 0.0)
        out[4] += np.where(fin, cur[3], 0.0)
        out[5] = np.where(fin, np.minimum(out[5], cur[0]), out[5])
        out[6] = np.where(fin, np.maximum(out[6], cur[0]), out[6])
        cur[:, done[t]] = 0.0
        valid = valid | done[t]
    carry_out = np.where(valid, cur, np.array([[0.0], [-1.0], [0.0], [0.0]]))
    return out, carry_out


# ---- the reference on hand-built cases (one env each, scale 1) ------------------------------------------------------------------
def _one(rews, dones, carry=None, scale=1.0):
    r = np.array(rews, np.float32).reshape(-1, 1)
    d = np.array(dones, bool).reshape(-1, 1)
    c = None if carry is None else np.array(carry, np.float64).reshape(4, 1)
    out, c2 = episodes_ref(r, d, scale, c)
    return out[:, 0], c2[:, 0]


def test_reference_no_dones():
    out, c = _one([0.01, 1.01, 0.0], [0, 0, 0])
    assert out[0] == 0 and out[5] == np.inf and out[6] == -np.inf and out[1:5].tolist() == [0, 0, 0, 0]
    assert c.tolist() == [float(np.float32(0.01)) + float(np.float32(1.01)), 3, 1, 0]


def test_reference_done_in_row_0_and_row_last():
    out, c = _one([-3.0, 0.01, 11.01], [1, 0, 1])
    assert out[0] == 2 and out[2] == 3 and out[3] == 1 and out[4] == 1     # episodes of length 1 and 2; the second laps (a gate too)
    assert out[5] == -3.0 and out[6] == float(np.float32(0.01)) + float(np.float32(11.01))
    assert c.tolist() == [0, 0, 0, 0]                                          # the window ended on a boundary: a fresh episode


def test_reference_consecutive_dones():
    out, c = _one([1.0, -2.0, 8.0, 0.01], [1, 1, 1, 0])
    assert out[0] == 3 and out[2] == 3 and out[3] == 3 and out[4] == 1
    assert out[1] == 7.0 and out[5] == -2.0 and out[6] == 8.0
    assert c.tolist() == [float(np.float32(0.01)), 1, 0, 0]


def test_reference_episode_spanning_three_calls():
    r = [1.01, 0.01, 11.01, 0.01, -2.99]
    out1, c1 = _one(r[:2], [0, 0])
    out2, c2 = _one(r[2:4], [0, 0], carry=c1)
    out3, c3 = _one(r[4:], [1], carry=c2)
    assert out1[0] == 0 and out2[0] == 0 and out3[0] == 1
    assert out3[2] == 5 and out3[3] == 2 and out3[4] == 1
    assert out3[1] == sum(float(np.float32(x)) for x in r)
    one, cone = _one(r, [0, 0, 0, 0, 1])
    assert np.array_equal(one, out3) and np.array_equal(cone, c3)


def test_reference_sentinel_start():
    out, c = _one([1.0, 0.01, 11.0, 0.01], [0, 1, 0, 0], carry=[0, -1, 0, 0])
    assert out[0] == 0 and out[2] == 0               # the episode whose start was not observed is dropped
    assert c.tolist() == [11.0 + float(np.float32(0.01)), 2, 1, 1]
    out, c = _one([0.01, 0.01], [0, 0], carry=[0, -1, 0, 0])
    assert c.tolist() == [0, -1, 0, 0]                # no boundary: the carry stays a sentinel


def test_reference_decoding_at_other_scales():
    for s in (0.1, 0.37, 1.0):
        r = (ALPHABET * s).astype(np.float32).reshape(-1, 1)
        k = np.rint(r.astype(np.float64) / s)[:, 0]
        assert np.array_equal(k, [0, 0, 1, 1, 11, 11, -3, -3, -2, -2, 8, 8])
        assert np.abs(r.astype(np.float64)[:, 0] / s - k).max() < 0.02


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_exports_and_library():
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    for name in ("pc_episode_stats", "pc_gae_episodes"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _capi.EXPORTS
        assert getattr(_capi.lib, name) is not None
    assert re.search(r"#define PC_EPISODE_BUFFER 0\b", hdr) and re.search(r"#define PC_EPISODE_STEPS 1\b", hdr)


P = 4096      # a non-NULL address: every call below is refused before any device call, so it is never dereferenced


def _stats(device=0, rew=P, term=P, trunc=P, lt=P, ltr=P, T=8, N=8, layout=0, s=0.1, carry=P, out=P):
    return _capi.lib.pc_episode_stats(device, rew, term, trunc, lt, ltr, T, N, layout, s, carry, out, None)


def _gae(device=0, ptrs=(P,) * 9, T=8, N=8, s=0.1, carry=P, out=P):
    rew, val, term, trunc, lv, lt, ltr, adv, ret = ptrs
    return _capi.lib.pc_gae_episodes(device, rew, val, term, trunc, lv, lt, ltr, 0.99, 0.95, T, N, adv, ret, s, carry, out, None)


@pytest.mark.parametrize("bad", [dict(rew=None), dict(term=None), dict(trunc=None), dict(carry=None), dict(out=None),
                                 dict(lt=None), dict(ltr=None), dict(T=0), dict(T=-3), dict(N=0), dict(layout=2), dict(layout=-1),
                                 dict(s=0.0), dict(s=-0.1), dict(s=math.nan), dict(s=math.inf), dict(s=5e-324)])
def test_episode_stats_argument_checks(bad):
    assert _stats(**bad) == INV


def test_episode_stats_steps_layout_needs_no_last_flags():
    # the STEPS layout ignores last_term / last_trunc: NULL passes the checks and the call then needs a device
    assert _stats(device=-1, lt=None, ltr=None, layout=1) == _capi.PC_ERR_NO_DEVICE


@pytest.mark.parametrize("which", list(range(9)) + ["carry", "out", "T", "N", "s0", "snan", "sinf", "sneg"])
def test_gae_episodes_argument_checks(which):
    kw = {}
    if isinstance(which, int):
        kw["ptrs"] = tuple(None if i == which else P for i in range(9))
    else:
        kw = {"carry": dict(carry=None), "out": dict(out=None), "T": dict(T=0), "N": dict(N=0), "s0": dict(s=0.0),
              "snan": dict(s=math.nan), "sinf": dict(s=math.inf), "sneg": dict(s=-1.0)}[which]
    assert _gae(**kw) == INV


def test_no_device():
    assert _stats(device=-1) == _capi.PC_ERR_NO_DEVICE and _gae(device=-1) == _capi.PC_ERR_NO_DEVICE
    if not torch.cuda.is_available():      # a box without a GPU: every device index
        assert _stats() == _capi.PC_ERR_NO_DEVICE and _gae() == _capi.PC_ERR_NO_DEVICE


# ---- the switches ----------------------------------------------------------------------------------------------------------------
def test_config_and_cli_default_off():
    import train
    from ppo_car_amd.ppo import PPOConfig
    assert PPOConfig().episode_stats is False
    assert train.parse_args(["--run-name", "x"]).episode_stats is False
    assert train.parse_args(["--run-name", "x", "--episode-stats"]).episode_stats is True


def test_episode_scalars_none_without_episodes():
    from ppo_car_amd.episodes import EPISODE_MEAN_KEYS, episode_scalars
    d = episode_scalars([0.0, 0.0, 0.0, 0.0, 0.0, math.inf, -math.inf], 0.1)
    assert d["charts/episodes"] == 0 and all(d[k] is None for k in EPISODE_MEAN_KEYS)
    d = episode_scalars([2.0, 0.3, 1500.0, 40.0, 2.0, 0.1, 0.2], 0.1)
    assert d["charts/episodes"] == 2 and d["charts/episodic_length"] == 750.0 and d["charts/laps_per_episode"] == 1.0
    assert math.isclose(d["charts/episodic_return"], 1.5) and math.isclose(d["charts/episodic_return_max"], 2.0)
