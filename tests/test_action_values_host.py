"""pc_sequences_action_values (K28) without a GPU: the symbol is declared, bound and exported; every argument check answers before the
device is looked at; and the numpy reference (action_values_reference.py) has the properties the GPU test relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ppo_car_amd as pc
from ppo_car_amd import _capi
from conftest import ROOT
import action_values_reference as V

NAMES = ("pc_sequences_action_values", "pc_bc_minibatch_soft")


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_declared_bound_and_exported(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppocar.h")).read(), flags=re.S)
    assert re.search(rf"\bint\s+{name}\s*\(", hdr)
    assert name in _capi.EXPORTS
    assert hasattr(C.CDLL(pc.lib_path()), name)


def _args(**over):
    """a valid call's arguments on host memory (nothing is dereferenced before the device check), with overrides"""
    M, K = 3, 16
    buf = {k: np.zeros(M * K * 8, np.uint8) for k in ("ret", "actions", "steps", "status", "active", "q", "count", "alive", "target")}
    a = dict(device=-1, ret=buf["ret"].ctypes.data, actions=buf["actions"].ctypes.data, stride=0, steps=buf["steps"].ctypes.data,
             status=buf["status"].ctypes.data, active=buf["active"].ctypes.data, M=M, K=K, accumulate=0, temperature=0.0,
             q=buf["q"].ctypes.data, count=buf["count"].ctypes.data, alive=buf["alive"].ctypes.data, target=buf["target"].ctypes.data,
             stream=None)
    a.update(over)
    return buf, list(a.values())


BAD = [dict(ret=None), dict(actions=None), dict(q=None), dict(count=None), dict(alive=None), dict(steps=None), dict(status=None),
       dict(M=0), dict(M=-4), dict(K=0), dict(K=_capi.PC_SEQ_MAX_CANDIDATES + 1), dict(temperature=-0.5), dict(temperature=float("nan")),
       dict(temperature=float("inf")), dict(temperature=float("-inf"))]


@pytest.mark.parametrize("over", BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_argument_checks_come_before_the_device(over):
    keep, args = _args(**over)
    assert _capi.lib.pc_sequences_action_values(*args) == _capi.PC_ERR_INVALID_ARG


def test_the_order_of_the_checks():
    # NULL pointers before the steps / status pair, that before M, M before K, K before the temperature
    for first, later in ((dict(ret=None), dict(steps=None)), (dict(steps=None), dict(M=0)), (dict(M=0), dict(K=0)),
                         (dict(K=0), dict(temperature=-1.0))):
        keep, args = _args(**first, **later)
        assert _capi.lib.pc_sequences_action_values(*args) == _capi.PC_ERR_INVALID_ARG


def test_no_device():
    for over in (dict(), dict(target=None), dict(active=None), dict(steps=None, status=None), dict(M=2 ** 31)):
        keep, args = _args(**over)      # (M above 2^31 - 1 is refused only after the device)
        assert _capi.lib.pc_sequences_action_values(*args) == _capi.PC_ERR_NO_DEVICE


@pytest.mark.parametrize("cid,M,K,per_state,seed", V.cases(), ids=[c[0] for c in V.cases()])
def test_reference_properties(cid, M, K, per_state, seed):
    c = V.case(M, K, per_state, seed)
    fm = np.minimum(np.broadcast_to(c["first"], (M, K)), 8)
    if K < 9:
        assert any((fm == a).sum() == 0 for a in range(9))
    for status in (True, False):
        st = dict(steps=c["steps"], status=c["status"]) if status else {}
        for T in V.TEMPERATURES:
            r = V.action_values(c["ret"], c["first"], active=c["active"], temperature=T, **st)
            for m in range(M):
                if c["active"][m] == 0:
                    assert (r["target"][m] == 0).all() and (r["count"][m] == 0).all()      # (empty(): untouched)
                    continue
                assert r["q"][m].max() == c["ret"][m].max()
                assert r["count"][m].sum() == K
                t = r["target"][m]
                if r["alive"][m].any():
                    assert abs(float(t.astype(np.float64).sum()) - 1.0) <= 9 * 2.0 ** -24
                    assert ((t != 0) <= (r["alive"][m] != 0)).all()
                    nz = t[t != 0]
                    assert (np.abs(nz) >= np.finfo(np.float32).tiny).all()      # normal float32: an ulp bound means what it says
                    if T > 0:
                        assert ((t != 0) == (r["alive"][m] != 0)).all()
                else:
                    assert (t == 0).all()
            if status:
                assert not r["alive"][0].any()      # row 0: every sequence dead at once
                if M >= 3 and (fm[1] > 2).any():
                    a = int(np.argmax(r["q"][1]))
                    assert r["alive"][1][a] == 0 and r["target"][1][a] == 0      # the row's maximum belongs to a dead action
                    assert np.array_equal(r["alive"][1][3:], np.zeros(6, np.uint8))      # only actions 0 .. 2 can be alive
                    assert np.array_equal(r["alive"][1][:3], (r["count"][1][:3] > 0).astype(np.uint8))


def test_accumulation_equals_the_concatenated_tables():
    M = 5
    parts = [V.case(M, K, True, 40 + i) for i, K in enumerate((9, 65, 17))]
    prev = None
    for i, c in enumerate(parts):
        prev = V.action_values(c["ret"], c["first"], c["steps"], c["status"], accumulate=i > 0, temperature=0.05, prev=prev)
    cat = {k: np.concatenate([c[k] for c in parts], axis=1) for k in ("ret", "first", "steps", "status")}
    whole = V.action_values(cat["ret"], cat["first"], cat["steps"], cat["status"], temperature=0.05)
    for k in whole:
        assert np.array_equal(prev[k].view(np.uint8), whole[k].view(np.uint8)), k
