"""pc_sequences_action_values (K28) on the GPU against its numpy restatement (action_values_reference.py) on synthetic tables, and end
to end on pc_env_rollout_sequences' outputs.  q on bits, count and alive exact, target at temperature 0 on bits; at a positive temperature
within one float32 ulp: both sides round a float64 quotient that is good to about 1e-15 relative, so they can differ only where it
lies on a float32 rounding boundary (the reference's non-zero entries are normal float32: test_action_values_host.py)."""
import numpy as np
import pytest
import torch

import ppo_car_amd as pc
from ppo_car_amd import _capi
from conftest import TRACKS
import action_values_reference as V
import sequences_reference as Q
import step_poses_reference as R

pytestmark = pytest.mark.gpu

OUT = (("q", torch.float64), ("count", torch.int32), ("alive", torch.uint8), ("target", torch.float32))
CASES = V.cases()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _sentinel(M):
    return {k: torch.full((M, 9), V.SENTINEL, dtype=dt, device="cuda") for k, dt in OUT}


def _call(c, temperature, out, accumulate=0, status=True, active=True, target=True):
    """one launch on device copies of the case's arrays into `out` (device tensors): dict of numpy arrays"""
    M, K = c["ret"].shape
    ret, first = _dev(c["ret"], torch.float64), _dev(c["first"], torch.uint8)
    steps, st = _dev(c["steps"], torch.int32), _dev(c["status"], torch.uint8)
    act = _dev(c["active"], torch.uint8)
    stride = K if c["first"].ndim == 2 else 0
    _capi.check(_capi.lib.pc_sequences_action_values(
        0, ret.data_ptr(), first.data_ptr(), stride, steps.data_ptr() if status else None, st.data_ptr() if status else None,
        act.data_ptr() if active else None, M, K, accumulate, float(temperature), out["q"].data_ptr(), out["count"].data_ptr(),
        out["alive"].data_ptr(), out["target"].data_ptr() if target else None, torch.cuda.current_stream().cuda_stream),
        "pc_sequences_action_values")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _sentinel_ref(M):
    return {k: np.full((M, 9), V.SENTINEL, dtype=dt) for k, dt in (("q", np.float64), ("count", np.int32), ("alive", np.uint8), ("target", np.float32))}


def _compare(got, want, temperature, what):
    for k in ("q", "count", "alive"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k, np.argwhere(_bits(got[k]) != _bits(want[k]))[:8])
    g, w = got["target"], want["target"]
    assert g.shape == w.shape and g.dtype == w.dtype
    if temperature == 0.0:
        assert np.array_equal(_bits(g), _bits(w)), (what, "target", np.argwhere(_bits(g) != _bits(w))[:8])
    else:
        assert np.array_equal(g != 0, w != 0), (what, "target pattern")
        ulp = np.spacing(np.abs(w))
        err = np.abs(g.astype(np.float64) - w.astype(np.float64))
        print(f"{what}: worst target error {float((err / np.maximum(ulp, 1e-300)).max()):.3f} ulp")
        assert (err <= ulp).all(), (what, "target", float((err / ulp).max()))


@pytest.mark.parametrize("cid,M,K,per_state,seed", CASES, ids=[c[0] for c in CASES])
def test_equals_the_reference(cid, M, K, per_state, seed):
    c = V.case(M, K, per_state, seed)
    for T in V.TEMPERATURES:
        want = V.action_values(c["ret"], c["first"], c["steps"], c["status"], c["active"], temperature=T, prev=_sentinel_ref(M))
        got = _call(c, T, _sentinel(M))
        _compare(got, want, T, (cid, T))
        if M >= 4:      # the inactive row between two active ones: not one byte written
            for k in got:
                assert (got[k][2] == V.SENTINEL).all(), (cid, k)
    # steps / status both NULL: alive iff count > 0
    want = V.action_values(c["ret"], c["first"], active=c["active"], temperature=1.0, prev=_sentinel_ref(M))
    _compare(_call(c, 1.0, _sentinel(M), status=False), want, 1.0, (cid, "no status"))
    # active NULL: every row; target NULL: the sentinel stays
    want = V.action_values(c["ret"], c["first"], c["steps"], c["status"], temperature=0.0)
    got = _call(c, 0.0, _sentinel(M), active=False, target=False)
    assert (got["target"] == V.SENTINEL).all()
    got["target"] = want["target"]
    _compare(got, want, 0.0, (cid, "no active, no target"))


@pytest.mark.parametrize("M,Ks,per_state", [(5, (9, 65, 17), True), (4, (64, 64, 129), False), (9, (1, 1, 1), True), (3, (4096, 63, 9), True)])
def test_accumulation_equals_the_concatenated_tables(M, Ks, per_state):
    parts = [V.case(M, K, per_state, 70 + i) for i, K in enumerate(Ks)]
    for c in parts:
        c["active"] = parts[0]["active"]
    for T in (0.0, 0.05):
        out = _sentinel(M)
        for i, c in enumerate(parts):
            got = _call(c, T, out, accumulate=int(i > 0))
        cat = {k: np.concatenate([np.broadcast_to(c[k], (M, c["ret"].shape[1])) for c in parts], axis=1) for k in ("ret", "first", "steps", "status")}
        want = V.action_values(cat["ret"], cat["first"], cat["steps"], cat["status"], parts[0]["active"], temperature=T, prev=_sentinel_ref(M))
        _compare(got, want, T, ("accumulate", M, Ks, T))


@pytest.mark.parametrize("M,K", [(9, 129), (5, 4096)])
def test_two_calls_give_the_same_bits(M, K):
    c = V.case(M, K, True, 5)
    a, b = _call(c, 0.05, _sentinel(M)), _call(c, 0.05, _sentinel(M))
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_end_to_end_on_the_scoring_launch():
    """33 harvested states of big_track at 16 rays, (K, H) = (70, 3): K28 on K22's outputs equals the reference on the same outputs, and
    agrees with the scoring launch's own best sequence."""
    K, H, M = 70, 3, 33
    s = {k: np.asarray(v)[:M] for k, v in Q.states("big_track", 16, "pre_crash").items()}
    env = pc.VecCarEnv(1, TRACKS["big_track"], num_rays=16, reward_scaling=R.REWARD_SCALE, dtype="f64")
    table = _dev(Q.table(H, K), torch.uint8)
    t = {k: _dev(s[k], torch.float64) for k in ("px", "py", "vx", "vy")}
    out = env.rollout_sequences(t["px"], t["py"], t["vx"], t["vy"], _dev(s["turns"], torch.int32), table,
                                next_gate=_dev(s["next_gate"], torch.int32), time_step=_dev(s["time_step"], torch.int32))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    c = dict(ret=host["ret"], first=Q.table(H, K)[0], steps=host["steps"], status=host["status"], active=np.ones(M, np.uint8))
    for T in (0.0, 0.05):
        got = _call(c, T, _sentinel(M))
        want = V.action_values(c["ret"], c["first"], c["steps"], c["status"], temperature=T)
        _compare(got, want, T, ("end to end", T))
    rows = np.arange(M)
    assert np.array_equal(_bits(got["q"][rows, host["best_action"]]), _bits(host["best_ret"]))
    assert np.array_equal(host["best_ret"], got["q"].max(1))
    env.close()
