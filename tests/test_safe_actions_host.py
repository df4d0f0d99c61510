"""Safe-action masks, the parts that need no GPU: the C-ABI's symbols and argument checks, the plain reference (safe_actions_reference.py)
against step_poses_reference.step and its own monotonicity, the recipes' class counts, and PolicyLandscape.viability() on a stand-in
envs / agent pair whose safe_actions() calls a search written here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from ppo_car_amd import _capi
from ppo_car_amd import landscape as L
from conftest import ROOT
import step_poses_reference as R
import safe_actions_reference as S
from test_step_poses_host import FakeAgent, FakeEnvs, _road

INV = _capi.PC_ERR_INVALID_ARG
P = 4096      # a non-NULL address: every call below is refused before any device call, so it is never dereferenced


def test_symbols_exported_with_signatures():
    lib = C.CDLL(_capi.lib_path())
    for name in ("pc_env_safe_actions", "pc_env_safe_actions_state"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.EXPORTS
    f = _capi.lib.pc_env_safe_actions
    assert f.restype is C.c_int and list(f.argtypes) == [C.c_void_p] * 9 + [C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    g = _capi.lib.pc_env_safe_actions_state
    assert g.restype is C.c_int and list(g.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    assert re.search(r"int pc_env_safe_actions\(const pc_env\* e, const double\* px, const double\* py, const double\* vx, const double\* vy,\s*"
                     r"const int32_t\* turns, const int32_t\* time_step, const uint8_t\* track_id, const uint8_t\* active, int64_t M,\s*"
                     r"int depth, uint8_t\* safe, void\* stream\);", hdr)
    assert re.search(r"int pc_env_safe_actions_state\(pc_env\* e, int depth, uint8_t\* safe, void\* stream\);", hdr)
    assert re.search(r"#define PC_SAFE_MAX_DEPTH 4\b", hdr) and _capi.PC_SAFE_MAX_DEPTH == 4


ARGS = ("e", "px", "py", "vx", "vy", "turns", "time_step", "track_id", "active", "M", "depth", "safe", "stream")


def _call(**kw):
    a = {k: P for k in ARGS}
    a.update(M=8, depth=2, stream=None)
    a.update(kw)
    return _capi.lib.pc_env_safe_actions(*[a[k] for k in ARGS])


@pytest.mark.parametrize("kw", [dict(e=None)] + [dict([(k, None)]) for k in ("px", "py", "vx", "vy", "turns", "safe")]
                         + [dict(M=0), dict(M=-5), dict(depth=0), dict(depth=5), dict(depth=-1), dict(depth=1 << 20),
                            dict(e=None, px=None, M=0, depth=0), dict(px=None, M=0, depth=9), dict(M=0, depth=9),
                            dict(depth=0, time_step=None, track_id=None, active=None)])
def test_argument_errors_before_any_device_call(kw):
    # (the handle is a made-up address too: the refusal comes before the handle is looked at)
    assert _call(**kw) == INV


@pytest.mark.parametrize("args", [(None, 2, P), (P, 2, None), (P, 0, P), (P, 5, P), (None, 0, None)])
def test_state_form_argument_errors_before_any_device_call(args):
    assert _capi.lib.pc_env_safe_actions_state(*args, None) == INV


# ---- the reference and the recipes -----------------------------------------------------------------------------------------------
def test_sequences_put_the_first_action_first():
    seq = S.sequences(3)
    assert seq.shape == (729, 3) and np.array_equal(seq[0], [0, 0, 0]) and np.array_equal(seq[1], [0, 0, 1]) and np.array_equal(seq[81], [1, 0, 0])
    assert len({tuple(r) for r in seq}) == 729


@pytest.mark.parametrize("track,n", S.CONFIGS)
def test_reference_depth_1_is_not_terminated_under_each_action(track, n):
    for recipe in ("edge", "near_gate", "pre_crash"):
        s, m = S.reference(track, n, recipe, 3)
        rows, acts = R.all_actions({k: s[k] for k in S.STATE_KEYS})
        ref = R.step(track, n, rows, acts)
        assert np.array_equal(m[0], ~ref["terminated"].reshape(9, -1).T), recipe


@pytest.mark.parametrize("track,n", S.CONFIGS)
def test_reference_masks_shrink_with_depth_and_truncation_is_safe(track, n):
    for recipe in ("edge", "near_gate", "pre_crash"):
        s, m = S.reference(track, n, recipe, 3)
        for d in (1, 2):
            assert not (m[d] & ~m[d - 1]).any(), (recipe, d)      # mask(d + 1) is a subset of mask(d)
        last = np.asarray(s["time_step"]) == 999                  # the step truncates unless it crashes: every depth's mask is depth 1's
        if recipe != "pre_crash":
            assert last.any()
        for d in (1, 2):
            assert np.array_equal(m[d][last], m[0][last]), (recipe, d)
    s, m = S.reference(track, n, "pre_crash", 3)
    assert (m[0] & ~m[2]).any()      # ... and a proper one somewhere: deeper searches do find doom the first step does not show


@pytest.mark.parametrize("track,n", S.CONFIGS)
def test_recipes_give_the_recorded_class_counts(track, n):
    s, m = S.reference(track, n, "pre_crash", 3)
    M = len(s["px"])
    rows, counts = S.PRE_CRASH_COUNTS[(track, n)]
    assert M == rows and [S.classes(x) for x in m] == counts
    for d, c in enumerate(counts):
        for share, need in zip(c, S.SHARES):
            assert share >= need * M, (d + 1, c)
    assert np.array_equal(s["rot"], S.with_turns(track, s)["rot"])      # on the one-way row of the turn count
    assert [S.classes(x) for x in S.reference(track, n, "edge", 3)[1]] == S.EDGE_COUNTS[(track, n)]
    assert [S.classes(x) for x in S.reference(track, n, "near_gate", 3)[1]] == [(0, 0, 240)] * 3


def test_one_run_gives_every_depth():
    track, n = "big_track", 16
    s, m = S.reference(track, n, "pre_crash", 3)
    sub = {k: v[:40] for k, v in s.items()}
    for d in (1, 2):
        assert np.array_equal(S.masks(track, n, sub, d)[-1], m[d - 1][:40])


# ---- PolicyLandscape.viability() on a stand-in world (torch CPU) ----------------------------------------------------------------------
class SafeEnvs(FakeEnvs):
    """test_step_poses_host's strip world with a safe_actions() that searches it: action 0 moves one cell right, 1 one cell left, the
    rest stay; a step terminates off the road and anywhere in the lethal top row.  No time limit."""

    def __init__(self, angles, cell):
        super().__init__(angles, cell)
        self.calls = []

    def _search(self, px, py, depth):
        """[M] bool per first action 0 / 1 / stay: some sequence of `depth` steps that starts with it never terminates"""
        if depth == 0:
            return None
        out = []
        for move in (1.0, -1.0, 0.0):
            x = px + self.cell * move
            ok = _road(x) & ~(py < self.cell)
            if depth > 1:
                ok = ok & torch.stack(self._search(x, py, depth - 1)).any(0)
            out.append(ok)
        return out

    def safe_actions(self, px, py, vx, vy, turns, depth=1, time_step=None, track_id=None, active=None, out=None):
        assert active is not None and active.dtype == torch.uint8 and out.dtype == torch.uint8 and out.shape == (px.numel(), 9)
        assert time_step is None and track_id is not None
        self.calls.append((px.numel(), depth))
        right, left, stay = self._search(px, py, depth)
        on = active != 0
        before = out.clone()
        full = torch.stack([right, left] + [stay] * 7, 1).to(torch.uint8)
        out[on] = full[on]
        assert torch.equal(before[~on], out[~on])      # an inactive row keeps its bytes
        return out.view(torch.bool)


@pytest.mark.parametrize("cell,chunks", [(80, [20736]), (20, [1 << 18, 2 * 72 * 36 * 64 - (1 << 18)])])
def test_viability_known_answer(cell, chunks, tmp_path):
    D = 3
    envs, agent = SafeEnvs([0.0, 90.0], cell), FakeAgent()
    ls = L.PolicyLandscape(agent, None, 16, cell_px=cell, speed=0.5, device="cpu", envs=envs)
    with pytest.raises(RuntimeError):
        ls.viability(D)
    poses0 = [t.clone() for t in ls.poses()]
    assert ls.compute().viability(D) is ls
    assert envs.calls == [(c, D) for c in chunks] and not envs.steps      # one search per chunk, not one step
    for a, b in zip(poses0, ls.poses()):
        assert torch.equal(a, b)
    GH, GW = 720 // cell, 1280 // cell
    px, py, vx, vy, turns, tid = (t.reshape(2, 72, GH, GW) for t in ls.poses())
    idx = torch.arange(GW).expand(2, 72, GH, GW)
    lo, hi = 640 // cell, 1200 // cell - 1      # the road's first and last cell
    road = (idx >= lo) & (idx <= hi)
    lethal = py < cell
    live = road & ~lethal
    # staying is always safe on the road below the top row, so a first move is safe iff it ends on the road
    want = torch.where(live, 0x1fc + (idx < hi).to(torch.int64) + 2 * (idx > lo).to(torch.int64), torch.zeros_like(idx))
    assert ls.viable.dtype == torch.uint16 and ls.viable.shape == (2, 72, GH, GW) and ls.viability_depth == D
    assert torch.equal(ls.viable.to(torch.int64), want)
    assert ls.doomed.dtype == torch.bool and torch.equal(ls.doomed, road & lethal) and ls.doomed.any()
    right = turns < 36
    late = live & torch.where(right, idx == hi, idx == lo)      # the greedy action drives off the road's end; the others do not
    assert ls.avoidable_late.dtype == torch.bool and torch.equal(ls.avoidable_late, late) and late.any()
    assert not ls.viable.to(torch.int64)[~ls.drivable].any()
    count = ls.viable_count(0)
    assert torch.equal(count.isnan(), ~ls.drivable[0].any(0)) and float(count[~count.isnan()].max()) == 9.0
    if cell == 80:
        ls.lookahead()
        bits = ls.viability(1).viable.to(torch.int64)
        assert torch.equal(sum((bits >> a) & 1 for a in range(9)).to(torch.uint8), ls.safe_actions)      # depth 1 is the look-ahead
        assert torch.equal(ls.avoidable_late, ls.avoidable)
        files = ls.save(str(tmp_path / "out" / "run"))
        assert [os.path.basename(f) for f in files] == ["run_landscape.npz", "run_landscape_track0.png", "run_landscape_track1.png",
                                                        "run_viability_track0.png", "run_viability_track1.png"]
        z = np.load(files[0])
        for k in ("viable", "doomed", "avoidable_late"):
            assert np.array_equal(z[k], getattr(ls, k).numpy()), k
        assert z["viable"].dtype == np.uint16 and int(z["viability_depth"]) == 1 and all(os.path.getsize(f) > 0 for f in files)
    ls.close()


def test_save_without_viability_writes_the_keys_it_always_wrote(tmp_path):
    ls = L.PolicyLandscape(FakeAgent(), None, 16, cell_px=80, speed=0.5, device="cpu", envs=SafeEnvs([0.0], 80))
    files = ls.compute().lookahead().save(str(tmp_path / "run"))
    assert [os.path.basename(f) for f in files] == ["run_landscape.npz", "run_landscape_track0.png"]
    assert sorted(np.load(files[0]).files) == sorted(["value", "action", "drivable", "best_value", "best_heading", "action_at_best", "cell_px",
                                                      "speed", "tracks", "safe_actions", "greedy_crashes", "avoidable"])
    ls.close()
