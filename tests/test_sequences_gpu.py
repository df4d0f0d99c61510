"""K22 (pc_env_rollout_sequences / pc_env_rollout_sequences_state; VecCarEnv.rollout_sequences / score_sequences), the shooting Planner
and its evaluation on the GPU.

Every comparison is an equality of bits.  F64 handles against the CPU oracle (sequences_reference.rollout), F32 handles against H
chained pc_env_step_poses calls on the same handle over the replicated rows, the ended rows frozen with `active`."""
import json

import numpy as np
import pytest
import torch

import ppo_car_amd as pc
from ppo_car_amd import _capi
from ppo_car_amd.evaluation import EVAL_KEYS, state_totals
from conftest import TRACKS
from first_episode_reference import first_episodes_ref
import oracle
import step_poses_reference as R
import sequences_reference as Q
import ray_counts_reference as rc
from test_sequences_host import PLAN_H, PLAN_K, PLAN_ROUNDS, PLAN_SEED

pytestmark = pytest.mark.gpu

F64_KEYS = ("px", "py", "vx", "vy")
OUT = (("ret", torch.float64, True), ("steps", torch.int32, True), ("status", torch.uint8, True), ("gates", torch.int32, True),
       ("laps", torch.int32, True), ("best_k", torch.int32, False), ("best_action", torch.int64, False), ("best_ret", torch.float64, False))
REQUIRED = ("ret", "steps", "status")
SENTINEL = 77


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _same(got, want, keys, what):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(_bits(g), _bits(w)), (what, k, np.argwhere(_bits(g) != _bits(w))[:8])


def _env(track, n, dtype, N=1):
    return pc.VecCarEnv(N, TRACKS[track], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype=dtype)


def _filled(M, K, keys):
    """output tensors pre-filled with a sentinel"""
    return {name: torch.full((M, K) if per_lane else (M,), SENTINEL, dtype=dtype, device="cuda") for name, dtype, per_lane in OUT if name in keys}


def _score(env, s, table, keys=tuple(o[0] for o in OUT), track_id=None, active=None, defaults=False):
    """One rollout_sequences call on device copies of the numpy rows s, the outputs pre-filled with a sentinel: dict of numpy arrays.
    The inputs must come back as they went in.  defaults: next_gate and time_step left out (NULL = 0)."""
    t = {k: _dev(s[k], torch.float64) for k in F64_KEYS}
    t["turns"] = _dev(s["turns"], torch.int32)
    if not defaults:
        t["next_gate"], t["time_step"] = _dev(s["next_gate"], torch.int32), _dev(s["time_step"], torch.int32)
    if track_id is not None:
        t["track_id"] = _dev(track_id, torch.uint8)
    if active is not None:
        t["active"] = _dev(active, torch.uint8)
    t["actions"] = _dev(table, torch.uint8)
    keep = {k: v.clone() for k, v in t.items()}
    M, K = len(s["px"]), t["actions"].shape[-1]
    out = _filled(M, K, keys)
    got = env.rollout_sequences(t["px"], t["py"], t["vx"], t["vy"], t["turns"], t["actions"], next_gate=t.get("next_gate"),
                                time_step=t.get("time_step"), track_id=t.get("track_id"), active=t.get("active"), out=out)
    assert set(got) == set(keys) and all(got[k].data_ptr() == out[k].data_ptr() for k in keys)
    for k in t:
        assert torch.equal(t[k], keep[k]), k      # read only
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- 1. F64 handles: the CPU oracle ----------------------------------------------------------------------------------------------------
OFF_MENU = [(rc.TRACK_OF[n], n) for n in (11, 90)]      # tests/ray_counts_reference.py: six collision rays; collision rays past the 64-bit mask


@pytest.mark.parametrize("K,H", [(64, 1), (64, 3), (64, 12), (70, 12), (1, 12)])
@pytest.mark.parametrize("track,n", Q.CONFIGS)
def test_f64_equals_the_reference(track, n, K, H):
    _f64_equals_the_reference(track, n, K, H)


@pytest.mark.parametrize("track,n", OFF_MENU)
def test_off_menu_ray_counts_f64_equals_the_reference(track, n):
    _f64_equals_the_reference(track, n, 70, 3)


def _f64_equals_the_reference(track, n, K, H):
    env = _env(track, n, "f64")
    for recipe in Q.RECIPES:
        s, ref = Q.reference(track, n, recipe, H, K)
        got = _score(env, s, Q.table(H, K))
        _same(got, ref, Q.OUT_KEYS + Q.BEST_KEYS, (recipe, "all"))
        part = _score(env, s, Q.table(H, K), keys=REQUIRED)      # gates, laps and best_* NULL
        _same(part, ref, REQUIRED, (recipe, "required only"))
    env.close()


# ---- 2. F32 handles: H chained K20 calls on the same handle ----------------------------------------------------------------------------
def _chained(env, s, table, track_id=None):
    """Q.rollout's loop with pc_env_step_poses on `env` in the oracle's place: dict of numpy arrays over Q.OUT_KEYS + Q.BEST_KEYS"""
    M = len(s["px"])
    table = np.asarray(table)
    tabs = np.broadcast_to(table, (M,) + table.shape) if table.ndim == 2 else table
    H, K = tabs.shape[1:]
    rep = lambda a, dt: _dev(np.repeat(np.asarray(a), K), dt)
    px, py, vx, vy = (rep(s[k], torch.float64) for k in F64_KEYS)
    turns, ng, ts = rep(s["turns"], torch.int32), rep(s["next_gate"], torch.int32), rep(s["time_step"], torch.int32)
    tid = None if track_id is None else rep(track_id, torch.uint8)
    ret = torch.zeros(M * K, dtype=torch.float64, device="cuda")
    steps, gates, laps = (torch.zeros(M * K, dtype=torch.int32, device="cuda") for _ in range(3))
    status = torch.zeros(M * K, dtype=torch.uint8, device="cuda")
    for t in range(H):
        live = status == Q.RUNNING
        acts = _dev(np.minimum(tabs[:, t, :].reshape(-1), 8), torch.int64)
        r = env.step_poses(px, py, vx, vy, turns, acts, next_gate=ng, time_step=ts, track_id=tid, active=live.to(torch.uint8))
        zero = torch.zeros_like(ret)      # (a frozen row's outputs are stale)
        ret += torch.where(live, r.reward.to(torch.float64), zero)
        steps += live.to(torch.int32)
        gate = live & (r.gate != 0)
        gates += gate.to(torch.int32)
        laps += (gate & (ng == 0)).to(torch.int32)
        now = torch.where(r.terminated != 0, Q.TERMINATED, torch.where(r.truncated != 0, Q.TRUNCATED, Q.RUNNING)).to(torch.uint8)
        status = torch.where(live, now, status)
    out = {k: v.reshape(M, K).cpu().numpy() for k, v in dict(ret=ret, steps=steps, status=status, gates=gates, laps=laps).items()}
    out["best_k"] = out["ret"].argmax(1).astype(np.int32)
    out["best_action"] = np.minimum(tabs[np.arange(M), 0, out["best_k"]], 8).astype(np.int64)
    out["best_ret"] = out["ret"][np.arange(M), out["best_k"]]
    return out


@pytest.mark.parametrize("track,n", Q.CONFIGS)
def test_f32_equals_chained_step_poses(track, n):
    _f32_equals_chained_step_poses(track, n, Q.K_REF, Q.H_REF)


@pytest.mark.parametrize("track,n", OFF_MENU)
def test_off_menu_ray_counts_f32_equals_chained_step_poses(track, n):
    _f32_equals_chained_step_poses(track, n, 70, 3)


def _f32_equals_chained_step_poses(track, n, K, H):
    env, env64 = _env(track, n, "f32"), _env(track, n, "f64")
    left_out = pairs = 0
    for recipe in Q.RECIPES:
        s, ref = Q.reference(track, n, recipe, H, K)
        got = _score(env, s, Q.table(H, K))
        _same(got, _chained(env, s, Q.table(H, K)), Q.OUT_KEYS + Q.BEST_KEYS, recipe)
        # status and steps are the F64 handle's wherever no collision ray of the F64 reference comes within 1e-6 px of the 10 px threshold
        f64 = _score(env64, s, Q.table(H, K), keys=REQUIRED)
        clear = ~ref["near10"]
        left_out += int(ref["near10"].sum())
        pairs += clear.size
        for k in ("status", "steps"):
            assert np.array_equal(got[k][clear], f64[k][clear]), (recipe, k, np.argwhere((got[k] != f64[k]) & clear)[:8])
    print(f"{track} {n}: {left_out} of {pairs} (state, sequence) pairs left out of the F32 / F64 comparison (a ray within 1e-6 px of 10 px)")
    assert left_out <= 0.01 * pairs
    env.close(); env64.close()


# ---- 3. per-state tables ---------------------------------------------------------------------------------------------------------------
def _mixed_rows(track, n, M):
    s, _ = Q.pooled(track, n)
    perm = np.random.default_rng(3).permutation(len(s["px"]))[:M]
    return {k: v[perm] for k, v in s.items()}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_per_state_tables_equal_single_state_calls(dtype):
    track, n, M, H, K = "big_track", 16, 37, 7, 20
    s = _mixed_rows(track, n, M)
    tabs = np.stack([Q.table(H, K, seed=100 + m) for m in range(M)])
    assert len({t.tobytes() for t in tabs}) == M
    env = _env(track, n, dtype)
    got = _score(env, s, tabs)
    assert len(np.unique(got["status"])) == 3
    for m in range(M):
        one = _score(env, {k: v[m:m + 1] for k, v in s.items()}, tabs[m])
        _same({k: got[k][m:m + 1] for k in got}, one, Q.OUT_KEYS + Q.BEST_KEYS, m)
    if dtype == "f64":
        _same(got, Q.rollout(track, n, s, tabs), Q.OUT_KEYS + Q.BEST_KEYS, "oracle")
    else:
        _same(got, _chained(env, s, tabs), Q.OUT_KEYS + Q.BEST_KEYS, "chain")
    env.close()


# ---- 4. the state form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("track,n", [("big_track", 16), ("track", 12)])
def test_state_form_equals_poses_form_and_leaves_the_state_alone(track, n, dtype):
    s, _ = Q.pooled(track, n)
    N, H, K = len(s["px"]), 12, 64
    env = _env(track, n, dtype, N)
    env.reset()
    env.set_state(passed=0, **{k: s[k] for k in Q.STATE_KEYS})
    before = env.get_state()
    table = _dev(Q.table(H, K), torch.uint8)
    out = _filled(N, K, [o[0] for o in OUT])
    got = env.score_sequences(table, out=out)
    assert set(got) == set(out)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    # the rotation a turn count names is the one-way sum; the recipes' rows lie on it
    on_row = np.array([Q.S.rot_after(R.track(track).start_rot, int(k)) == r for k, r in zip(s["turns"], s["rot"])])
    assert on_row.sum() > N // 2
    if dtype == "f32":
        on_row[:] = True      # (the turn count is all an F32 handle keeps of a rotation)
    want = _score(env, s, Q.table(H, K))
    _same({k: v[on_row] for k, v in got.items()}, {k: v[on_row] for k, v in want.items()}, Q.OUT_KEYS + Q.BEST_KEYS, "poses form")
    if dtype == "f64":      # every row, from the env's own rotation
        _same(got, Q.rollout(track, n, s, Q.table(H, K)), Q.OUT_KEYS + Q.BEST_KEYS, "oracle")
    part = env.score_sequences(table)      # allocating; then with the optional arrays left out
    _same({k: v.cpu().numpy() for k, v in part.items()}, got, Q.OUT_KEYS + Q.BEST_KEYS, "allocated")
    req = env.score_sequences(table, out=_filled(N, K, REQUIRED))
    assert set(req) == set(REQUIRED)
    _same({k: v.cpu().numpy() for k, v in req.items()}, got, REQUIRED, "required only")
    after = env.get_state()
    for k in before:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k      # the env state is not touched
    env.close()


# ---- 5. rows that are not rolled out, out-of-range action bytes --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_inactive_rows_unknown_tracks_and_action_bytes(dtype):
    track, n, M, H, K = "big_track", 16, 257, 6, 13      # 257 x 13 lanes: no multiple of a wave or a workgroup
    s = _mixed_rows(track, n, M)
    env = _env(track, n, dtype, 3)
    env.reset()
    before = env.get_state()
    table = Q.table(H, K)
    full = _score(env, s, table)
    assert len(np.unique(full["status"])) == 3 and (full["steps"] >= 1).all() and (full["steps"] <= H).all()
    _same(_score(env, s, table), full, Q.OUT_KEYS + Q.BEST_KEYS, "repeat")
    # active == 0: the sentinel stays in every output array
    active = (np.arange(M) % 3 != 1).astype(np.uint8)
    part = _score(env, s, table, active=active)
    on = active != 0
    for k in Q.OUT_KEYS + Q.BEST_KEYS:
        assert np.array_equal(_bits(part[k][on]), _bits(full[k][on])), k
        assert (part[k][~on] == SENTINEL).all(), k
    # a track the handle does not have: the documented zeros
    tid = np.zeros(M, np.uint8)
    tid[[0, 100, 256]] = (1, 255, 7)
    bad = tid != 0
    got = _score(env, s, table, track_id=tid)
    for k in Q.OUT_KEYS + Q.BEST_KEYS:
        assert np.array_equal(_bits(got[k][~bad]), _bits(full[k][~bad])), k
        assert (got[k][bad] == (8 if k == "best_action" else 0)).all(), k
    assert got["status"].dtype == np.uint8 and _capi.PC_FIRST_RUNNING == 0
    both = _score(env, s, table, track_id=tid, active=active)
    for k in Q.OUT_KEYS + Q.BEST_KEYS:
        assert np.array_equal(_bits(both[k][on]), _bits(got[k][on])) and (both[k][~on] == SENTINEL).all(), k
    # an action byte outside 0 .. 8 acts as 8, and best_action reports 8
    eight = table.copy()
    eight[2, 10] = eight[4, 12] = eight[0, 9] = 8      # drawn columns with an 8, the first step included
    odd = eight.copy()
    where = eight == 8
    odd[where] = 200
    odd[:, 8], eight[:, 8] = 9, 8
    odd[0, 8] = 255
    a, b = _score(env, s, odd), _score(env, s, eight)
    _same(a, b, Q.OUT_KEYS + Q.BEST_KEYS, "bytes above 8")
    assert (a["best_action"] <= 8).all()
    # next_gate and time_step NULL mean 0
    zero = dict(s, next_gate=np.zeros(M, np.int64), time_step=np.zeros(M, np.int64))
    _same(_score(env, s, table, defaults=True), _score(env, zero, table), Q.OUT_KEYS + Q.BEST_KEYS, "defaults")
    after = env.get_state()
    for k in before:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k      # the handle's own state is neither read nor written
    env.close()


# ---- 6. two tracks in one wave ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_two_tracks_in_one_wave(dtype):
    n, M, H, K = 16, 200, 8, 9      # 7 states per wave: both tracks sit in every wave
    s = _mixed_rows("big_track", n, M)
    table = Q.table(H, K)
    singles = []
    for track in ("track", "big_track"):
        env = _env(track, n, dtype)
        singles.append(_score(env, s, table))
        env.close()
    env = pc.VecCarEnv(2, [TRACKS["track"], TRACKS["big_track"]], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype=dtype,
                       track_id=np.array([0, 1], np.uint8))
    tid = (np.arange(M) & 1).astype(np.uint8)
    both = _score(env, s, table, track_id=tid)
    for k in (0, 1):
        sel = tid == k
        _same({key: both[key][sel] for key in both}, {key: singles[k][key][sel] for key in both}, Q.OUT_KEYS + Q.BEST_KEYS, k)
    assert not np.array_equal(both["ret"][0::2], singles[1]["ret"][0::2])      # (the two tracks do differ)
    env.close()


# ---- 7. the planner ------------------------------------------------------------------------------------------------------------------
def test_planner_equals_the_oracle_planning_on_its_own_state():
    track, n, N = "big_track", 16, 64
    pre, near = Q.states(track, n, "pre_crash"), Q.states(track, n, "near_gate")
    s0 = {k: np.stack([np.asarray(pre[k][:N // 2]), np.asarray(near[k][:N // 2])], 1).reshape(-1) for k in Q.STATE_KEYS}      # interleaved
    env = _env(track, n, "f64", N)
    env.reset()
    env.set_state(passed=0, **s0)
    orc = oracle.OracleVecEnv(R.track(track), N, n, reward_scaling=R.REWARD_SCALE)
    orc.reset()
    orc.set_state(passed=0, destroyed=0, **s0)
    planner = pc.Planner(env, horizon=PLAN_H, candidates=PLAN_K, seed=PLAN_SEED)
    taken, done = [], 0
    for step in range(PLAN_ROUNDS):
        table, _ = Q.planner_draw(PLAN_H, PLAN_K, PLAN_SEED, step)
        act = planner.act(step)
        assert act.dtype == torch.int64 and act.shape == (N,)
        assert np.array_equal(planner.table.cpu().numpy(), table), step
        want = Q.rollout(track, n, {k: getattr(orc, k).copy() for k in Q.STATE_KEYS}, table)
        got = {k: v.cpu().numpy() for k, v in planner.out.items()}
        _same(got, want, REQUIRED + Q.BEST_KEYS, step)
        taken.append(got["best_action"].copy())
        _, _, term, trunc, _ = env.step(act)
        _, _, oterm, otrunc = orc.step(want["best_action"])
        assert np.array_equal(term.cpu().numpy() != 0, oterm) and np.array_equal(trunc.cpu().numpy() != 0, otrunc), step
        done += int(oterm.sum() + otrunc.sum())
    assert done > 0 and len({a.tobytes() for a in taken}) > 1      # auto-resets included; the plans do change
    st = env.get_state()
    for k in Q.STATE_KEYS:
        assert np.array_equal(_bits(st[k]), _bits(getattr(orc, k).astype(st[k].dtype))), k
    # the same seed gives the same actions on a second Planner (from the same states)
    env.set_state(passed=0, **s0)
    again = pc.Planner(env, horizon=PLAN_H, candidates=PLAN_K, seed=PLAN_SEED)
    for step in range(PLAN_ROUNDS):
        act = again.act(step)
        assert np.array_equal(act.cpu().numpy(), taken[step]), step
        env.step(act)
    other = pc.Planner(env, horizon=PLAN_H, candidates=PLAN_K, seed=PLAN_SEED + 1)
    assert not np.array_equal(other.candidate_table(0).cpu().numpy(), Q.planner_draw(PLAN_H, PLAN_K, PLAN_SEED, 0)[0])
    env.close()


def test_planner_drive_returns_the_rows_of_its_steps():
    env = _env("big_track", 16, "f32", 16)
    env.reset()
    planner = pc.Planner(env, horizon=4, candidates=16, seed=1)
    rew, term, trunc = planner.drive(5, start=40)
    assert rew.shape == term.shape == trunc.shape == (5, 16) and rew.dtype == torch.float32
    env.reset()
    for t in range(5):
        _, r, te, tr, _ = env.step(planner.act(40 + t))
        assert torch.equal(r, rew[t]) and torch.equal(te, term[t]) and torch.equal(tr, trunc[t])
    env.close()


# ---- 8. the planner's evaluation -------------------------------------------------------------------------------------------------------
def test_planner_evaluation_totals_equal_a_host_scan():
    N = 64
    ev = pc.PlannerEvaluator(TRACKS["big_track"], n_envs=N, num_rays=16, reward_scaling=0.1, horizon=8, candidates=32, seed=2)
    out = ev.evaluate()
    assert set(out) == set(EVAL_KEYS) and out["eval/episodes"] == N and ev.last_path == "planner"
    state = ev.state.cpu().numpy()
    want = first_episodes_ref(ev.rew.cpu().numpy(), ev.term.cpu().numpy(), ev.trunc.cpu().numpy(), 0.1)
    assert np.array_equal(_bits(state), _bits(want))
    assert (state[4] != 0).all()      # every env closed its first episode
    tot = ev.totals().cpu().numpy()
    ref_tot = state_totals(torch.from_numpy(want).cuda(), torch.zeros(1, dtype=torch.int32, device="cuda")).cpu().numpy()
    assert np.array_equal(_bits(tot), _bits(ref_tot))
    lapped = np.isfinite(want[7])
    exact = {0: N, 4: want[1].sum(), 5: want[2].sum(), 6: want[3].sum(), 7: (want[4] == 1).sum(), 8: want[5].sum(), 9: want[6].min(),
             10: lapped.sum(), 11: want[7][lapped].sum(), 12: 0}      # the integer-valued totals, and the extrema
    for i, v in exact.items():
        assert tot[i] == v, (i, tot[i], v)
    assert tot[2] == want[0].min() and tot[3] == want[0].max() and abs(tot[1] - want[0].sum()) <= 1e-9 * max(1.0, abs(want[0].sum()))
    assert out == ev.scalars(tot.tolist())
    assert out["eval/episodic_length"] == want[1].sum() / N and out["eval/crash_rate"] == (want[4] == 1).sum() / N
    # a second run gives the same bits
    ev.run()
    assert np.array_equal(_bits(ev.state.cpu().numpy()), _bits(state))
    ev.close()


def test_evaluate_planner_prints_the_policy_evaluations_keys(capsys):
    import evaluate
    out = evaluate.main(["--planner", "shooting", "--plan-horizon", "8", "--plan-candidates", "32", "--envs", "64", "--track",
                         TRACKS["big_track"], "--num-rays", "16"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    assert {k for k in out if k.startswith("eval/")} == set(EVAL_KEYS)      # exactly the policy evaluation's eval/* keys
    assert out["eval/episodes"] == 64 and out["path"] == "planner"
    assert out["planner"] == {"kind": "shooting", "horizon": 8, "candidates": 32}
    assert 0.0 <= out["eval/crash_rate"] <= 1.0 and 1.0 <= out["eval/episodic_length"] <= 1000.0
