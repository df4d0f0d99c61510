"""K23 / K24 (pc_cem_sample, pc_cem_refit), CEMPlanner and its evaluation on the GPU.

Every comparison is an equality of bits: the two kernels against cem_reference.py on hand-made inputs, CEMPlanner.plan on an F64 handle
against the reference loop scored by the CPU oracle, on an F32 handle against the same loop scored by that handle's own K22 (which
test_sequences_gpu.py holds to chained K20)."""
import itertools
import json

import numpy as np
import pytest
import torch

import ppo_car_amd as pc
from ppo_car_amd import _capi
from ppo_car_amd.evaluation import EVAL_KEYS
from conftest import TRACKS
from first_episode_reference import first_episodes_ref
import oracle
import step_poses_reference as R
import sequences_reference as Q
import cem_reference as X
from test_sequences_host import PLAN_H, PLAN_K, PLAN_SEED

pytestmark = pytest.mark.gpu

SENTINEL = 77
F64_KEYS = ("px", "py", "vx", "vy")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _weights(w):
    """uint32 numpy weights -> the int32 device tensor that holds the same bits"""
    return _dev(np.ascontiguousarray(w, np.uint32).view(np.int32))


def _back(t):
    return t.cpu().numpy().view(np.uint32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(_bits(got), _bits(want)), (what, np.argwhere(_bits(got) != _bits(want))[:8])


# ---- 1. pc_cem_sample ------------------------------------------------------------------------------------------------------------------
def _sample_weights():
    """[3, 5, 9]: rows with zeros, one-hot rows, an all-zero row, 65536, values above 65536 (the largest uint32 among them)"""
    w = np.random.default_rng(1).integers(0, 3000, (3, 5, 9)).astype(np.uint32)
    w[0, 0, [1, 4, 8]] = 0
    w[0, 1] = 0
    w[0, 1, 6] = 9          # one-hot
    w[0, 2] = 0             # all zero: nine ones
    w[0, 3] = 65536
    w[0, 4, 2], w[0, 4, 7] = 200000, 0xFFFFFFFF
    w[1, 0] = 0
    w[1, 0, 0] = 65536      # one-hot on the first action
    w[1, 1] = 0
    w[1, 1, 8] = 1          # ... on the last
    w[1, 2, :8] = 0         # the same, from a random weight
    w[2, 3] = (0, 0, 1, 0, 0, 70000, 0, 0, 0)
    return w


@pytest.mark.parametrize("K", [1, 9, 10, 64, 70, 257])
def test_sample_equals_the_reference(K):
    M, H, seed = 3, 5, 0x1234567890ABCDEF
    w = _sample_weights()
    wd = _weights(w)
    keep = np.random.default_rng(2).integers(0, 9, (M, H)).astype(np.uint8)
    keep[0, 0], keep[2, 4] = 200, 9      # copied as stored
    kd = _dev(keep)
    active = np.array([1, 0, 1], np.uint8)
    ad = _dev(active)
    seen = set()
    for offset, const, with_keep, with_active in itertools.product((0, 1, 6, 7, (1 << 40) + 3), (1, 0), (True, False), (False, True)):
        table = torch.full((M, H, K), SENTINEL, dtype=torch.uint8, device="cuda")
        rc = _capi.lib.pc_cem_sample(0, wd.data_ptr(), M, H, K, seed, offset, const, kd.data_ptr() if with_keep else None,
                                     ad.data_ptr() if with_active else None, table.data_ptr(), _stream())
        assert rc == _capi.PC_OK
        want = X.sample(w, K, seed, offset, bool(const), keep if with_keep else None, active if with_active else None,
                        out=np.full((M, H, K), SENTINEL, np.uint8))
        _same(table.cpu().numpy(), want, (K, offset, const, with_keep, with_active))
        if with_active:
            assert (want[1] == SENTINEL).all()      # the inactive row keeps its sentinel
        seen.add(offset & 3)
    assert seen == {0, 1, 2, 3}
    _same(_back(wd), w, "weights read only")
    _same(kd.cpu().numpy(), keep, "keep read only")


def test_sample_two_workgroups_and_a_far_state():
    """More than one workgroup, no multiple of it; the element index runs on over the states"""
    M, H, K = 41, 7, 33
    w = np.random.default_rng(3).integers(0, 65537, (M, H, 9)).astype(np.uint32)
    w[np.random.default_rng(4).random((M, H, 9)) < 0.3] = 0
    table = torch.empty(M, H, K, dtype=torch.uint8, device="cuda")
    assert _capi.lib.pc_cem_sample(0, _weights(w).data_ptr(), M, H, K, 5, 9, 0, None, None, table.data_ptr(), _stream()) == _capi.PC_OK
    _same(table.cpu().numpy(), X.sample(w, K, 5, 9, False), "table")


# ---- 2. pc_cem_refit -------------------------------------------------------------------------------------------------------------------
def _returns(M, K, rng):
    """row 0: a few levels, ties everywhere (across the waves of a workgroup too), -0.0 beside 0.0; row 1: all equal; row 2: negative,
    all different; row 3: inactive; row 4: two levels; row 5: like 0 with other values"""
    ret = np.zeros((M, K))
    ret[0] = rng.integers(-2, 3, K) * 0.25
    ret[0][rng.random(K) < 0.5] *= -1.0      # -0.0 among the zeros
    ret[1] = -1.5
    ret[2] = -rng.random(K) - 0.5
    ret[3] = rng.random(K)
    ret[4] = rng.integers(0, 2, K) * 3.0
    ret[5] = rng.integers(-40, 40, K) * 0.125
    return ret


@pytest.mark.parametrize("K", [1, 64, 70, 300, 4096])
def test_refit_equals_the_reference(K):
    M = 6
    rng = np.random.default_rng(10 + K)
    ret = _returns(M, K, rng)
    if K >= 64:
        zeros = ret[0] == 0.0
        assert np.signbit(ret[0][zeros]).any() and not np.signbit(ret[0][zeros]).all()
    active = np.array([1, 1, 1, 0, 1, 1], np.uint8)
    rd, ad = _dev(ret), _dev(active)
    n = 0
    for H in (1, 12, 256):
        table = rng.integers(0, 9, (M, H, K)).astype(np.uint8)
        table[rng.random((M, H, K)) < 0.05] = 200      # entries above 8
        table[0, 0, 0] = 9
        td = _dev(table)
        w = rng.integers(0, 65537, (M, H, 9)).astype(np.uint32)
        w[0, 0] = 0                      # an all-zero row
        w[1, 0] = 0xFFFFFFFF             # above 65536
        for E, shift in itertools.product(sorted({1, min(7, K), K}), (0, 1, 3)):
            w_min, with_best = (0, 64)[n & 1], bool(n & 2) or n % 5 == 0
            n += 1
            wd = _weights(w)
            best = torch.full((M, H), SENTINEL, dtype=torch.uint8, device="cuda")
            rc = _capi.lib.pc_cem_refit(0, wd.data_ptr(), rd.data_ptr(), td.data_ptr(), M, H, K, E, shift, w_min, ad.data_ptr(),
                                        best.data_ptr() if with_best else None, _stream())
            assert rc == _capi.PC_OK
            want_w, want_b = X.refit(w, ret, table, E, shift, w_min, active, np.full((M, H), SENTINEL, np.uint8))
            what = (K, H, E, shift, w_min, with_best)
            _same(_back(wd), want_w, what)
            assert np.array_equal(want_w[3], w[3])      # the inactive row is untouched
            if with_best:
                _same(best.cpu().numpy(), want_b, what)
                assert (want_b[3] == SENTINEL).all()
            else:
                assert (best == SENTINEL).all()
        _same(td.cpu().numpy(), table, "table read only")
    _same(rd.cpu().numpy(), ret, "ret read only")
    _same(ad.cpu().numpy(), active, "active read only")
    # without `active`: every row
    wd = _weights(w)
    assert _capi.lib.pc_cem_refit(0, wd.data_ptr(), rd.data_ptr(), td.data_ptr(), M, H, K, min(7, K), 1, 64, None, None, _stream()) == _capi.PC_OK
    _same(_back(wd), X.refit(w, ret, table, min(7, K), 1, 64)[0], "all rows")


# ---- 3 / 4. the planner's loop on the driven rows ---------------------------------------------------------------------------------------
def _env(track, n, dtype, N=1):
    return pc.VecCarEnv(N, TRACKS[track], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype=dtype)


def _planner(env, **kw):
    return pc.CEMPlanner(env, horizon=X.H_REF, candidates=X.K_REF, elites=X.E_REF, iterations=X.ITERATIONS_REF, seed=X.SEED_REF, **kw)


def _states(s):
    t = {k: _dev(s[k], torch.float64) for k in F64_KEYS}
    t.update(turns=_dev(s["turns"], torch.int32), next_gate=_dev(s["next_gate"], torch.int32), time_step=_dev(s["time_step"], torch.int32))
    return t


def _check_plan(planner, ref, what):
    got = {k: v.cpu().numpy() for k, v in planner.out.items()}
    for k in ("ret",) + Q.BEST_KEYS:
        _same(got[k], ref[k], (what, k))
    _same(_back(planner.weights), ref["weights"], (what, "weights"))
    _same(planner.iter_best_ret.cpu().numpy(), ref["iter_best_ret"], (what, "iter_best_ret"))
    _same(planner.table.cpu().numpy(), ref["tables"], (what, "tables"))
    _same(planner.best_seq.cpu().numpy(), ref["best_seq"], (what, "best_seq"))


@pytest.mark.parametrize("track,n", X.CONFIGS)
def test_f64_plan_equals_the_reference_loop(track, n):
    s, ref = X.reference(track, n)
    M = len(s["px"])
    env = _env(track, n, "f64")
    planner = _planner(env)
    states = _states(s)
    keep = {k: v.clone() for k, v in states.items()}
    out = planner.plan(0, states=states)
    assert out is planner.out and out["best_action"].dtype == torch.int64 and out["best_action"].shape == (M,)
    _check_plan(planner, ref, "states")
    for k in states:
        assert torch.equal(states[k], keep[k]), k      # read only
    env.close()
    # the state form, on a handle put into those rows
    env = _env(track, n, "f64", M)
    env.reset()
    env.set_state(passed=0, **{k: s[k] for k in Q.STATE_KEYS})
    before = env.get_state()
    planner = _planner(env)
    act = planner.act(0)
    assert act.data_ptr() == planner.out["best_action"].data_ptr()
    _check_plan(planner, ref, "handle")
    after = env.get_state()
    for k in before:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k      # the env state is not touched
    env.close()


@pytest.mark.parametrize("track,n", X.CONFIGS)
def test_f32_plan_equals_the_loop_scored_by_its_own_k22(track, n):
    s = X.driven(track, n)
    M = len(s["px"])
    env = _env(track, n, "f32")
    states = _states(s)

    def score(tables):
        out = env.rollout_sequences(states["px"], states["py"], states["vx"], states["vy"], states["turns"], _dev(tables),
                                    next_gate=states["next_gate"], time_step=states["time_step"])
        return {k: v.cpu().numpy() for k, v in out.items()}

    ref = X.plan(X.uniform_weights(M, X.H_REF), score, X.K_REF, X.E_REF, X.ITERATIONS_REF, X.SEED_REF, 5 * X.ITERATIONS_REF)
    planner = _planner(env)
    planner.plan(5, states=states)      # step_index 5: offsets 20 .. 23
    _check_plan(planner, ref, "f32")
    assert (np.diff(ref["iter_best_ret"], axis=0) >= 0).all()
    env.close()


# ---- 5. the planner's behaviour --------------------------------------------------------------------------------------------------------
def test_warm_start_and_done_restart_on_a_drive():
    track, n, N, steps = "big_track", 16, 8, 40
    H, K, E, iters, seed = 8, 32, 4, 3, 11
    s = X.driven(track, n)
    s0 = {k: np.asarray(s[k][40:40 + N]).copy() for k in Q.STATE_KEYS}
    s0["time_step"][::2] = 985      # every other env meets the time limit on the way: an auto-reset
    env = _env(track, n, "f64", N)
    env.reset()
    env.set_state(passed=0, **s0)
    orc = oracle.OracleVecEnv(R.track(track), N, n, reward_scaling=R.REWARD_SCALE)
    orc.reset()
    orc.set_state(passed=0, destroyed=0, **s0)
    planner = pc.CEMPlanner(env, horizon=H, candidates=K, elites=E, iterations=iters, seed=seed)
    w = X.uniform_weights(N, H)
    done_ref = done = None
    resets, rows, warm = 0, [], False
    for step in range(steps):
        w = np.roll(w, -1, axis=1)
        w[:, -1] = X.INIT_WEIGHT
        if done_ref is not None:
            w[done_ref] = X.INIT_WEIGHT
        carried = w.copy()
        ref = X.plan(w, X.oracle_scorer(track, n, {k: getattr(orc, k).copy() for k in Q.STATE_KEYS}), K, E, iters, seed, step * iters)
        w = ref["weights"]
        act = planner.act(step, done=done)
        _check_plan(planner, ref, step)
        if step > 0 and not done_ref.all():      # the warm start matters: a plan from fresh weights is another plan
            warm |= bool((carried[~done_ref] != X.INIT_WEIGHT).any())
        _, r, term, trunc, _ = env.step(act)
        _, _, oterm, otrunc = orc.step(ref["best_action"])
        done, done_ref = term + trunc, oterm | otrunc
        assert np.array_equal(done.cpu().numpy() != 0, done_ref), step
        resets += int(done_ref.sum())
        rows.append(r.clone())
    assert resets >= N // 2 and warm
    # drive() feeds the flags itself: the same rewards from the same start
    env.set_state(passed=0, **s0)
    planner.reset_plan()
    rew, _, _ = planner.drive(steps)
    assert torch.equal(rew, torch.stack(rows))
    # without warm start every plan starts from the initial weights
    env.set_state(passed=0, **s0)
    orc.set_state(passed=0, destroyed=0, **s0)
    cold = pc.CEMPlanner(env, horizon=H, candidates=K, elites=E, iterations=iters, seed=seed, warm_start=False)
    for step in range(2):
        ref = X.plan(X.uniform_weights(N, H), X.oracle_scorer(track, n, {k: getattr(orc, k).copy() for k in Q.STATE_KEYS}), K, E, iters, seed,
                     step * iters)
        env.step(cold.act(step))
        _check_plan(cold, ref, ("cold", step))
        orc.step(ref["best_action"])
    env.close()


def test_cem_evaluation_is_reproducible_and_shooting_is_what_it_was():
    N = 64
    ev = pc.PlannerEvaluator(TRACKS["big_track"], n_envs=N, num_rays=16, reward_scaling=0.1, horizon=8, candidates=16, seed=2, kind="cem",
                             elites=4, iterations=2)
    assert isinstance(ev.planner, pc.CEMPlanner) and ev.kind == "cem"
    a = ev.evaluate()
    state, tot = ev.state.cpu().numpy().copy(), ev.totals().cpu().numpy()
    assert set(a) == set(EVAL_KEYS) and a["eval/episodes"] == N and (state[4] != 0).all()
    want = first_episodes_ref(ev.rew.cpu().numpy(), ev.term.cpu().numpy(), ev.trunc.cpu().numpy(), 0.1)
    assert np.array_equal(_bits(state), _bits(want))
    b = ev.evaluate()      # the plan is reset at the start of run()
    assert a == b and np.array_equal(_bits(ev.state.cpu().numpy()), _bits(state)) and np.array_equal(_bits(ev.totals().cpu().numpy()), _bits(tot))
    ev.close()
    # kind="shooting", and the default: a Planner driven by hand over the same 1000 steps
    kw = dict(n_envs=N, num_rays=16, reward_scaling=0.1, horizon=PLAN_H, candidates=PLAN_K, seed=PLAN_SEED)
    env = pc.VecCarEnv(N, TRACKS["big_track"], num_rays=16, reward_scaling=0.1)
    env.reset()
    rew, term, trunc = pc.Planner(env, PLAN_H, PLAN_K, PLAN_SEED).drive(_capi.PC_TIME_LIMIT)
    want = first_episodes_ref(rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), 0.1)
    env.close()
    for more in (dict(), dict(kind="shooting")):
        ev = pc.PlannerEvaluator(TRACKS["big_track"], **kw, **more)
        assert type(ev.planner) is pc.Planner and ev.kind == "shooting"
        ev.run()
        assert np.array_equal(_bits(ev.state.cpu().numpy()), _bits(want)), more
        assert torch.equal(ev.rew, rew) and torch.equal(ev.term, term) and torch.equal(ev.trunc, trunc)
        ev.close()


def test_evaluate_cem_prints_the_planner_it_ran(capsys):
    import evaluate
    out = evaluate.main(["--planner", "cem", "--plan-iterations", "2", "--plan-elites", "4", "--plan-horizon", "6", "--plan-candidates", "16",
                         "--envs", "16", "--track", TRACKS["big_track"], "--num-rays", "16"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    assert {k for k in out if k.startswith("eval/")} == set(EVAL_KEYS)
    assert out["eval/episodes"] == 16 and out["path"] == "planner"
    assert out["planner"] == {"kind": "cem", "horizon": 6, "candidates": 16, "iterations": 2, "elites": 4}
