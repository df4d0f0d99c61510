"""Batched evaluation on the GPU: K14 (pc_first_episodes) bit for bit against the numpy reference of first_episode_reference.py and
against pc_episode_stats, K15 (pc_greedy) against torch.argmax / log_softmax, the Evaluator on the trained policy fixture against a
loop written here, the Trainer with and without evaluations (training must not move by a bit), resume, and evaluate.py --envs."""
import math

import numpy as np
import pytest
import torch

import ppo_car_amd as pc
from ppo_car_amd import _capi
from ppo_car_amd.evaluation import EVAL_KEYS, Evaluator
from ppo_car_amd.ppo import PPOConfig, Trainer
from conftest import TRACKS
from first_episode_reference import RUNNING, first_episodes_ref, new_state
from test_episode_stats_host import ALPHABET, init_out

pytestmark = pytest.mark.gpu

BUFFER, STEPS = _capi.PC_EPISODE_BUFFER, _capi.PC_EPISODE_STEPS


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _eq(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (what, np.argwhere(_bits(a) != _bits(b))[:5])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _synthetic(T, N, s, seed):
    """Step-layout rows: rewards from the reference's alphabet x scale, done probability 0.05 (a few with both flags), and two forced
    envs: env 0 closes at step 0, env N - 1 at the last step and nowhere else."""
    rng = np.random.default_rng(seed)
    rew = (ALPHABET[rng.integers(0, len(ALPHABET), size=(T, N))] * s).astype(np.float32)
    done = rng.random((T, N)) < 0.05
    kind = rng.integers(0, 5, size=(T, N))              # 0, 1: terminated; 2, 3: truncated; 4: both
    term = (done & ((kind < 2) | (kind == 4))).astype(np.float32)
    trunc = (done & (kind >= 2)).astype(np.float32)
    term[0, 0] = 1.0
    if N > 1:
        term[:, N - 1] = 0.0
        trunc[:, N - 1] = 0.0
        trunc[T - 1, N - 1] = 1.0
    return rew, term, trunc


def _scan(rew, term, trunc, layout, s, state):
    """One pc_first_episodes call on step-layout numpy rows, handed over in `layout` (the Buffer layout gets a row 0 of ones: the
    flags of the step before the window, which the kernel must not read as this window's)."""
    T, N = rew.shape
    if layout == BUFFER:
        lt, ltr = _dev(term[T - 1]), _dev(trunc[T - 1])
        term = np.concatenate([np.ones((1, N), np.float32), term[:T - 1]], axis=0)
        trunc = np.concatenate([np.ones((1, N), np.float32), trunc[:T - 1]], axis=0)
    R, TE, TR = _dev(rew), _dev(term), _dev(trunc)
    _capi.check(_capi.lib.pc_first_episodes(0, R.data_ptr(), TE.data_ptr(), TR.data_ptr(), lt.data_ptr() if layout == BUFFER else None,
                                            ltr.data_ptr() if layout == BUFFER else None, T, N, layout, s, state.data_ptr(), _stream()),
                "pc_first_episodes")
    torch.cuda.synchronize()


# ---- K14 against the numpy reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0.1, 0.37])
@pytest.mark.parametrize("layout", [BUFFER, STEPS])
@pytest.mark.parametrize("T", [1, 7, 8, 9, 33])
@pytest.mark.parametrize("N", [1, 65, 300])
def test_scan_bitwise(N, T, layout, s):
    rew, term, trunc = _synthetic(T, N, s, seed=T * 1009 + N)
    ref = first_episodes_ref(rew, term, trunc, s)
    assert ref[4, 0] != RUNNING and ref[1, 0] == 1
    if N > 1:
        assert ref[1, N - 1] == T and ref[4, N - 1] == 2
    if N == 300 and T == 33:
        assert (ref[4] == RUNNING).any() and (ref[3] > 1).any()       # some envs never close; some lap more than once
    state = _dev(new_state(N))
    _scan(rew, term, trunc, layout, s, state)
    _eq(state.cpu().numpy(), ref, "state")


@pytest.mark.parametrize("layout", [BUFFER, STEPS])
@pytest.mark.parametrize("N", [65, 300])
def test_windows_chain_and_closed_envs_stay(N, layout):
    T, s = 33, 0.1
    rew, term, trunc = _synthetic(T, N, s, seed=77 + N)
    one = _dev(new_state(N))
    _scan(rew, term, trunc, layout, s, one)
    cut = _dev(new_state(N))
    a = 0
    for w in (1, 7, 8, 17):
        _scan(rew[a:a + w], term[a:a + w], trunc[a:a + w], layout, s, cut)
        a += w
    assert a == T
    _eq(cut.cpu().numpy(), one.cpu().numpy(), "1 + 7 + 8 + 17 vs 33")
    _eq(one.cpu().numpy(), first_episodes_ref(rew, term, trunc, s), "33 vs numpy")
    # every env closed: a further window changes nothing
    end = np.ones((1, N), np.float32)
    _scan(rew[:1], end, end, layout, s, one)
    closed = one.cpu().numpy().copy()
    assert (closed[4] != RUNNING).all()
    rew2, term2, trunc2 = _synthetic(9, N, s, seed=5)
    _scan(rew2, term2, trunc2, layout, s, one)
    _eq(one.cpu().numpy(), closed, "closed state")


def test_scan_agrees_with_episode_stats():
    """Step-layout rows in which every env has exactly one done, in the last row, from a zero carry: pc_episode_stats' sums of the one
    finished episode (return, length, gates, laps) are the first-episode state's rows 0-3."""
    T, N, s = 40, 300, 0.1
    rng = np.random.default_rng(11)
    rew = (ALPHABET[rng.integers(0, len(ALPHABET), size=(T, N))] * s).astype(np.float32)
    term = np.zeros((T, N), np.float32)
    trunc = np.zeros((T, N), np.float32)
    term[T - 1, ::2] = 1.0
    trunc[T - 1, 1::2] = 1.0
    R, TE, TR = _dev(rew), _dev(term), _dev(trunc)
    carry, out = torch.zeros(4, N, dtype=torch.float64, device="cuda"), _dev(init_out(N))
    _capi.check(_capi.lib.pc_episode_stats(0, R.data_ptr(), TE.data_ptr(), TR.data_ptr(), None, None, T, N, STEPS, s, carry.data_ptr(),
                                           out.data_ptr(), _stream()), "pc_episode_stats")
    state = _dev(new_state(N))
    _scan(rew, term, trunc, STEPS, s, state)
    out, state = out.cpu().numpy(), state.cpu().numpy()
    assert (out[0] == 1).all()
    _eq(out[1:5], state[0:4], "episode_stats out[1..4] vs state rows 0-3")
    assert np.array_equal(state[4, ::2], np.ones(N // 2)) and np.array_equal(state[4, 1::2], np.full(N // 2, 2.0))


# ---- K15 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 2, 9, 16])
@pytest.mark.parametrize("N", [1, 63, 1025])
def test_greedy(N, A):
    g = torch.Generator(device="cuda").manual_seed(N * 31 + A)
    logits = torch.randn(N, A, device="cuda", generator=g) * 1.5
    if N > 2 and A > 1:
        logits[1, A - 1] = logits[1].max()                  # a duplicated maximum: the first index wins
        logits[1, 0] = logits[1, A - 1]
        logits[2] = 0.25                                    # an all-equal row
    act = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    af = torch.full((N,), -1.0, device="cuda")
    lp = torch.full((N,), 9.0, device="cuda")
    _capi.check(_capi.lib.pc_greedy(0, logits.data_ptr(), N, A, act.data_ptr(), af.data_ptr(), lp.data_ptr(), _stream()), "pc_greedy")
    want = torch.argmax(logits, dim=1)
    assert torch.equal(act, want)
    if N > 2 and A > 1:
        assert int(act[1]) == 0 and int(act[2]) == 0
    assert torch.equal(af, act.float())
    ref = torch.log_softmax(logits.double(), dim=1).gather(1, want[:, None])[:, 0]
    err = float((lp.double() - ref).abs().max())
    print(f"pc_greedy N={N} A={A}: max |logprob - log_softmax| = {err:.3e}")
    assert err <= 2e-6
    act2 = torch.full((N,), -1, dtype=torch.int64, device="cuda")       # the optional outputs left out
    _capi.check(_capi.lib.pc_greedy(0, logits.data_ptr(), N, A, act2.data_ptr(), None, None, _stream()), "pc_greedy")
    assert torch.equal(act2, want)


# ---- the Evaluator on the trained policy ------------------------------------------------------------------------------------------
N_EV, SEED = 64, 1234


def _trained_agent():
    from oracle.scenarios import load_trained_policy
    agent = pc.Agent(23, 9).cuda()
    load_trained_policy(agent)
    return agent


def _evaluator(agent, **kw):
    return Evaluator(agent, TRACKS["big_track"], n_envs=N_EV, num_rays=16, reward_scaling=0.1, device="cuda", seed=SEED, **kw)


def _run(ev, index):
    ev.run(index=index)
    torch.cuda.synchronize()
    return ev.state.cpu().numpy().copy()


def _loop(agent, index, greedy, dtype="f32"):
    """1000 x (pc_policy_act at (SEED, index * 1000 + t); VecCarEnv.step) from reset, the rows accumulated by the numpy reference."""
    env = pc.VecCarEnv(N_EV, TRACKS["big_track"], num_rays=16, reward_scaling=0.1, device="cuda", dtype=dtype)
    agent.rng_seed = SEED
    obs, _ = env.reset()
    rew, term, trunc = (torch.empty(1000, N_EV, device="cuda") for _ in range(3))
    logits = torch.empty(N_EV, 9, device="cuda")
    with torch.no_grad():
        for t in range(1000):
            a, _, _ = agent.act(obs, out_logits=logits, offset=index * 1000 + t, repack=t == 0)
            if greedy:
                a = torch.argmax(logits, dim=1)
            env.step(a, out=(obs, rew[t], term[t], trunc[t]))
    torch.cuda.synchronize()
    env.close()
    return first_episodes_ref(rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), 0.1)


@pytest.fixture(scope="module")
def trained():
    """The states every test below reads, computed once: mega and steps at index 3 (both dtypes), index 3 again, index 4, greedy."""
    agent = _trained_agent()
    out = {}
    for dtype in ("f32", "f64"):
        mega, steps = _evaluator(agent, dtype=dtype), _evaluator(agent, dtype=dtype, rollout_kernel="steps")
        out[dtype, "mega"], out[dtype, "steps"] = _run(mega, 3), _run(steps, 3)
        out[dtype, "paths"] = (mega.last_path, steps.last_path)
        if dtype == "f32":
            out["again"], out["index4"] = _run(mega, 3), _run(mega, 4)
            out["scalars"] = mega.scalars(mega.totals().tolist())
        mega.close(); steps.close()
    out["loop"] = _loop(agent, 3, greedy=False)
    return out


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_evaluator_mega_and_steps_leave_the_same_state(trained, dtype):
    assert trained[dtype, "paths"] == ("mega", "steps")
    _eq(trained[dtype, "mega"], trained[dtype, "steps"], "mega vs steps")


def test_evaluator_equals_a_loop_written_here(trained):
    _eq(trained["f32", "steps"], trained["loop"], "steps vs loop")
    _eq(trained["f32", "mega"], trained["loop"], "mega vs loop")


def test_evaluator_closes_every_episode_and_times_laps(trained):
    s = trained["f32", "mega"]
    assert (s[4] != RUNNING).all() and ((s[4] == 1) | (s[4] == 2)).all()
    assert (s[1] >= 1).all() and (s[1] <= 1000).all() and (s[1][s[4] == 2] == 1000).all()
    lapped = s[3] > 0
    assert lapped.any(), "the trained policy fixture laps (~3 laps per episode)"
    assert np.isfinite(s[6][lapped]).all() and np.isfinite(s[7][lapped]).all() and (s[6][lapped] <= s[7][lapped]).all()
    assert (s[5][lapped] <= s[1][lapped]).all() and (s[6][lapped] * s[3][lapped] <= s[5][lapped]).all()
    assert np.isinf(s[6][~lapped]).all() and np.isinf(s[7][~lapped]).all() and (s[5][~lapped] == 0).all()
    d = trained["scalars"]          # of the run at index 4
    assert set(d) == set(EVAL_KEYS) and d["eval/episodes"] == N_EV and 0.0 <= d["eval/crash_rate"] <= 1.0
    assert d["eval/episodic_return_min"] <= d["eval/episodic_return"] <= d["eval/episodic_return_max"]


def test_evaluator_index_is_the_stream_position(trained):
    _eq(trained["again"], trained["f32", "mega"], "index 3 twice")
    assert not np.array_equal(_bits(trained["index4"]), _bits(trained["f32", "mega"]))


def test_evaluator_greedy():
    agent = _trained_agent()
    a, b = _evaluator(agent, greedy=True), Evaluator(agent, TRACKS["big_track"], n_envs=N_EV, num_rays=16, reward_scaling=0.1,
                                                     device="cuda", seed=SEED + 1, greedy=True)
    sa, sb = _run(a, 0), _run(b, 5)
    assert a.last_path == "steps" and b.last_path == "steps"
    a.close(); b.close()
    _eq(sa, sb, "greedy: the seed and the index do not matter")
    _eq(sa, _loop(agent, 0, greedy=True), "greedy vs loop")
    assert (sa[4] != RUNNING).all()


def test_evaluator_leaves_the_agent_alone_and_runs_a_fresh_policy():
    torch.manual_seed(3)
    agent = pc.Agent(23, 9).cuda()
    agent.rng_seed = 99
    before = (agent._rng_offset, agent.__dict__.get("_image"), agent.__dict__.get("_range_event"), torch.cuda.get_rng_state().clone(),
              torch.get_rng_state().clone())
    ev = _evaluator(agent)
    d = ev.evaluate()
    ev.close()
    assert 0.0 <= d["eval/crash_rate"] <= 1.0 and d["eval/episodes"] == N_EV and 1 <= d["eval/episodic_length"] <= 1000
    assert agent._rng_offset == before[0] and agent.__dict__.get("_image") is before[1] and agent.__dict__.get("_range_event") is before[2]
    assert torch.equal(torch.cuda.get_rng_state(), before[3]) and torch.equal(torch.get_rng_state(), before[4])


def test_evaluator_with_an_agent_outside_the_fused_menu():
    """A 128-wide agent has no pc_policy handle: agent.actor(obs) + pc_sample / pc_greedy on the per-step path."""
    torch.manual_seed(4)
    agent = pc.Agent(23, 9, hidden_size=128).cuda()
    assert agent.policy_form() is None
    ev = _evaluator(agent)
    s0, s1, s2 = _run(ev, 2), _run(ev, 2), _run(ev, 3)
    assert ev.last_path == "steps" and (s0[4] != RUNNING).all()
    _eq(s0, s1, "index 2 twice")
    assert not np.array_equal(_bits(s0), _bits(s2))
    ev.close()
    # greedy: the state of a loop of agent.actor, torch.argmax and VecCarEnv.step
    ev = _evaluator(agent, greedy=True)
    sg = _run(ev, 0)
    ev.close()
    env = pc.VecCarEnv(N_EV, TRACKS["big_track"], num_rays=16, reward_scaling=0.1, device="cuda")
    obs, _ = env.reset()
    rew, term, trunc = (torch.empty(1000, N_EV, device="cuda") for _ in range(3))
    with torch.no_grad():
        for t in range(1000):
            env.step(torch.argmax(agent.actor(obs), dim=1), out=(obs, rew[t], term[t], trunc[t]))
    torch.cuda.synchronize()
    env.close()
    _eq(sg, first_episodes_ref(rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), 0.1), "greedy vs loop")


# ---- training is not perturbed -----------------------------------------------------------------------------------------------------
WALL = ("elapsed", "charts/SPS")


def _cfg(**kw):
    base = dict(n_envs=64, n_steps=32, batch_size=32, train_iters=2, track=TRACKS["big_track"], num_rays=16, seed=5)
    base.update(kw)
    return PPOConfig(**base)


def _train(epochs, sync=True, **kw):
    tr = Trainer(_cfg(**kw), device="cuda")
    rows = [tr.run_epoch(sync=sync) for _ in range(epochs)]
    if sync == "lazy":
        rows.append(tr.flush_scalars())
    torch.cuda.synchronize()
    end = (tr.learner.flat_param.clone(), tr.next_obs.clone(), tr.rng_base.clone(), tr.agent._rng_offset, tr.rollout_mode,
           None if tr.evaluator is None else tr.evaluator.last_path)
    tr.close()
    return rows, end


def _train_rows(r):
    return [{k: v for k, v in row.items() if not k.startswith("eval/") and k not in WALL} for row in r]


@pytest.fixture(scope="module")
def evaluated_run():
    return _train(3, rollout_kernel="mega", eval_every=1, eval_envs=64)


@pytest.mark.parametrize("mode", ["mega", "steps"])
def test_training_is_bitwise_untouched(mode, evaluated_run):
    kw = dict(rollout_kernel="mega") if mode == "mega" else dict(rollout_kernel="steps", use_graphs=False)
    plain, end0 = _train(3, **kw)
    evald, end1 = evaluated_run if mode == "mega" else _train(3, eval_every=1, eval_envs=64, **kw)
    assert end0[4] == end1[4] == ("mega" if mode == "mega" else "steps-eager") and end0[5] is None and end1[5] == mode
    assert torch.equal(end0[0], end1[0]) and torch.equal(end0[1], end1[1]) and torch.equal(end0[2], end1[2]) and end0[3] == end1[3]
    assert _train_rows(plain) == _train_rows(evald)
    for a, b in zip(plain, evald):
        assert not any(k.startswith("eval/") for k in a)
        assert set(EVAL_KEYS) <= set(b) and b["eval/episodes"] == 64 and b["eval/episodic_return"] is not None


def test_eval_every_2_and_lazy_and_resume(evaluated_run, tmp_path):
    every1 = evaluated_run[0]
    ev = lambda row: {k: v for k, v in row.items() if k.startswith("eval/")}
    # eval_every = 2: epoch 2 carries the keys -- the values of the every-epoch run's epoch 2 (the index is the epoch) --, 1 and 3 none
    rows, _ = _train(3, rollout_kernel="mega", eval_every=2, eval_envs=64)
    assert ev(rows[0]) == {} and ev(rows[2]) == {} and ev(rows[1]) == ev(every1[1]) and set(ev(rows[1])) == set(EVAL_KEYS)
    # sync = "lazy": the same values, one call later
    lazy, _ = _train(3, sync="lazy", rollout_kernel="mega", eval_every=1, eval_envs=64)
    assert lazy[0] is None and [ev(r) for r in lazy[1:]] == [ev(r) for r in every1]
    # resume after epoch 1: epoch 2 evaluates as in the uninterrupted run, and nothing of the evaluator is in the checkpoint
    a = Trainer(_cfg(rollout_kernel="mega", eval_every=1, eval_envs=64), device="cuda")
    a.run_epoch()
    sd = a.state_dict()
    assert not any("eval" in k for k in sd)
    torch.save(sd, tmp_path / "t.pt")
    a.close()
    b = Trainer(_cfg(rollout_kernel="mega", eval_every=1, eval_envs=64), device="cuda")
    b.load_state_dict(torch.load(tmp_path / "t.pt", map_location="cuda", weights_only=False))
    row = b.run_epoch()
    b.close()
    assert ev(row) == ev(every1[1]) and set(ev(row)) == set(EVAL_KEYS)


# ---- evaluate.py --envs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("greedy", [False, True])
def test_evaluate_envs(tmp_path, greedy, capsys):
    import json

    import evaluate
    torch.manual_seed(0)
    torch.save(pc.Agent(18, 9).state_dict(), tmp_path / "model.dat")
    out = evaluate.main(["--checkpoint", str(tmp_path / "model.dat"), "--track", TRACKS["big_track"], "--envs", "32"]
                        + (["--greedy"] if greedy else []))
    assert set(EVAL_KEYS) <= set(out) and out["eval/episodes"] == 32 and out["path"] in (("steps",) if greedy else ("mega", "steps"))
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    assert 1 <= out["eval/episodic_length"] <= 1000 and 0.0 <= out["eval/crash_rate"] <= 1.0 and not math.isnan(out["eval/episodic_return"])
