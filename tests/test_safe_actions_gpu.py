"""K21 (pc_env_safe_actions / pc_env_safe_actions_state; VecCarEnv.safe_actions / action_masks), PolicyLandscape.viability() and the
shielded Evaluator on the GPU.

Everything is an equality of 0 / 1 bytes.  F64 handles against the enumeration on the CPU oracle (safe_actions_reference.masks), F32
handles against the same enumeration by chained pc_env_step_poses calls on the same handle: every row replicated 9^d times, one copy
per action sequence, stepped d times with the copies that terminated or truncated frozen (inactive), folded back over the sequences
that share a first action."""
import numpy as np
import pytest
import torch

import ppo_car_amd as pc
from ppo_car_amd.evaluation import EVAL_KEYS, SHIELD_KEYS, Evaluator
from conftest import TRACKS
from first_episode_reference import first_episodes_ref
from oracle.scenarios import load_trained_policy
import step_poses_reference as R
import safe_actions_reference as S
import ray_counts_reference as rc

pytestmark = pytest.mark.gpu

F64_KEYS = ("px", "py", "vx", "vy")
SENTINEL = 7
RECIPES = ("edge", "near_gate", "pre_crash")


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _tensors(s):
    t = {k: _dev(s[k], torch.float64) for k in F64_KEYS}
    t["turns"] = _dev(s["turns"], torch.int32)
    t["time_step"] = _dev(s["time_step"], torch.int32)
    return t


def _masks(env, s, depth, track_id=None, active=None, time_step=True):
    """One safe_actions call on device copies of the numpy rows s, the output pre-filled with a sentinel: uint8 [M, 9] numpy.  The inputs
    must come back as they went in."""
    t = _tensors(s)
    keep = {k: v.clone() for k, v in t.items()}
    M = len(s["px"])
    out = torch.full((M, 9), SENTINEL, dtype=torch.uint8, device="cuda")
    got = env.safe_actions(t["px"], t["py"], t["vx"], t["vy"], t["turns"], depth=depth, time_step=t["time_step"] if time_step else None,
                           track_id=None if track_id is None else _dev(track_id, torch.uint8),
                           active=None if active is None else _dev(active, torch.uint8), out=out)
    assert got.dtype == torch.bool and got.shape == (M, 9) and got.data_ptr() == out.data_ptr()
    for k in t:
        assert torch.equal(t[k], keep[k]), k      # read only
    return out.cpu().numpy()


def _chained(env, s, depth, track_id=None):
    """The enumeration by chained pc_env_step_poses calls on `env`: [depth][M, 9] bool, entry d - 1 the mask at depth d."""
    M = len(s["px"])
    seq = S.sequences(depth)
    K = len(seq)
    rep = lambda a, dt: _dev(np.repeat(np.asarray(a), K), dt)
    px, py, vx, vy = (rep(s[k], torch.float64) for k in F64_KEYS)
    turns, ts, ng = rep(s["turns"], torch.int32), rep(s["time_step"], torch.int32), torch.zeros(M * K, dtype=torch.int32, device="cuda")
    tid = None if track_id is None else rep(track_id, torch.uint8)
    dead = torch.zeros(M * K, dtype=torch.bool, device="cuda")
    frozen = torch.zeros(M * K, dtype=torch.bool, device="cuda")
    out = []
    for j in range(depth):
        acts = _dev(np.tile(seq[:, j], M), torch.int64)
        r = env.step_poses(px, py, vx, vy, turns, acts, next_gate=ng, time_step=ts, track_id=tid, active=(~frozen).to(torch.uint8))
        term, trunc = (r.terminated != 0) & ~frozen, (r.truncated != 0) & ~frozen      # (a frozen row's flags are stale)
        dead |= term
        frozen |= term | trunc
        out.append((~dead).reshape(M, 9, K // 9).any(2).cpu().numpy())
    return out


def _env(track, n, dtype, N=1):
    return pc.VecCarEnv(N, TRACKS[track], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype=dtype)


def _exact(got, want, what):
    assert set(np.unique(got)) <= {0, 1}, what
    assert np.array_equal(got != 0, want), (what, np.argwhere((got != 0) != want)[:8])


# ---- 1. F64 handles: the enumeration on the CPU oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("track,n", S.CONFIGS)
def test_f64_equals_the_reference(track, n, recipe):
    s, ref = S.reference(track, n, recipe, 3)
    env = _env(track, n, "f64")
    for d in (1, 2, 3):
        _exact(_masks(env, s, d), ref[d - 1], (recipe, d))
    if recipe == "pre_crash":
        assert [S.classes(m) for m in ref] == S.PRE_CRASH_COUNTS[(track, n)][1]      # empty, mixed and full masks at every depth
    env.close()


# ---- 2. F32 handles: the enumeration by chained K20 calls on the same handle ---------------------------------------------------------
@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("track,n", S.CONFIGS)
def test_f32_equals_chained_step_poses(track, n, recipe):
    s = S.RECIPES[recipe](track, n)
    env = _env(track, n, "f32")
    want = _chained(env, s, 3)
    for d in (1, 2, 3):
        _exact(_masks(env, s, d), want[d - 1], (recipe, d))
    if recipe == "pre_crash":      # the F32 rows are as mixed as the oracle's (a 10 px threshold can fall differently in a row or two)
        M = len(s["px"])
        for m in want:
            assert all(c >= need * M for c, need in zip(S.classes(m), S.SHARES)), S.classes(m)
    env.close()


# ---- 2b. the off-menu ray counts (tests/ray_counts_reference.py): 7 collision rays of 8 rays; collision rays past the 64-bit mask ------------
OFF_MENU = [(rc.TRACK_OF[n], n) for n in (7, 181)]


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("track,n", OFF_MENU)
def test_off_menu_ray_counts_f64_equals_the_reference(track, n, recipe):
    s, ref = S.reference(track, n, recipe, 2)
    env = _env(track, n, "f64")
    for d in (1, 2):
        _exact(_masks(env, s, d), ref[d - 1], (recipe, d))
    if recipe == "pre_crash":      # empty, mixed and full masks at both depths
        for m in ref[:2]:
            assert all(c >= need * len(s["px"]) for c, need in zip(S.classes(m), S.SHARES)), S.classes(m)
    env.close()


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("track,n", OFF_MENU)
def test_off_menu_ray_counts_f32_equals_chained_step_poses(track, n, recipe):
    s = S.RECIPES[recipe](track, n)
    env = _env(track, n, "f32")
    want = _chained(env, s, 2)
    for d in (1, 2):
        _exact(_masks(env, s, d), want[d - 1], (recipe, d))
    if recipe == "pre_crash":
        for m in want:
            assert all(c >= need * len(s["px"]) for c, need in zip(S.classes(m), S.SHARES)), S.classes(m)
    env.close()


# ---- 3. depth 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("track,n", S.CONFIGS)
def test_depth_4(track, n, dtype):
    env = _env(track, n, dtype)
    for recipe in RECIPES:
        s = S.RECIPES[recipe](track, n)
        m3, m4 = _masks(env, s, 3), _masks(env, s, 4)
        assert set(np.unique(m4)) <= {0, 1} and not ((m4 != 0) & (m3 == 0)).any(), recipe      # mask(4) is a subset of mask(3)
    s = {k: v[:64] for k, v in S.pre_crash_states(track, n).items()}
    want = S.masks(track, n, s, 4)[3] if dtype == "f64" else _chained(env, s, 4)[3]      # 64 x 6561 copies
    got = _masks(env, s, 4)
    _exact(got, want, "depth 4")
    assert (got.sum(1) == 0).any() and (got.sum(1) == 9).any() and (got != _masks(env, s, 3)).any()
    env.close()


# ---- 4. the state form -----------------------------------------------------------------------------------------------------------
def _state_rows(env, track):
    st = env.get_state()
    s = {k: st[k] for k in F64_KEYS}
    s.update(rot=st["rot"], turns=R.turns_of(st["rot"], R.track(track).start_rot), time_step=st["time_step"])
    return st, s


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("track,n", [("big_track", 16), ("track", 12)])
def test_state_form_equals_poses_form_of_get_state(track, n, dtype):
    rows = [S.RECIPES[r](track, n) for r in RECIPES]
    s0 = {k: np.concatenate([r[k] for r in rows]) for k in S.STATE_KEYS}
    N = len(s0["px"])
    env = _env(track, n, dtype, N)
    env.reset()
    env.set_state(passed=0, **s0)
    rng = np.random.default_rng(23)
    actions = rng.integers(0, 9, size=(40, N))
    actions[rng.random((40, N)) < 0.4] = 0
    for phase in ("set_state", "stepped"):
        if phase == "stepped":
            done = 0
            for t in range(40):
                _, _, te, tr, _ = env.step(torch.from_numpy(actions[t]).cuda())
                done += int(((te + tr) > 0).sum())
            assert done > 0      # auto-resets included
        before, s = _state_rows(env, track)
        # the rotation a turn count names is the one-way sum: an F64 env that turned both ways can sit a few ulps off it, and the state form
        # reads the env's own rotation -- those rows are held to the oracle from that very rotation instead (every F64 row is, below)
        on_row = np.array([S.rot_after(R.track(track).start_rot, int(k)) == r for k, r in zip(s["turns"], s["rot"])]) if dtype == "f64" \
            else np.ones(N, bool)
        assert on_row.sum() > N // 2
        for d in (1, 2, 3):
            out = torch.full((N, 9), SENTINEL, dtype=torch.uint8, device="cuda")
            got = env.action_masks(d, out=out)
            assert got.dtype == torch.bool and got.shape == (N, 9) and got.data_ptr() == out.data_ptr()
            got = out.cpu().numpy()
            assert set(np.unique(got)) <= {0, 1}
            assert np.array_equal(got[on_row], _masks(env, s, d)[on_row]), (phase, d)
        if dtype == "f64":
            want = S.masks(track, n, s, 3)
            for d in (1, 2, 3):
                _exact(env.action_masks(d).to(torch.uint8).cpu().numpy(), want[d - 1], (phase, d))
        after = env.get_state()
        for k in before:
            assert np.array_equal(_bits(before[k]), _bits(after[k])), (phase, k)      # the env state is not touched
    env.close()


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------
def _mixed_rows(track, n, M=257):
    rows = [S.RECIPES[r](track, n) for r in RECIPES]
    s = {k: np.concatenate([r[k] for r in rows]) for k in F64_KEYS + ("turns", "time_step")}
    perm = np.random.default_rng(3).permutation(len(s["px"]))[:M]
    return {k: v[perm] for k, v in s.items()}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_edges_one_row_odd_count_inactive_repeat_time_limit(dtype):
    track, n = "big_track", 16
    env = _env(track, n, dtype, 3)
    env.reset()
    before = env.get_state()
    s = _mixed_rows(track, n)
    M = len(s["px"])
    assert M == 257      # not a multiple of the 64 / 9 rows of a wave, nor of the 256 / 9 of a workgroup
    for d in (1, 2, 3, 4):
        full = _masks(env, s, d)
        assert set(np.unique(full)) <= {0, 1} and 0 < full.sum() < full.size
        assert np.array_equal(_masks(env, s, d), full)      # a repeat call gives the same bytes
        for m in (0, 5, 256):      # M = 1
            assert np.array_equal(_masks(env, {k: v[m:m + 1] for k, v in s.items()}, d), full[m:m + 1]), (d, m)
        active = (np.arange(M) % 3 != 1).astype(np.uint8)
        part = _masks(env, s, d, active=active)
        assert np.array_equal(part[active != 0], full[active != 0]) and (part[active == 0] == SENTINEL).all()
        # time_step NULL means 0
        zero = dict(s, time_step=np.zeros(M, np.int64))
        assert np.array_equal(_masks(env, s, d, time_step=False), _masks(env, zero, d))
        # a time_step of 999: the step truncates unless it crashes, so it is safe wherever it does not crash, at every depth
        last = dict(s, time_step=np.full(M, 999))
        want = _masks(env, zero, 1)
        assert np.array_equal(_masks(env, last, d), want), d
        if d > 1:
            assert (full != want).any()      # (without the limit the deeper search does find more doom)
    after = env.get_state()
    for k in before:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k      # the handle's own state is neither read nor written
    env.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_edges_two_tracks_in_one_wave_and_unknown_track(dtype):
    n = 16
    s = _mixed_rows("big_track", n)
    M = len(s["px"])
    singles = []
    for track in ("track", "big_track"):
        env = _env(track, n, dtype)
        singles.append([_masks(env, s, d) for d in (1, 3)])
        env.close()
    env = pc.VecCarEnv(2, [TRACKS["track"], TRACKS["big_track"]], num_rays=n, reward_scaling=R.REWARD_SCALE, dtype=dtype,
                       track_id=np.array([0, 1], np.uint8))
    tid = (np.arange(M) & 1).astype(np.uint8)
    tid2 = tid.copy()
    tid2[[0, 100, 256]] = (2, 255, 7)
    bad = tid2 >= 2
    active = (np.arange(M) % 4 != 0).astype(np.uint8)
    for i, d in enumerate((1, 3)):
        both = _masks(env, s, d, track_id=tid)
        for k in (0, 1):
            assert np.array_equal(both[tid == k], singles[k][i][tid == k]), (d, k)
        assert not np.array_equal(both[0::2], singles[1][i][0::2])      # (the two tracks do differ)
        got = _masks(env, s, d, track_id=tid2)
        assert (got[bad] == 0).all() and np.array_equal(got[~bad], both[~bad])      # an id the handle does not have: 9 zeros
        part = _masks(env, s, d, track_id=tid2, active=active)
        assert np.array_equal(part[active != 0], got[active != 0]) and (part[active == 0] == SENTINEL).all()
    env.close()


# ---- 6. the landscape --------------------------------------------------------------------------------------------------------------
def test_viability_equals_lookahead_at_depth_1_and_a_plain_loop_at_depth_2():
    agent = pc.Agent(23, 9)
    load_trained_policy(agent)
    agent = agent.cuda()
    ls = pc.PolicyLandscape(agent, TRACKS["big_track"], 16, cell_px=80, speed=0.5, dtype="f32", device="cuda")
    with pytest.raises(RuntimeError):
        ls.viability(1)
    ls.compute().lookahead().viability(1)
    bit = torch.arange(9, dtype=torch.int32, device="cuda")
    v = ls.viable.to(torch.int32)
    assert ls.viable.dtype == torch.uint16 and ls.viable.shape == (1, 72, 9, 16) and ls.viability_depth == 1
    assert torch.equal(((v.unsqueeze(-1) >> bit) & 1).sum(-1).to(torch.uint8), ls.safe_actions)
    assert torch.equal(ls.avoidable_late, ls.avoidable) and torch.equal(ls.doomed, ls.drivable & (ls.safe_actions == 0))
    assert ls.viability(2).viability_depth == 2
    px, py, vx, vy, turns, tid = ls.poses()
    safe = ls.envs.safe_actions(px, py, vx, vy, turns, depth=2, track_id=tid)      # every pose, no active mask
    drivable, greedy = ls.drivable.view(-1), ls.action.view(-1).to(torch.int64)
    bits = (safe.to(torch.int32) << bit).sum(1)
    want = torch.where(drivable, bits, torch.zeros_like(bits))
    v = ls.viable.view(-1).to(torch.int32)
    assert torch.equal(v, want) and int(v.max()) == 0x1ff
    assert torch.equal(ls.doomed.view(-1), drivable & (want == 0)) and ls.doomed.any()
    late = drivable & ~safe.gather(1, greedy.unsqueeze(1)).squeeze(1) & (want != 0)
    assert torch.equal(ls.avoidable_late.view(-1), late)
    ls.close()


# ---- 7. the shield -----------------------------------------------------------------------------------------------------------------
N_EV, DEPTH = 64, 2


def _trained_agent():
    agent = pc.Agent(23, 9).cuda()
    load_trained_policy(agent)
    return agent


def _shield_loop(agent, greedy, seed, index):
    """1000 x (pc_policy_act_greedy, or pc_policy_act at (seed, index * 1000 + t); action_masks; the replacement rule in numpy; step)."""
    env = pc.VecCarEnv(N_EV, TRACKS["big_track"], num_rays=16, reward_scaling=0.1, device="cuda", dtype="f32")
    agent.rng_seed = seed
    obs, _ = env.reset()
    rew, term, trunc = (torch.empty(1000, N_EV, device="cuda") for _ in range(3))
    logits = torch.empty(N_EV, 9, device="cuda")
    running = np.ones(N_EV, bool)
    counts = np.zeros(3)
    with torch.no_grad():
        for t in range(1000):
            a, _, _ = agent.act(obs, out_logits=logits, greedy=greedy, offset=index * 1000 + t, repack=t == 0)
            a, lg, mask = a.cpu().numpy(), logits.cpu().numpy(), env.action_masks(DEPTH).cpu().numpy()
            doomed = ~mask.any(1)
            replace = ~mask[np.arange(N_EV), a] & ~doomed
            best = np.where(mask, lg, -np.finfo(np.float32).max).argmax(1)      # the first maximum over the safe actions
            a = np.where(replace, best, a)
            counts += (running.sum(), (running & replace).sum(), (running & doomed).sum())
            env.step(torch.from_numpy(a).cuda(), out=(obs, rew[t], term[t], trunc[t]))
            running &= ~((term[t] + trunc[t]) > 0).cpu().numpy()
    env.close()
    return first_episodes_ref(rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), 0.1), counts


# trained-greedy is the case to hold.  The fixture's argmax drives every env into the same wall from too far out for a 2-step shield (its
# crashes are strategic: doomed steps, no intervention), so the same policy SAMPLED makes the replacement rule work -- and its draws must be
# the unshielded evaluation's: the stream is not touched.
@pytest.mark.parametrize("case", ["trained-greedy", "trained-sampled"])
def test_shielded_evaluation_equals_a_plain_loop(case):
    agent = _trained_agent()
    greedy, seed, index = case == "trained-greedy", 1234, 3
    kw = dict(n_envs=N_EV, num_rays=16, reward_scaling=0.1, device="cuda", greedy=greedy, seed=seed)
    ev = Evaluator(agent, TRACKS["big_track"], shield_depth=DEPTH, **kw)
    ev.run(index)
    out = ev.scalars(ev.totals().tolist(), host_shield_totals=ev.shield_totals().tolist())
    assert ev.last_path == "steps" and set(out) == set(EVAL_KEYS) | set(SHIELD_KEYS)
    state, counts = ev.state.cpu().numpy(), ev.shield_totals().cpu().numpy()
    want_state, want_counts = _shield_loop(agent, greedy, seed, index)
    assert np.array_equal(_bits(state), _bits(np.asarray(want_state, np.float64)))      # hence totals(): a fixed-order reduction of the state
    assert np.array_equal(counts, want_counts) and counts[0] == state[1].sum()      # the counted steps are the first episodes' lengths
    assert out["eval/shield_interventions"] == want_counts[1] / want_counts[0] and out["eval/shield_doomed"] == want_counts[2] / want_counts[0]
    # a second run starts its counts afresh
    ev.run(index)
    assert np.array_equal(ev.shield_totals().cpu().numpy(), counts) and np.array_equal(_bits(ev.state.cpu().numpy()), _bits(state))
    ev.close()
    # off: the bits and the keys of an evaluator that never heard of a shield
    plain, off = Evaluator(agent, TRACKS["big_track"], rollout_kernel="steps", **kw), Evaluator(agent, TRACKS["big_track"], shield_depth=0,
                                                                                                rollout_kernel="steps", **kw)
    plain.run(index); off.run(index)
    d_plain, d_off = plain.scalars(plain.totals().tolist()), off.scalars(off.totals().tolist())
    assert d_plain == d_off and set(d_off) == set(EVAL_KEYS) and off._shield is None
    assert np.array_equal(_bits(plain.totals().cpu().numpy()), _bits(off.totals().cpu().numpy()))
    assert np.array_equal(_bits(plain.state.cpu().numpy()), _bits(off.state.cpu().numpy()))
    with pytest.raises(RuntimeError):
        off.shield_totals()
    print(case, "crash rate", d_plain["eval/crash_rate"], "shielded", out["eval/crash_rate"], "steps / replaced / doomed", counts)
    # an env that crashes under the shield was doomed in its last step: a replacement is safe for one step at least, so the action that
    # crashed was the policy's own, unsafe, with no safe action beside it
    assert counts[2] >= (state[4] == 1).sum()
    if case == "trained-sampled":
        assert want_counts[1] > 0      # the shield did step in ...
        assert not np.array_equal(_bits(plain.state.cpu().numpy()), _bits(state))      # ... and the episodes are not the unshielded ones
    plain.close(); off.close()


def test_evaluator_refuses_a_shield_it_cannot_run():
    agent = pc.Agent(23, 9).cuda()
    kw = dict(n_envs=8, num_rays=16, device="cuda")
    for bad in (dict(shield_depth=5), dict(shield_depth=-1), dict(shield_depth=2, rollout_kernel="mega"),
                dict(shield_depth=1, rollout_kernel="mega", greedy=True)):
        with pytest.raises(ValueError):
            Evaluator(agent, TRACKS["big_track"], **kw, **bad)
    ev = Evaluator(agent, TRACKS["big_track"], shield_depth=1, **kw)      # "auto" with a shield: the per-step path, sampled too
    ev.run()
    assert ev.last_path == "steps"
    ev.close()


def test_evaluate_shield_option(tmp_path, capsys):
    import json

    import evaluate
    torch.save(_trained_agent().state_dict(), tmp_path / "model.dat")
    base = ["--checkpoint", str(tmp_path / "model.dat"), "--track", TRACKS["big_track"], "--num-rays", "16", "--envs", "32", "--greedy"]
    out = evaluate.main(base + ["--shield", "2"])
    assert set(EVAL_KEYS) | set(SHIELD_KEYS) <= set(out) and out["path"] == "steps"
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    assert 0.0 <= out["eval/shield_interventions"] <= 1.0 and 0.0 <= out["eval/shield_doomed"] <= 1.0
    assert not set(SHIELD_KEYS) & set(evaluate.main(base))
    with pytest.raises(ValueError, match="--shield"):
        evaluate.main(base + ["--shield", "2", "--rollout-kernel", "mega"])
