"""Episode statistics on the GPU (K3e: gae_kernel<1,0,1,0>, <0,0,1,STEPS>): per env bit for bit against the forward numpy
reference of test_episode_stats_host.py on synthetic buffers, against the env's own gate count on real rollouts, through
VecCarEnv(record_episode_statistics=True), and through the Trainer (PPOConfig.episode_stats) and train.py --episode-stats."""
import io
import json
import os

import numpy as np
import pytest
import torch

import ppo_car_amd as pc
from ppo_car_amd import _capi
from ppo_car_amd.episodes import EPISODE_MEAN_KEYS, EpisodeStats, episode_scalars
from ppo_car_amd.ppo import PPOConfig, Trainer
from conftest import TRACKS
from test_episode_stats_host import ALPHABET, buffer_dones, episodes_ref, init_out

pytestmark = pytest.mark.gpu

EP_KEYS = ("charts/episodes",) + EPISODE_MEAN_KEYS


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _eq(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (what, np.argwhere(_bits(a) != _bits(b))[:5])


def _synthetic(T, N, s, seed):
    rng = np.random.default_rng(seed)
    rew = (ALPHABET[rng.integers(0, len(ALPHABET), size=(T, N))] * s).astype(np.float32)
    p = rng.choice([0.0, 0.01, 0.2], size=N)                       # per env: no dones, rare, frequent
    term = (rng.random((T, N)) < p / 2).astype(np.float32)
    trunc = (rng.random((T, N)) < p / 2).astype(np.float32)
    lt = (rng.random(N) < 0.1).astype(np.float32)
    ltr = (rng.random(N) < 0.1).astype(np.float32)
    val = rng.standard_normal((T, N)).astype(np.float32)
    lv = rng.standard_normal(N).astype(np.float32)
    carry = np.zeros((4, N))                                       # a third fresh, a third sentinel, a third mid-episode
    kind = np.arange(N) % 3
    carry[1, kind == 1] = -1.0
    m = kind == 2
    steps = rng.integers(1, 500, size=N)
    carry[0, m] = np.round(steps[m] * 0.01 * s / 2.0 ** -30) * 2.0 ** -30
    carry[1, m] = steps[m]
    carry[2, m] = steps[m] // 50
    carry[3, m] = steps[m] // 400
    return rew, val, term, trunc, lv, lt, ltr, carry


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gae(rew, val, term, trunc, lv, lt, ltr, episodes=None):
    T, N = rew.shape
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    s = torch.cuda.current_stream().cuda_stream
    if episodes is None:
        _capi.check(_capi.lib.pc_gae(0, rew.data_ptr(), val.data_ptr(), term.data_ptr(), trunc.data_ptr(), lv.data_ptr(), lt.data_ptr(),
                                     ltr.data_ptr(), 0.99, 0.95, T, N, adv.data_ptr(), ret.data_ptr(), s), "pc_gae")
    else:
        sc, carry, out = episodes
        _capi.check(_capi.lib.pc_gae_episodes(0, rew.data_ptr(), val.data_ptr(), term.data_ptr(), trunc.data_ptr(), lv.data_ptr(),
                                              lt.data_ptr(), ltr.data_ptr(), 0.99, 0.95, T, N, adv.data_ptr(), ret.data_ptr(), sc,
                                              carry.data_ptr(), out.data_ptr(), s), "pc_gae_episodes")
    return adv, ret


def _stats(rew, term, trunc, lt, ltr, layout, s, carry, out):
    T, N = rew.shape
    _capi.check(_capi.lib.pc_episode_stats(0, rew.data_ptr(), term.data_ptr(), trunc.data_ptr(), None if lt is None else lt.data_ptr(),
                                           None if ltr is None else ltr.data_ptr(), T, N, layout, s, carry.data_ptr(), out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "pc_episode_stats")


@pytest.mark.parametrize("N", [1, 255, 257, 4096, 65536])
@pytest.mark.parametrize("T", [1, 7, 8, 9, 1000, 1024])
def test_synthetic_buffers_bitwise(T, N):
    s = (0.1, 0.37, 1.0)[(T + N) % 3]
    rew, val, term, trunc, lv, lt, ltr, carry = _synthetic(T, N, s, seed=T * 100003 + N)
    ref_out, ref_carry = episodes_ref(rew, buffer_dones(term, trunc, lt, ltr), s, carry)
    R, V, TE, TR, LV, LT, LTR = map(_dev, (rew, val, term, trunc, lv, lt, ltr))
    adv0, ret0 = _gae(R, V, TE, TR, LV, LT, LTR)
    c1, o1 = _dev(carry), _dev(init_out(N))
    adv1, ret1 = _gae(R, V, TE, TR, LV, LT, LTR, episodes=(s, c1, o1))
    c2, o2 = _dev(carry), _dev(init_out(N))
    _stats(R, TE, TR, LT, LTR, _capi.PC_EPISODE_BUFFER, s, c2, o2)
    torch.cuda.synchronize()
    assert torch.equal(adv0.view(torch.int32), adv1.view(torch.int32)) and torch.equal(ret0.view(torch.int32), ret1.view(torch.int32))
    _eq(o1.cpu().numpy(), ref_out, "fused out")
    _eq(c1.cpu().numpy(), ref_carry, "fused carry")
    _eq(o2.cpu().numpy(), o1.cpu().numpy(), "standalone out")
    _eq(c2.cpu().numpy(), c1.cpu().numpy(), "standalone carry")
    # the STEPS layout: flags[t] belong to rew[t]; k chained calls = one call over the concatenated window (out accumulates)
    done = buffer_dones(term, trunc, lt, ltr).astype(np.float32)
    zero = np.zeros_like(done)
    c3, o3 = _dev(carry), _dev(init_out(N))
    cuts = sorted({0, T, T // 3, (2 * T) // 3})
    for a, b in zip(cuts[:-1], cuts[1:]):
        _stats(_dev(rew[a:b]), _dev(done[a:b]), _dev(zero[a:b]), None, None, _capi.PC_EPISODE_STEPS, s, c3, o3)
    torch.cuda.synchronize()
    _eq(o3.cpu().numpy(), ref_out, "chained steps out")
    _eq(c3.cpu().numpy(), ref_carry, "chained steps carry")


# ---- an independent source: the env's own counters -------------------------------------------------------------------------------
def test_idle_envs_truncate_at_1000_with_return_0():
    """Action 8 (no thrust, no turn): every episode ends by the time limit after 1000 steps with return 0 and no gate."""
    N = 256
    env = pc.VecCarEnv(N, TRACKS["big_track"], num_rays=16, reward_scaling=0.1, device="cuda", record_episode_statistics=True)
    env.reset()
    a = torch.full((N,), 8, dtype=torch.int64, device="cuda")
    seen = 0
    for t in range(1000):
        _, _, term, trunc, info = env.step(a)
        if t < 999:
            seen += int(info["_episode"].sum())
    assert seen == 0
    assert bool(info["_episode"].all()) and bool((trunc != 0).all()) and not bool((term != 0).any())
    ep = info["episode"]
    assert bool((ep["l"] == 1000).all()) and bool((ep["r"] == 0).all()) and bool((ep["gates"] == 0).all()) and bool((ep["laps"] == 0).all())
    s = {k: float(v) for k, v in env.episode_statistics().items()}
    assert s["episodes"] == N and s["length"] == 1000 and s["return"] == 0 and s["return_max"] == 0
    env.close()


def test_trained_policy_gates_match_the_env():
    """The trained policy (tests/golden/policy_trained.npz, ~3 laps per episode) stepped by VecCarEnv.step: the gates decoded from the
    rewards of every finished episode equal the env's own gates_passed at the done, and episodes lap."""
    from oracle.scenarios import load_trained_policy
    N, T = 512, 1100
    env = pc.VecCarEnv(N, TRACKS["big_track"], num_rays=16, reward_scaling=0.1, device="cuda", record_episode_statistics=True)
    agent = pc.Agent(env.obs_dim, env.act_dim).cuda()
    load_trained_policy(agent)
    obs, _ = env.reset()
    gp = torch.empty(N, dtype=torch.int32, device="cuda")
    finished = laps = 0
    rows = []
    with torch.no_grad():
        for t in range(T):
            act, _, _, _ = agent.get_action_and_value(obs)
            obs, rew, term, trunc, info = env.step(act, gates_passed=gp)
            m = info["_episode"]
            assert torch.equal(info["episode"]["gates"][m], gp[m])
            finished += int(m.sum())
            laps += int(info["episode"]["laps"][m].sum())
            rows.append((rew.clone(), ((term != 0) | (trunc != 0)).clone(), info["episode"]["l"].clone(), m.clone()))
    assert finished >= N // 2 and laps > 0, (finished, laps)
    rew = torch.stack([r[0] for r in rows]).cpu().numpy()
    done = torch.stack([r[1] for r in rows]).cpu().numpy()
    ref_out, _ = episodes_ref(rew, done, 0.1)
    s = env.episode_statistics()
    assert float(s["episodes"]) == ref_out[0].sum() == finished
    assert float(s["laps"]) * finished == pytest.approx(ref_out[4].sum(), rel=1e-12)
    env.close()


# ---- VecCarEnv(record_episode_statistics=True) ----------------------------------------------------------------------------------------
def _actions(T, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randint(0, 9, (T, N), generator=g, device="cuda")
    a[torch.rand(T, N, generator=g, device="cuda") < 0.6] = 0      # mostly forward: gates and crashes
    return a


def test_record_step_infos_and_step_many():
    N, T = 512, 300
    acts = _actions(T, N, 3)
    a = pc.VecCarEnv(N, TRACKS["big_track"], num_rays=16, reward_scaling=0.1, device="cuda", record_episode_statistics=True)
    b = pc.VecCarEnv(N, TRACKS["big_track"], num_rays=16, reward_scaling=0.1, device="cuda", record_episode_statistics=True)
    c = pc.VecCarEnv(N, TRACKS["big_track"], num_rays=16, reward_scaling=0.1, device="cuda")
    a.reset(); b.reset(); c.reset()
    rews, dones = [], []
    ref_carry = np.zeros((4, N))
    for t in range(T):
        o, r, te, tr, info = a.step(acts[t])
        oc, rc, tec, trc, infoc = c.step(acts[t])
        assert torch.equal(o, oc) and torch.equal(r, rc) and torch.equal(te, tec) and torch.equal(tr, trc)
        assert set(infoc) == set() and set(info) == {"episode", "_episode"}
        rn = r.cpu().numpy()[None]
        dn = ((te != 0) | (tr != 0)).cpu().numpy()[None]
        out, ref_carry = episodes_ref(rn, dn, 0.1, ref_carry)
        m = out[0] > 0
        assert np.array_equal(info["_episode"].cpu().numpy(), m)
        assert info["episode"]["r"].dtype == torch.float64 and info["episode"]["l"].dtype == torch.int32
        _eq(info["episode"]["r"].cpu().numpy()[m], out[1][m] / 0.1, "r")
        assert np.array_equal(info["episode"]["l"].cpu().numpy()[m], out[2][m])
        assert np.array_equal(info["episode"]["gates"].cpu().numpy()[m], out[3][m])
        assert np.array_equal(info["episode"]["laps"].cpu().numpy()[m], out[4][m])
        rews.append(rn[0]); dones.append(dn[0])
    ref_out, _ = episodes_ref(np.stack(rews), np.stack(dones), 0.1)
    b.step_many(acts)
    _eq(b._episodes.out.cpu().numpy(), a._episodes.out.cpu().numpy(), "step_many out vs T x step")
    _eq(b._episodes.carry.cpu().numpy(), a._episodes.carry.cpu().numpy(), "step_many carry vs T x step")
    _eq(a._episodes.out.cpu().numpy(), ref_out, "running out vs numpy")
    sa = {k: v.item() for k, v in a.episode_statistics().items()}
    assert sa["episodes"] == ref_out[0].sum() > 0
    assert sa["length"] == pytest.approx(ref_out[2].sum() / ref_out[0].sum(), rel=1e-12)
    assert sa["return"] == pytest.approx(ref_out[1].sum() / ref_out[0].sum() / 0.1, rel=1e-12)
    assert sa["return_min"] == ref_out[5].min() / 0.1 and sa["return_max"] == ref_out[6].max() / 0.1
    after = {k: v.item() for k, v in a.episode_statistics().items()}       # cleared by the call before
    assert after["episodes"] == 0 and np.isnan(after["return"])
    with pytest.raises(RuntimeError):
        c.episode_statistics()
    a.set_state(time_step=np.zeros(N, np.int64))                            # an injected state: its episodes' starts are unknown
    assert bool((a._episodes.carry[1] == -1).all())
    a.reset()
    assert bool((a._episodes.carry == 0).all())
    for e in (a, b, c):
        e.close()


# ---- the Trainer --------------------------------------------------------------------------------------------------------------------
def _cfg(n_envs, **kw):
    base = dict(n_envs=n_envs, n_steps=64, batch_size=64 if n_envs <= 256 else 512, train_iters=2, track=TRACKS["big_track"], num_rays=16,
                seed=5)
    base.update(kw)
    return PPOConfig(**base)


def _snap(tr):
    b = tr.buffer
    return [x.clone() for x in (b.obs_buf, b.act_buf, b.rew_buf, b.val_buf, b.term_buf, b.trunc_buf, b.logprob_buf, b.adv_buf, b.ret_buf,
                                tr.next_obs, tr.next_term, tr.next_trunc,
                                torch.cat([p.detach().reshape(-1) for p in tr.agent.parameters()]))]


OLD_KEYS = ("losses/policy_loss", "losses/value_loss", "losses/entropy", "losses/total_loss", "charts/avg_reward", "charts/learning_rate",
            "global_step")


@pytest.mark.parametrize("n_envs,kw", [(256, dict(rollout_kernel="steps")), (256, dict(rollout_kernel="steps", env_dtype="f64")),
                                       (4096, dict(rollout_kernel="mega"))])
def test_trainer_stats_on_equals_off_and_matches_numpy(n_envs, kw):
    E = 3
    off, on = Trainer(_cfg(n_envs, **kw), device="cuda"), Trainer(_cfg(n_envs, episode_stats=True, **kw), device="cuda")
    ref_carry = np.zeros((4, n_envs))
    total_eps = 0
    for ep in range(E):
        s0, s1 = off.run_epoch(), on.run_epoch()
        assert set(s1) == set(s0) | set(EP_KEYS) and not set(s0) & set(EP_KEYS)
        for k in OLD_KEYS:
            assert s0[k] == s1[k], k
        for x, y in zip(_snap(off), _snap(on)):
            assert torch.equal(x, y)
        b = on.buffer
        done = buffer_dones(b.term_buf.cpu().numpy(), b.trunc_buf.cpu().numpy(), on.next_term.cpu().numpy(), on.next_trunc.cpu().numpy())
        ref_out, ref_carry = episodes_ref(b.rew_buf.cpu().numpy(), done, 0.1, ref_carry)
        _eq(on.episodes.out.cpu().numpy(), ref_out, f"epoch {ep} out")
        _eq(on.episodes.carry.cpu().numpy(), ref_carry, f"epoch {ep} carry")
        want = episode_scalars([ref_out[0].sum(), ref_out[1].sum(), ref_out[2].sum(), ref_out[3].sum(), ref_out[4].sum(), ref_out[5].min(),
                                ref_out[6].max()], 0.1)
        for k in EP_KEYS:
            assert (s1[k] is None) == (want[k] is None) and (want[k] is None or s1[k] == pytest.approx(want[k], rel=1e-12)), k
        total_eps += s1["charts/episodes"]
    assert total_eps > 0
    off.close(); on.close()


def test_trainer_lazy_resume_and_statsless_checkpoint():
    cfg = _cfg(256, episode_stats=True, rollout_kernel="steps")
    ref = Trainer(cfg, device="cuda")
    rows = [ref.run_epoch() for _ in range(4)]
    # sync="lazy": the same rows one epoch late
    lz = Trainer(cfg, device="cuda")
    got = [lz.run_epoch(sync="lazy") for _ in range(4)] + [lz.flush_scalars()]
    assert got[0] is None
    for a, b in zip(rows, got[1:]):
        for k in EP_KEYS:
            assert a[k] == b[k], k
    lz.close()
    # resume after 2 epochs = the uninterrupted run; a checkpoint without "episodes" drops exactly the in-progress episodes
    A = Trainer(cfg, device="cuda")
    A.run_epoch(); A.run_epoch()
    buf = io.BytesIO()
    torch.save(A.state_dict(), buf)
    assert "episodes" in A.state_dict()
    A.close()
    for statsless in (False, True):
        buf.seek(0)
        sd = torch.load(buf, map_location="cuda", weights_only=False)
        if statsless:
            del sd["episodes"]
        B = Trainer(cfg, device="cuda")
        B.load_state_dict(sd)
        carry0 = B.episodes.carry.cpu().numpy()
        s = B.run_epoch()
        if not statsless:
            for k in EP_KEYS:
                assert s[k] == rows[2][k], k
        else:
            assert (carry0[1] == -1).all()
            b = B.buffer
            done = buffer_dones(b.term_buf.cpu().numpy(), b.trunc_buf.cpu().numpy(), B.next_term.cpu().numpy(), B.next_trunc.cpu().numpy())
            ref_out, _ = episodes_ref(b.rew_buf.cpu().numpy(), done, 0.1, carry0)
            _eq(B.episodes.out.cpu().numpy(), ref_out, "statsless out")
            assert s["charts/episodes"] == ref_out[0].sum() < rows[2]["charts/episodes"]
            for k in OLD_KEYS:
                assert s[k] == rows[2][k], k
        B.close()
    # a stats-less trainer writes no "episodes" key
    C = Trainer(_cfg(256, rollout_kernel="steps"), device="cuda")
    assert "episodes" not in C.state_dict()
    C.close()
    ref.close()


# ---- train.py --episode-stats -------------------------------------------------------------------------------------------------------
def test_train_cli_episode_stats_rows(tmp_path):
    import train
    keys = {}
    for name, extra in (("plain", []), ("stats", ["--episode-stats"])):
        out = str(tmp_path / name)
        train.main(["--run-name", name, "--n-epochs", "3", "--cuda", "--track", TRACKS["big_track"], "--n-envs", "256", "--n-steps", "64",
                    "--batch-size", "64", "--train-iters", "2", "--num-rays", "16", "--out-dir", out] + extra)
        lg = sorted(os.listdir(os.path.join(out, "logs")))
        rows = [json.loads(l) for l in open(os.path.join(out, "logs", lg[0], "scalars.jsonl"))]
        assert len(rows) == 3
        keys[name] = set(rows[0])
        if name == "stats":
            assert all(set(EP_KEYS) <= set(r) for r in rows)
            assert sum(r["charts/episodes"] for r in rows) > 0
    assert keys["stats"] == keys["plain"] | set(EP_KEYS) and not keys["plain"] & set(EP_KEYS)
