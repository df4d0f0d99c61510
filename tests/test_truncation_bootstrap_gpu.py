"""Truncation bootstrap on the GPU: K3b gae_kernel<1,1,EPI,0> (pc_gae_bootstrap) against a float32 torch restatement bit for bit, the
final-observation capture of every persistent rollout family (pc_rollout_final_obs) against the per-step kernel K1's final_obs, the
value pass of both bootstrap_value arithmetics, the Trainer's three rollout paths, and train.py --truncation-bootstrap."""
import json
import os

import numpy as np
import pytest
import torch

from ppo_car_amd import Buffer, _capi
from ppo_car_amd.episodes import EpisodeStats
from ppo_car_amd.ppo import PPOConfig, Trainer
from conftest import TRACKS
from oracle.scenarios import load_trained_policy
from test_rollout_baseline_gpu import _snap
from test_rollout_rare_branches_gpu import _inject
from test_truncation_bootstrap_host import gae_bootstrap_ref

pytestmark = pytest.mark.gpu

LIMIT = _capi.PC_TIME_LIMIT
MIXED = [TRACKS["track"], TRACKS["big_track"]]


# ---- 1. the GAE kernel ------------------------------------------------------------------------------------------------------------
def torch_gae_bootstrap(rew, val, term, trunc, lv, lt, ltr, fv, gamma, lam):
    """The reference's torch expression (buffer.py:51-63) in float32 with next_v replaced at truncated steps."""
    T = rew.shape[0]
    adv = torch.zeros_like(rew)
    last_gae = torch.zeros_like(lv)
    for t in reversed(range(T)):
        if t == T - 1:
            next_vals, term_mask, trunc_mask, tr = lv, 1.0 - lt, 1.0 - ltr, ltr
        else:
            next_vals, term_mask, trunc_mask, tr = val[t + 1], 1.0 - term[t + 1], 1.0 - trunc[t + 1], trunc[t + 1]
        next_v = torch.where(tr != 0, fv[t // LIMIT], next_vals)
        delta = rew[t] + gamma * next_v * term_mask - val[t]
        last_gae = delta + gamma * lam * term_mask * trunc_mask * last_gae
        adv[t] = last_gae
    return adv, adv + val


def _synthetic(T, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rew = torch.randn(T, N, device="cuda", generator=g)
    val = torch.randn(T, N, device="cuda", generator=g)
    term = (torch.rand(T, N, device="cuda", generator=g) < 0.02).float()
    trunc = torch.zeros(T, N, device="cuda")
    lv = torch.randn(N, device="cuda", generator=g)
    lt = (torch.rand(N, device="cuda", generator=g) < 0.02).float()
    ltr = torch.zeros(N, device="cuda")
    K = -(-T // LIMIT)
    n = torch.arange(N, device="cuda")
    for k in range(K):     # one truncation per (slot, env), at a random step of the slot; the edge steps are forced for some envs
        lo, hi = k * LIMIT, min(T, (k + 1) * LIMIT)
        t = torch.randint(lo, hi, (N,), device="cuda", generator=g)
        t[n % 7 == 0] = hi - 1                      # the slot's last step (t = 999, T - 1)
        t[n % 7 == 1] = lo                          # its first (t = 1000)
        last = t == T - 1
        ltr[last], lt[last] = 1.0, 0.0
        rows = (t + 1).clamp(max=T - 1)
        sel = ~last
        trunc[rows[sel], n[sel]] = 1.0
        term[rows[sel], n[sel]] = 0.0
    fv = torch.randn(K, N, device="cuda", generator=g) * 3.0
    return rew, val, term, trunc, lv, lt, ltr, fv


@pytest.mark.parametrize("N", [1, 257, 65536])
@pytest.mark.parametrize("T", [1, 7, 1000, 1001, 2500])
def test_gae_bootstrap_kernel_bitwise(T, N):
    rew, val, term, trunc, lv, lt, ltr, fv = _synthetic(T, N, T * 7 + N)
    K = fv.shape[0]
    buf = Buffer((1,), T, N, "cuda:0")
    buf.rew_buf.copy_(rew); buf.val_buf.copy_(val); buf.term_buf.copy_(term); buf.trunc_buf.copy_(trunc)
    buf.ptr = T
    a, r = buf.calculate_advantages(lv, lt, ltr, final_values=fv)
    a, r = a.clone(), r.clone()
    A, R = torch_gae_bootstrap(rew, val, term, trunc, lv, lt, ltr, fv, 0.99, 0.95)
    assert torch.equal(a, A) and torch.equal(r, R)
    if T > 1000:
        assert int(trunc[1000].sum()) > 0           # truncations at t = 999 ...
    if T > 1001 and N > 1:
        assert int(trunc[1001].sum()) > 0           # ... and at t = 1000 (slot 1)
    assert int(ltr.sum()) > 0 or N == 1 or T == 1
    if T == 2500:
        assert K == 3
    # final_val = the next rows' values: pc_gae itself, bit for bit
    nxt = torch.cat([val[1:], lv[None]], 0)
    flags = torch.cat([trunc[1:], ltr[None]], 0) != 0
    fv_same = torch.zeros_like(fv)
    for k in range(K):
        lo, hi = k * LIMIT, min(T, (k + 1) * LIMIT)
        m = flags[lo:hi]
        fv_same[k] = torch.where(m.any(0), (nxt[lo:hi] * m).sum(0), fv_same[k])      # one truncation per (slot, env): the sum is the value
    a1, r1 = buf.calculate_advantages(lv, lt, ltr, final_values=fv_same)
    a1, r1 = a1.clone(), r1.clone()
    a0, r0 = buf.calculate_advantages(lv, lt, ltr)
    assert torch.equal(a1, a0) and torch.equal(r1, r0)
    # the episodes instance: adv / ret as the plain instance, statistics as pc_gae_episodes
    e1, e0 = EpisodeStats(N, 0.1, torch.device("cuda", 0)), EpisodeStats(N, 0.1, torch.device("cuda", 0))
    a2, r2 = buf.calculate_advantages(lv, lt, ltr, episodes=e1, final_values=fv)
    assert torch.equal(a2, A) and torch.equal(r2, R)
    buf.calculate_advantages(lv, lt, ltr, episodes=e0)
    assert torch.equal(e1.out, e0.out) and torch.equal(e1.carry, e0.carry)
    # float64 numpy restatement (host file): agreement to float32 rounding
    if T * N <= 1001 * 257:
        cpu = lambda x: x.double().cpu().numpy()
        A64, _ = gae_bootstrap_ref(cpu(rew), cpu(val), cpu(term), cpu(trunc), cpu(lv), cpu(lt), cpu(ltr), cpu(fv), 0.99, 0.95)
        assert np.abs(cpu(a) - A64).max() < 1e-4


# ---- 2. the capture in every persistent family ----------------------------------------------------------------------------------
def _inject_times(tr, n_envs):
    st = tr.envs.get_state()
    st["time_step"] = 990 + np.arange(n_envs) % 10       # truncations at t = 0 .. 9 (cars at the start line, a fresh policy)
    tr.envs.set_state(**st)


def _run(kw, mode, tb, inject, T, trained=False):
    kw = dict(kw)
    kw.setdefault("policy_split", 1 if kw["n_envs"] <= 8192 else 0)      # the persistent form's policy arithmetic on the per-step path too
    cfg = PPOConfig(n_steps=T, rollout_kernel=mode, use_graphs=False, seed=41, truncation_bootstrap=tb, **kw)
    tr = Trainer(cfg, device="cuda")
    if trained:
        load_trained_policy(tr.agent)
    if inject == "inject":
        _inject(tr, cfg, cfg.n_envs)
    elif inject == "times":
        _inject_times(tr, cfg.n_envs)
    else:
        st = tr.envs.get_state()
        st["time_step"] = np.full(cfg.n_envs, 999)      # every env truncates at t = 0; the survivors again at t = 1000 (slot 1)
        tr.envs.set_state(**st)
    tr.rollout()
    torch.cuda.synchronize()
    out = dict(snap=_snap(tr), state=tr.envs.get_state(), mode=tr.rollout_mode, kernel=tr.envs.last_rollout_kernel())
    if mode == "mega":
        out["aux"] = (tr._boot_val.clone(), tr._rew_sum.clone())
    if tb == "final_obs":
        out["final_obs"] = tr.buffer.final_obs_buf.clone()
    tr.close()
    return out


def _truncations(snap):
    """[T, N] bool: step t of env n truncated (its flag in trunc row t + 1, next_trunc for t = T - 1)."""
    trunc, next_trunc = snap[6], snap[9]
    return torch.cat([trunc[1:], next_trunc[None]], 0) != 0


CAPTURE = [
    # id, PPOConfig fields, injection, expected kernel
    ("K9", dict(n_envs=65536, num_rays=16, track=TRACKS["big_track"]), "inject", "K9"),
    ("K9M", dict(n_envs=20000, num_rays=16, track=TRACKS["big_track"]), "inject", "K9m"),
    ("K9S", dict(n_envs=4096, num_rays=16, track=TRACKS["big_track"], policy_split=1), "inject", "K9s"),
    ("K9S_epw32", dict(n_envs=8000, num_rays=16, track=TRACKS["big_track"], policy_split=1, rollout_epw=32), "inject", "K9s"),
    ("K9_33rays", dict(n_envs=40000, num_rays=32, track=TRACKS["big_track"]), "inject", "K9"),
    ("K9S_12rays", dict(n_envs=3000, num_rays=12, track=TRACKS["track"], policy_split=1), "inject", "K9s"),
    ("K9_generic", dict(n_envs=65536, num_rays=16, track=TRACKS["big_track"], rollout_fast=0), "inject", "K9"),
    ("K9S_generic", dict(n_envs=4096, num_rays=16, track=TRACKS["big_track"], policy_split=1, rollout_fast=0), "inject", "K9s"),
    ("K9_lit", dict(n_envs=65536, num_rays=16, track=TRACKS["big_track"], env_dtype="f64"), "inject", "K9-literal"),
    ("K9M_lit", dict(n_envs=20000, num_rays=16, track=TRACKS["big_track"], env_dtype="f64"), "inject", "K9m-literal"),
    ("K9S_lit", dict(n_envs=4096, num_rays=16, track=TRACKS["big_track"], env_dtype="f64", policy_split=1), "inject", "K9s-literal"),
    ("K9D_filter", dict(n_envs=20480, num_rays=16, track=TRACKS["big_track"], env_dtype="f64", rollout_fast=0), "inject", "K9d-filter"),
    ("K9D_selector", dict(n_envs=65536, num_rays=16, track=MIXED, track_interleave=True, env_dtype="f64", policy_split=0, rollout_fast=2),
     "times", "K9d-selector"),
    ("two_track_halves", dict(n_envs=65536, num_rays=16, track=MIXED), "inject", "K9"),
    ("two_track_halves_lit", dict(n_envs=65536, num_rays=16, track=MIXED, env_dtype="f64"), "inject", "K9-literal"),
    ("interleaved_deint", dict(n_envs=65536, num_rays=16, track=MIXED, track_interleave=True, policy_split=0, rollout_fast=1), "times", "K9"),
    ("interleaved_passes", dict(n_envs=65536, num_rays=16, track=MIXED, track_interleave=True, policy_split=0, rollout_fast=3), "times", "K9"),
    ("interleaved_lit", dict(n_envs=65536, num_rays=16, track=MIXED, track_interleave=True, env_dtype="f64", policy_split=0, rollout_fast=1),
     "times", "K9-literal"),
]


@pytest.mark.parametrize("kw,inject,kernel", [c[1:] for c in CAPTURE], ids=[c[0] for c in CAPTURE])
def test_capture_in_every_persistent_family(kw, inject, kernel):
    T = 12
    cap = _run(kw, "mega", "final_obs", inject, T)
    ref = _run(kw, "mega", "reference", inject, T)
    steps = _run(kw, "steps", "final_obs", inject, T)
    assert cap["mode"] == ref["mode"] == "mega" and steps["mode"] == "steps-eager"
    assert cap["kernel"] == ref["kernel"] == kernel, (cap["kernel"], ref["kernel"])
    # every other output: pc_rollout's bits
    for i, (a, b) in enumerate(zip(cap["snap"], ref["snap"])):
        assert torch.equal(a, b), f"buffer {i} differs from pc_rollout"
    for a, b in zip(cap["aux"], ref["aux"]):
        assert torch.equal(a, b)
    for k in ref["state"]:
        assert np.array_equal(cap["state"][k], ref["state"][k]), k
    for i, (a, b) in enumerate(zip(cap["snap"], steps["snap"])):
        assert torch.equal(a, b), f"buffer {i} differs from the per-step kernels"
    # the truncated (env, step) rows: K1's final_obs, bit for bit; every other row of the side buffer untouched (zero)
    tr = _truncations(cap["snap"])
    n_tr = int(tr.sum())
    assert n_tr > 0
    written = torch.zeros(cap["final_obs"].shape[:2], dtype=torch.bool, device="cuda")
    for t in range(T):
        written[t // LIMIT] |= tr[t]
    fo_c, fo_s = cap["final_obs"], steps["final_obs"]
    assert torch.equal(fo_c[written], fo_s[written])
    assert not bool((fo_c[~written] != 0).any())
    # the final observations are not the reset observations that the buffer rows hold (a car that has not moved yet has the same row)
    idx = torch.nonzero(tr[:-1])
    rows_fo, rows_buf = fo_c[idx[:, 0] // LIMIT, idx[:, 1]], cap["snap"][0][idx[:, 0] + 1, idx[:, 1]]
    assert bool((rows_fo != rows_buf).any(1).float().mean() > 0.5)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_capture_fills_slot_1_at_T_1005(dtype):
    T = 1005
    kw = dict(n_envs=4096, num_rays=16, track=TRACKS["big_track"], env_dtype=dtype, policy_split=1)
    cap = _run(kw, "mega", "final_obs", "t999", T, trained=True)
    steps = _run(kw, "steps", "final_obs", "t999", T, trained=True)
    assert cap["kernel"] == ("K9s" if dtype == "f32" else "K9s-literal")
    for i, (a, b) in enumerate(zip(cap["snap"], steps["snap"])):
        assert torch.equal(a, b), f"buffer {i}"
    tr = _truncations(cap["snap"])
    assert int(tr[0].sum()) == 4096 - int((cap["snap"][5][1] != 0).sum())     # every env that did not crash in step 0 truncated there
    in_slot1 = tr[LIMIT:].any(0)
    assert int(in_slot1.sum()) > 0, "no env reached the time limit a second time"
    w1 = in_slot1
    assert torch.equal(cap["final_obs"][1][w1], steps["final_obs"][1][w1])
    assert torch.equal(cap["final_obs"][0][tr[:LIMIT].any(0)], steps["final_obs"][0][tr[:LIMIT].any(0)])


# ---- 3. the value pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_envs", [4096, 65536])
def test_final_values_kernel_and_fp32(n_envs):
    kw = dict(n_envs=n_envs, num_rays=16, track=TRACKS["big_track"], rollout_kernel="mega", use_graphs=False, seed=43,
              truncation_bootstrap="final_obs")
    for bv in ("kernel", "fp32"):
        tr = Trainer(PPOConfig(n_steps=12, bootstrap_value=bv, **kw), device="cuda")
        _inject_times(tr, n_envs)
        tr.rollout()
        off, base = tr.agent._rng_offset, tr.rng_base.clone()
        fv = tr.final_values().clone()
        torch.cuda.synchronize()
        assert tr.agent._rng_offset == off and torch.equal(tr.rng_base, base)
        buf = tr.buffer
        tmask = _truncations(_snap(tr))
        w = tmask[:10].any(0)
        assert int(w.sum()) > n_envs // 2
        fo = buf.final_obs_buf[0]
        if bv == "kernel":
            # the rollout's own values: one fused policy call of N rows reproduces val_buf row for row ...
            v = torch.empty(n_envs, device="cuda")
            tr.agent.act(buf.obs_buf[3].contiguous(), out_value=v, fused=True, repack=False, offset=0)
            assert torch.equal(v, buf.val_buf[3])
            # ... and gives the final values' bits
            v2 = torch.empty(n_envs, device="cuda")
            tr.agent.act(fo.contiguous(), out_value=v2, fused=True, repack=False, offset=5)
            assert torch.equal(v2[w], fv[0][w])
            with torch.no_grad():
                ref = tr.agent.get_value(fo).view(-1)
            assert float((fv[0][w] - ref[w]).abs().max()) <= 4e-6
        else:
            with torch.no_grad():
                ref = tr.agent.get_value(fo).view(-1)
            assert torch.equal(fv[0][w], ref[w])
        tr.close()


# ---- 4. the Trainer's paths -------------------------------------------------------------------------------------------------------
def test_trainer_paths_agree_and_only_truncated_segments_change():
    N, T = 1024, 16
    res = {}
    for name, mode, graphs in (("mega", "mega", False), ("steps-graph", "steps", True), ("steps-eager", "steps", False)):
        cfg = PPOConfig(n_envs=N, n_steps=T, num_rays=16, track=TRACKS["big_track"], rollout_kernel=mode, use_graphs=graphs, seed=47,
                        batch_size=256, train_iters=2, bootstrap_value="fp32", truncation_bootstrap="final_obs", policy_split=1)
        tr = Trainer(cfg, device="cuda")
        st = tr.envs.get_state()
        st["time_step"] = 980 + np.arange(N) % 36       # truncations in both epochs
        tr.envs.set_state(**st)
        out = []
        for ep in range(2):
            tr.run_epoch()
            out.append((tr.buffer.adv_buf.clone(), tr.buffer.ret_buf.clone(), tr.rollout_mode))
        res[name] = (out, tr)
    assert [o[2] for o in res["mega"][0]] == ["mega", "mega"]
    assert [o[2] for o in res["steps-graph"][0]] == ["steps-eager", "steps-graph"]
    assert [o[2] for o in res["steps-eager"][0]] == ["steps-eager", "steps-eager"]
    for ep in range(2):
        for name in ("steps-graph", "steps-eager"):
            assert torch.equal(res["mega"][0][ep][0], res[name][0][ep][0]), (name, ep)
            assert torch.equal(res["mega"][0][ep][1], res[name][0][ep][1]), (name, ep)
    # against "reference" on the same rollout (the mega trainer's last buffers): only segments that end in a truncation differ
    tr = res["mega"][1]
    with torch.no_grad():
        lv = tr.agent.get_value(tr.next_obs).view(-1)
    # (the update has moved the parameters: recompute both from the same values)
    b = tr.buffer
    b.ptr = T
    a_fo, r_fo = b.calculate_advantages(lv, tr.next_term, tr.next_trunc, final_values=b.final_val_buf)
    a_fo, r_fo = a_fo.clone(), r_fo.clone()
    b.ptr = T
    a_ref, _ = b.calculate_advantages(lv, tr.next_term, tr.next_trunc)
    a_ref = a_ref.clone()
    done = torch.cat([(b.term_buf[1:] != 0) | (b.trunc_buf[1:] != 0), ((tr.next_term != 0) | (tr.next_trunc != 0))[None]], 0)
    tend = torch.cat([b.trunc_buf[1:] != 0, (tr.next_trunc != 0)[None]], 0)
    seg_trunc = torch.zeros_like(done)
    cur = torch.zeros(N, dtype=torch.bool, device="cuda")
    for t in reversed(range(T)):
        cur = torch.where(done[t], tend[t], cur)
        seg_trunc[t] = cur
    differ = a_fo != a_ref
    assert bool(differ.any())
    assert not bool((differ & ~seg_trunc).any())
    # float64 numpy GAE on the GPU's own rows
    cpu = lambda x: x.double().cpu().numpy()
    A64, R64 = gae_bootstrap_ref(cpu(b.rew_buf), cpu(b.val_buf), cpu(b.term_buf), cpu(b.trunc_buf), cpu(lv), cpu(tr.next_term),
                                 cpu(tr.next_trunc), cpu(b.final_val_buf), 0.99, 0.95)
    assert np.abs(cpu(a_fo) - A64).max() < 1e-5 and np.abs(cpu(r_fo) - R64).max() < 1e-5
    for _, t in res.values():
        t.close()


# ---- 5. train.py --------------------------------------------------------------------------------------------------------------------
def test_train_cli_truncation_bootstrap(tmp_path):
    import train
    out = str(tmp_path / "tb")
    train.main(["--run-name", "tb", "--n-epochs", "2", "--cuda", "--track", TRACKS["big_track"], "--n-envs", "256", "--n-steps", "64",
                "--batch-size", "64", "--train-iters", "2", "--num-rays", "16", "--out-dir", out, "--truncation-bootstrap", "final_obs",
                "--episode-stats"])
    lg = sorted(os.listdir(os.path.join(out, "logs")))
    rows = [json.loads(l) for l in open(os.path.join(out, "logs", lg[0], "scalars.jsonl"))]
    assert len(rows) == 2 and all(np.isfinite(r["losses/total_loss"]) and "charts/episodic_return" in r for r in rows)
    hp = open(os.path.join(out, "logs", lg[0], "hyperparameters.md")).read()
    assert "|truncation_bootstrap|final_obs|" in hp
