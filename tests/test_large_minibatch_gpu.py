"""The large-minibatch update on the GPU: pc_ppo_adv_stats (KLs) and pc_ppo_minibatch_large (K10L + K11 + K12) through the C-ABI against
the float64 restatement of the step (ppo.ppo_loss on a .double() copy of the agent, clip_grad_norm_, torch.optim.Adam(lr 3e-4, eps 1e-5),
computed on the CPU here), and PPOConfig.large_minibatch end to end against the torch-op step.  The bars are tests/test_ppo_golden.py's.

Inputs of every kernel-level case: a pool of 8192 samples, indices drawn without replacement, Agent(D, A) at its seeded initial weights,
obs uniform in [-1, 1.6], old log-probs = the agent's own + 0.3 N(0, 1) (about half the samples on each side of the clip),
adv = 3 + 0.5 N(0, 1), ret = N(0, 1)."""
import functools

import numpy as np
import pytest
import torch

from ppo_car_amd import Agent, _capi
from ppo_car_amd._capi import check, lib
from ppo_car_amd.ppo import PPOConfig, Trainer, ppo_loss
from conftest import TRACKS

pytestmark = pytest.mark.gpu

POOL = 8192
CLIP, VF, EC, LR = 0.2, 0.5, 0.001, 3e-4
SHAPES = [(23, 9, 1025), (18, 9, 2056), (39, 9, 4099), (7, 3, 1031)]     # (D, A, B): a last group of one sample | one workgroup walks two
NORMS = [1e9, 0.05]                                                       # groups at 256 compute units | primes | the generic kernels


def _flat(agent):
    return torch.cat([p.detach().reshape(-1) for p in agent.parameters()])


@functools.lru_cache(maxsize=None)
def _case(D, A, B):
    """The inputs and the float64 reference of one shape, computed once and shared (read-only) by every test that needs it."""
    torch.manual_seed(1000 + B)
    agent = Agent(D, A)
    g = torch.Generator().manual_seed(B)
    obs = torch.rand(POOL, D, generator=g) * 2.6 - 1.0
    act = torch.randint(0, A, (POOL,), generator=g).float()
    with torch.no_grad():
        own = torch.log_softmax(agent.actor(obs), -1).gather(1, act.long().view(-1, 1)).view(-1)
    old_lp = own + 0.3 * torch.randn(POOL, generator=g)
    adv = 3.0 + 0.5 * torch.randn(POOL, generator=g)
    ret = torch.randn(POOL, generator=g)
    idx = torch.randperm(POOL, generator=g)[:B].contiguous()
    ref = {}
    for max_norm in NORMS:
        a64 = Agent(D, A).double()
        a64.load_state_dict({k: v.double() for k, v in agent.state_dict().items()})
        opt = torch.optim.Adam(a64.parameters(), lr=LR, eps=1e-5)
        loss, pl, vl, en = ppo_loss(a64, obs[idx].double(), act[idx].double(), old_lp[idx].double(), adv[idx].double(), ret[idx].double(),
                                    CLIP, VF, EC)
        loss.backward()
        norm = float(torch.nn.utils.clip_grad_norm_(a64.parameters(), max_norm))
        grad = torch.cat([p.grad.reshape(-1) for p in a64.parameters()]).numpy().copy()
        opt.step()
        ref[max_norm] = dict(metrics=[float(pl), float(vl), float(en), float(loss)], grad=grad, norm=norm, param=_flat(a64).numpy().copy())
    ratio = torch.exp(own - old_lp)[idx]
    assert float((ratio < 0.8).float().mean()) > 0.1 and float((ratio > 1.2).float().mean()) > 0.1      # both sides of the clip
    assert ref[0.05]["norm"] > 0.05                                                                    # ... and the norm clip bites
    return dict(D=D, A=A, B=B, p0=_flat(agent).clone(), obs=obs, act=act, old_lp=old_lp, adv=adv, ret=ret, idx=idx, ref=ref)


def _adv_stats(idx2d, B, adv):
    """pc_ppo_adv_stats on idx2d [n_mb][B] (device) -> [n_mb][2] float32 (device)"""
    n_mb = idx2d.shape[0]
    stats = torch.full((n_mb, 2), float("nan"), device="cuda")
    ws = torch.full((lib.pc_ppo_adv_stats_workspace_doubles(n_mb, B),), float("nan"), device="cuda", dtype=torch.float64)
    check(lib.pc_ppo_adv_stats(0, idx2d.data_ptr(), idx2d.stride(0), n_mb, B, adv.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), "pc_ppo_adv_stats")
    return stats


def _step(c, max_norm, apply=1, ws_fill=0.0, state=None):
    """One pc_ppo_minibatch_large call on case c from its initial parameters (or `state`); everything it writes, on the host."""
    D, A, B = c["D"], c["A"], c["B"]
    dv = {k: c[k].cuda().contiguous() for k in ("obs", "act", "old_lp", "adv", "ret", "idx")}
    n_ws = lib.pc_ppo_large_workspace_floats(0, B, D, 256, A)
    assert n_ws > 0
    ws = torch.full((n_ws,), ws_fill, device="cuda")
    param = c["p0"].cuda().clone()
    z = lambda: torch.zeros_like(param)
    grad, m, v = torch.full_like(param, 7.0), z(), z()
    step, lr, metrics = torch.zeros(1, device="cuda"), torch.full((1,), LR, device="cuda"), torch.zeros(4, device="cuda")
    if state is not None:
        for t, s in zip((param, m, v, step), state):
            t.copy_(s)
    stats = _adv_stats(dv["idx"].view(1, B), B, dv["adv"])
    st = torch.cuda.current_stream().cuda_stream
    check(lib.pc_ppo_minibatch_large(0, dv["idx"].data_ptr(), B, D, 256, A, dv["obs"].data_ptr(), dv["act"].data_ptr(), dv["old_lp"].data_ptr(),
                                     dv["adv"].data_ptr(), dv["ret"].data_ptr(), stats.data_ptr(), param.data_ptr(), grad.data_ptr(),
                                     m.data_ptr(), v.data_ptr(), step.data_ptr(), lr.data_ptr(), CLIP, VF, EC, max_norm, 0.9, 0.999, 1e-5,
                                     metrics.data_ptr(), ws.data_ptr(), apply, st), "pc_ppo_minibatch_large")
    torch.cuda.synchronize()
    return dict(param=param, grad=grad, m=m, v=v, step=step, lr=lr, metrics=metrics)


def _hold_to_reference(c, max_norm):
    r = c["ref"][max_norm]
    out = _step(c, max_norm)
    got = out["metrics"].cpu().numpy()
    print(f"D {c['D']} A {c['A']} B {c['B']} max_norm {max_norm}: metrics {got} ref {r['metrics']}")
    gref = r["grad"]                                         # (clip_grad_norm_ has scaled it in place)
    g = out["grad"].cpu().numpy().astype(np.float64)
    print(f"  gradient: max abs err {np.abs(g - gref).max():.3e}, max err / (2e-7 + 2e-4 |ref|) {(np.abs(g - gref) / (2e-7 + 2e-4 * np.abs(gref))).max():.3f}")
    p = out["param"].cpu().numpy().astype(np.float64)
    print(f"  parameters: max abs err {np.abs(p - r['param']).max():.3e}")
    for a, b, key in zip(got, r["metrics"], ("policy_loss", "value_loss", "entropy", "loss")):
        assert float(a) == pytest.approx(b, rel=1e-5, abs=1e-6), key
    assert np.allclose(g, gref, rtol=2e-4, atol=2e-7)
    assert np.abs(p - r["param"]).max() <= 3e-6
    assert np.abs(r["param"] - c["p0"].numpy()).max() > 1e-4          # (the step is visible at that tolerance)
    assert float(out["step"]) == 1.0


@pytest.mark.parametrize("max_norm", NORMS)
@pytest.mark.parametrize("D,A,B", SHAPES)
def test_one_step_against_float64(D, A, B, max_norm):
    assert lib.pc_ppo_large_workspace_floats(0, B, D, 256, A) > 0
    _hold_to_reference(_case(D, A, B), max_norm)


@pytest.mark.parametrize("max_norm", NORMS)
@pytest.mark.parametrize("which", [0, 1])
def test_one_step_at_the_grid_cap(which, max_norm):
    """cap = the most workgroups the step launches on this device: 8 (cap + 1) samples give exactly one workgroup a second group,
    8 cap + 1 a second group of one sample."""
    cap = lib.pc_ppo_large_parts(0, _capi.PC_PPO_LARGE_MAX_B)
    assert 128 < cap <= 1024
    B = (8 * (cap + 1), 8 * cap + 1)[which]
    assert lib.pc_ppo_large_parts(0, B) == cap and lib.pc_ppo_large_parts(0, 1025) == min(129, cap)
    _hold_to_reference(_case(23, 9, B), max_norm)


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("n_mb,B,pool", [(3, 1025, POOL), (3, 4099, 3 * 4099), (1, 65536, 1 << 17)])
def test_advantage_statistics(n_mb, B, pool):
    """mean 100 x the std: (mean, unbiased std) within one float32 ulp of float64 numpy rounded to float32 (float64 accumulation of at
    most 2^20 float32 values loses nothing a float32 sees); a constant advantage gives exactly the floor 1e-5f."""
    g = torch.Generator().manual_seed(B)
    adv = (100.0 + torch.randn(pool, generator=g)).float()
    idx = torch.stack([torch.randperm(pool, generator=g)[:B] for _ in range(n_mb)]).contiguous()
    stats = _adv_stats(idx.cuda(), B, adv.cuda()).cpu().numpy()
    for m in range(n_mb):
        x = adv.numpy()[idx[m].numpy()].astype(np.float64)
        mean, sd = np.float32(x.mean()), np.float32(x.std(ddof=1))
        print(f"B {B} minibatch {m}: mean {stats[m, 0]!r} ref {mean!r}, std {stats[m, 1]!r} ref {sd!r}")
        assert _ulps(stats[m, 0], mean) <= 1 and _ulps(stats[m, 1], sd) <= 1
    const = _adv_stats(idx.cuda(), B, torch.full((pool,), 2.5, device="cuda")).cpu().numpy()
    assert (const[:, 0] == np.float32(2.5)).all() and (const[:, 1] == np.float32(1e-5)).all()


def test_apply_contract():
    """apply = 0: the gradient and nothing else.  apply = 2 + pc_clip_adam_advanced = apply = 1, bit for bit where the clip coefficient
    is exactly 1 (max_grad_norm above the norm): the two clip + Adam kernels are the existing ones and sum the squared norm in different
    orders (K12 from K11's per-block partials, pc_clip_adam_advanced over the bucket), so with a biting clip their coefficients may
    differ in the last bit -- there the two routes are held to each other at 1e-6, the bar tests/test_cli_and_surface_gpu.py sets for
    the same pair of kernels."""
    c = _case(18, 9, 2056)
    st = torch.cuda.current_stream().cuda_stream
    for max_norm in NORMS:
        only = _step(c, max_norm, apply=0)
        assert torch.equal(only["param"].cpu(), c["p0"]) and float(only["step"]) == 0.0
        assert not only["m"].any() and not only["v"].any()
        one = _step(c, max_norm, apply=1)
        two = _step(c, max_norm, apply=2)
        assert float(two["step"]) == 1.0 and torch.equal(two["param"].cpu(), c["p0"]) and not two["m"].any() and not two["v"].any()
        # apply = 0 and 2 leave the raw gradient; apply = 1 has clipped it in place
        assert torch.equal(only["grad"], two["grad"]) and torch.equal(only["metrics"], two["metrics"])
        assert float(only["grad"].double().norm()) == pytest.approx(c["ref"][max_norm]["norm"], rel=1e-5)
        check(lib.pc_clip_adam_advanced(0, two["param"].data_ptr(), two["grad"].data_ptr(), two["m"].data_ptr(), two["v"].data_ptr(),
                                        two["step"].data_ptr(), two["lr"].data_ptr(), two["param"].numel(), max_norm, 1.0, 0.9, 0.999, 1e-5,
                                        st), "pc_clip_adam_advanced")
        torch.cuda.synchronize()
        for k in ("param", "m", "v", "step", "metrics"):
            if max_norm > 1.0:
                assert torch.equal(one[k], two[k]), k
            else:
                assert torch.allclose(one[k], two[k], atol=2e-6, rtol=1e-5), k


@pytest.mark.parametrize("D,A,B", [(23, 9, 1025), (39, 9, 4099), (7, 3, 1031)])
def test_determinism_and_workspace_padding(D, A, B):
    """the same call twice into fresh buffers: the same bits; a workspace full of NaN: the same bits again (nothing is read that the
    step has not written)"""
    c = _case(D, A, B)
    a, b, n = _step(c, 1.0), _step(c, 1.0), _step(c, 1.0, ws_fill=float("nan"))
    for k in ("grad", "metrics", "param", "m", "v"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], n[k]), k
    assert bool(torch.isfinite(n["param"]).all())


# ---- the trainer, end to end -------------------------------------------------------------------------------------------
def _cfg(**kw):
    return PPOConfig(n_envs=256, n_steps=16, batch_size=2056, train_iters=2, track=TRACKS["big_track"], num_rays=16, seed=5, **kw)


BUFS = ("obs_buf", "act_buf", "rew_buf", "val_buf", "term_buf", "trunc_buf", "logprob_buf")


def _epoch(cfg):
    tr = Trainer(cfg, device="cuda:0")
    s = tr.run_epoch()
    L = tr.learner
    out = dict(bufs=[getattr(tr.buffer, k).clone() for k in BUFS], param=L.flat_param.clone(), scalars=s, large=L.large,
               step=float(L.step_count) if L.flat_adam else None, captured=L._epoch_graph is not None,
               state=[t.clone() for t in (L.flat_param, L.exp_avg, L.exp_avg_sq, L.step_count, L.lr_dev, L.metrics)] if L.flat_adam else None)
    tr.close()
    return out


@functools.lru_cache(maxsize=None)
def _torch_epoch():
    return _epoch(_cfg(large_minibatch=True, fused_update=False))


@functools.lru_cache(maxsize=None)
def _graph_epoch():
    return _epoch(_cfg(large_minibatch=True))


LOSSES = ("losses/policy_loss", "losses/value_loss", "losses/entropy", "losses/total_loss")


def _hold_to_torch_epoch(got):
    ref = _torch_epoch()
    assert not ref["large"] and got["large"]
    for a, b, k in zip(got["bufs"], ref["bufs"], BUFS):
        assert torch.equal(a, b), k
    print("parameters: max abs difference", float((got["param"] - ref["param"]).abs().max()))
    assert float((got["param"] - ref["param"]).abs().max()) <= 2 * 3e-6            # two applied steps at the per-step bar
    for k in LOSSES:
        print(k, got["scalars"][k], ref["scalars"][k])
        assert got["scalars"][k] == pytest.approx(ref["scalars"][k], rel=1e-5, abs=1e-6), k
    assert got["step"] == 2.0


def test_trainer_epoch_in_one_graph():
    got = _graph_epoch()
    assert got["captured"]
    _hold_to_torch_epoch(got)


def test_trainer_epoch_eager_equals_the_graph():
    got = _epoch(_cfg(large_minibatch=True, use_graphs=False))
    assert not got["captured"]
    _hold_to_torch_epoch(got)
    for a, b in zip(got["state"], _graph_epoch()["state"]):
        assert torch.equal(a, b)


def test_trainer_epoch_with_an_exchange_step():
    """force_collective: apply = 2, the all-reduce (one rank: the identity) and pc_clip_adam_advanced per minibatch"""
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        got = _epoch(_cfg(large_minibatch=True, force_collective=True))
    finally:
        dist.destroy_process_group()
    _hold_to_torch_epoch(got)


def test_resume_continues_bit_for_bit():
    """two epochs in one run = one epoch, a checkpoint through state_dict / load_state_dict into a fresh trainer, one more epoch"""
    a = Trainer(_cfg(large_minibatch=True), device="cuda:0")
    a.run_epoch()
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.state_dict().items()}
    sd["opt"] = {k: v.clone() for k, v in sd["opt"].items()}
    sd["agent"] = {k: v.clone() for k, v in sd["agent"].items()}
    a.run_epoch()
    b = Trainer(_cfg(large_minibatch=True), device="cuda:0")
    assert b.learner.large and sd["fused"] is True
    b.load_state_dict(sd)
    b.run_epoch()
    for k in ("flat_param", "exp_avg", "exp_avg_sq", "step_count", "lr_dev", "metrics"):
        assert torch.equal(getattr(a.learner, k), getattr(b.learner, k)), k
    assert float(a.learner.step_count) == 4.0
    a.close()
    b.close()
