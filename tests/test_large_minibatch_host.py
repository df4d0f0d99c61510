"""The large-minibatch update (pc_ppo_adv_stats, pc_ppo_minibatch_large, PPOConfig.large_minibatch): the C-ABI surface and its argument
checks, the limits of the small path next to it, the config / CLI switches, and the CPU learner, which the flag must not change by a
bit.  No GPU needed: every check below runs before any device call (a non-NULL dummy address is never dereferenced)."""
import os
import re
import sys

import pytest
import torch

from ppo_car_amd import Agent, _capi
from ppo_car_amd.ppo import PPOConfig, PPOLearner
from conftest import ROOT

INV, UNS, NODEV = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_UNSUPPORTED, _capi.PC_ERR_NO_DEVICE
P = 4096      # a non-NULL address
MAXB = _capi.PC_PPO_LARGE_MAX_B
NEW = ("pc_ppo_large_workspace_floats", "pc_ppo_large_parts", "pc_ppo_adv_stats_workspace_doubles", "pc_ppo_adv_stats", "pc_ppo_minibatch_large")


def test_symbols_in_header_exports_and_library():
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    for name in NEW:
        assert re.search(r"\b(int|int64_t) " + name + r"\(", hdr), name
        assert name in _capi.EXPORTS
        assert getattr(_capi.lib, name) is not None
    m = re.search(r"#define PC_PPO_LARGE_MAX_B \(1 << (\d+)\)", hdr)
    assert m and (1 << int(m.group(1))) == MAXB == 1 << 20
    for word in ("summation order is fixed", "1024 < B <= PC_PPO_LARGE_MAX_B", "[parts][n_pad]"):
        assert word in hdr, word      # the header states the limits, the workspace layout and the fixed order


@pytest.mark.parametrize("kw", [dict(B=1024), dict(B=MAXB + 1), dict(H=128), dict(A=16), dict(D=41), dict(A=0), dict(D=0)])
def test_large_workspace_refuses_shapes_outside_its_limits(kw):
    a = dict(B=2056, D=23, H=256, A=9)
    a.update(kw)
    assert _capi.lib.pc_ppo_large_workspace_floats(0, a["B"], a["D"], a["H"], a["A"]) == UNS


def test_large_workspace_and_parts_need_a_device():
    """the grid depends on the device's compute units: a supported shape with device < 0 is 'no device', not a guess"""
    assert _capi.lib.pc_ppo_large_workspace_floats(-1, 2056, 23, 256, 9) == NODEV
    assert _capi.lib.pc_ppo_large_parts(-1, 2056) == NODEV
    assert _capi.lib.pc_ppo_large_parts(0, 1024) == UNS and _capi.lib.pc_ppo_large_parts(0, MAXB + 1) == UNS
    if not torch.cuda.is_available():
        assert _capi.lib.pc_ppo_large_workspace_floats(0, 2056, 23, 256, 9) == NODEV


def test_the_small_path_keeps_its_limits():
    assert _capi.lib.pc_ppo_workspace_floats(1025, 23, 256, 9) == UNS
    assert _capi.lib.pc_ppo_workspace_floats(1024, 23, 256, 9) > 0
    assert _capi.lib.pc_ppo_prepared_floats(1025, 23) == UNS
    assert _capi.lib.pc_ppo_minibatch(0, P, 1025, 23, 256, 9, *(P,) * 5, P, P, *(P,) * 4, 0.2, 0.5, 0.001, 1.0, 0.9, 0.999, 1e-5, P, P, 1,
                                      None) == UNS


def _mb(device=0, idx=P, data=(P,) * 5, stats=P, param=P, grad=P, state=(P,) * 4, metrics=P, ws=P, apply=1, B=2056, D=23, H=256, A=9):
    return _capi.lib.pc_ppo_minibatch_large(device, idx, B, D, H, A, *data, stats, param, grad, *state, 0.2, 0.5, 0.001, 1.0, 0.9, 0.999, 1e-5,
                                            metrics, ws, apply, None)


@pytest.mark.parametrize("kw", [dict(idx=None), dict(stats=None), dict(param=None), dict(grad=None), dict(metrics=None), dict(ws=None),
                                dict(data=(None, P, P, P, P)), dict(data=(P, None, P, P, P)), dict(data=(P, P, P, P, None)),
                                dict(state=(None, P, P, P)), dict(state=(P, None, P, P)), dict(state=(P, P, None, P)),
                                dict(state=(P, P, P, None)), dict(apply=2, state=(P, P, None, P)), dict(apply=3), dict(apply=-1)])
def test_minibatch_large_argument_checks(kw):
    assert _mb(**kw) == INV


def test_minibatch_large_check_order_and_shapes():
    """pc_ppo_minibatch's order: NULL / apply checks, then the shape, then the device"""
    for kw in (dict(B=1024), dict(B=MAXB + 1), dict(H=128), dict(A=16), dict(D=41)):
        assert _mb(**kw) == UNS, kw
        assert _mb(device=-1, **kw) == UNS, kw
        assert _mb(param=None, **kw) == INV, kw
    assert _mb(device=-1) == NODEV
    assert _mb(device=-1, apply=0, state=(None,) * 4) == NODEV      # apply == 0 needs no optimizer state
    assert _mb(device=-1, apply=2, state=(None, None, P, None)) == NODEV


def _st(device=0, idx=P, ld=2056, n_mb=3, B=2056, adv=P, stats=P, ws=P):
    return _capi.lib.pc_ppo_adv_stats(device, idx, ld, n_mb, B, adv, stats, ws, None)


@pytest.mark.parametrize("kw", [dict(idx=None), dict(adv=None), dict(stats=None), dict(ws=None), dict(n_mb=0), dict(n_mb=-1), dict(n_mb=65536),
                                dict(ld=2055)])
def test_adv_stats_argument_checks(kw):
    assert _st(**kw) == INV


def test_adv_stats_shapes_device_and_workspace():
    assert _st(B=1024, ld=1024) == UNS and _st(B=MAXB + 1, ld=MAXB + 1) == UNS
    assert _st(device=-1) == NODEV
    ws = _capi.lib.pc_ppo_adv_stats_workspace_doubles
    assert ws(0, 2056) == INV and ws(3, 1024) == UNS and ws(3, MAXB + 1) == UNS
    assert ws(1, 1025) >= 2 and ws(3, 4099) == 3 * ws(1, 4099) and ws(1, MAXB) >= ws(1, 65536) >= ws(1, 1025)


@pytest.mark.parametrize("kw,word", [(dict(update_diagnostics=True), "update_diagnostics"), (dict(target_kl=0.02), "target_kl"),
                                     (dict(deferred_adam=True), "deferred_adam"), (dict(full_sweep=True), "full_sweep")])
def test_config_refuses_the_combinations_the_large_path_does_not_have(kw, word):
    with pytest.raises(ValueError, match=word):
        PPOConfig(batch_size=2056, large_minibatch=True, **kw)
    PPOConfig(batch_size=2056, **kw)                          # (the flag is what is refused, not the option)


def test_config_accepts_the_flag_where_it_changes_nothing():
    assert PPOConfig().large_minibatch is False
    assert PPOConfig(large_minibatch=True, batch_size=512).large_minibatch is True
    PPOConfig(large_minibatch=True, batch_size=512, update_diagnostics=True)
    PPOConfig(large_minibatch=True, batch_size=1024, full_sweep=True)
    assert PPOConfig(large_minibatch=True, batch_size=2056).large_minibatch is True


def test_train_cli_accepts_the_flag():
    sys.path.insert(0, ROOT)
    import train
    assert train.parse_args(["--run-name", "x", "--batch-size", "4096", "--large-minibatch"]).large_minibatch is True
    assert train.parse_args(["--run-name", "x"]).large_minibatch is False


@pytest.mark.parametrize("kw", [dict(), dict(fused_update=False), dict(custom_mlp=False), dict(use_graphs=False), dict(prepared_minibatches=False),
                                dict(deferred_adam=True), dict(force_collective=True), dict(full_sweep=True), dict(update_diagnostics=True),
                                dict(target_kl=0.02), dict(target_kl=0.02, custom_mlp=False), dict(large_minibatch=True),
                                dict(large_minibatch=True, batch_size=2056), dict(batch_size=2056)])
def test_cpu_learner_plan_is_the_torch_path_with_the_legacy_attributes(kw):
    """The update plan PPOLearner decides once (path, prepared, chained) and the attributes it is read through elsewhere: on the CPU
    every configuration is the torch path, none of the kernel paths' attributes is set, and diag_on follows target_kl."""
    cfg = PPOConfig(n_envs=4, n_steps=64, train_iters=1, **kw)
    L = PPOLearner(Agent(18, 9), cfg, "cpu")
    assert L.path == "torch" and not L.prepared and not L.chained
    assert L.fused is False and L.custom is False and L.large is False and L.flat_adam is False and L.graphs is False
    assert L.diag_on == (cfg.target_kl is not None or bool(kw.get("update_diagnostics")))
    assert (L.diag is not None) == L.diag_on
    assert L.collective == bool(kw.get("force_collective"))
    assert isinstance(L.optimizer, torch.optim.Adam) and not hasattr(L, "exp_avg")


def test_cpu_learner_is_the_torch_path_bit_for_bit():
    """On the CPU there are no kernels to take: the flag leaves the torch-op step exactly as it is (parameters, optimizer state,
    metrics, index draws)."""
    M, D = 4200, 18
    g = torch.Generator().manual_seed(3)
    obs = torch.rand(M, D, generator=g) * 2.6 - 1.0
    act = torch.randint(0, 9, (M,), generator=g).float()
    lp = -2.2 + 0.3 * torch.randn(M, generator=g)
    adv = 3.0 + 0.5 * torch.randn(M, generator=g)
    ret = torch.randn(M, generator=g)
    out = []
    for flag in (False, True):
        torch.manual_seed(11)
        agent = Agent(D, 9)
        L = PPOLearner(agent, PPOConfig(n_envs=4, n_steps=1050, batch_size=2056, train_iters=2, seed=5, large_minibatch=flag), "cpu")
        assert not L.large and not L.fused and not L.custom and not L.flat_adam
        L.update(obs, act, lp, adv, ret)
        L.update(obs, act, lp, adv, ret)
        st = L.optimizer.state_dict()["state"]
        out.append([L.flat_param.clone(), L.flat_grad.clone(), L.metrics.clone(), torch.tensor(L.current_lr())]
                   + [st[k][n].clone() for k in sorted(st) for n in ("exp_avg", "exp_avg_sq")])
    assert len(out[0]) == len(out[1]) > 4
    for a, b in zip(*out):
        assert torch.equal(a, b)
    torch.manual_seed(11)
    assert not torch.equal(out[0][0], torch.cat([p.detach().reshape(-1) for p in Agent(D, 9).parameters()]))      # (the updates did step)
