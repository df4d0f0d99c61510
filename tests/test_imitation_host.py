"""Imitation (ppo_car_amd.imitation, pc_bc_minibatch, distill.py) as far as it goes without a GPU: bc_loss against torch's own
cross-entropy in float64, BCLearner on the CPU (the torch path), the per-env teacher assignment, the argument checks of
pc_bc_minibatch that run before any device call (a non-NULL dummy address is never dereferenced), and the CLI's parser."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ppo_car_amd import Agent, BCLearner, _capi, bc_loss, teacher_envs
from conftest import ROOT

INV, UNS = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_UNSUPPORTED
P = 4096      # a non-NULL address


def _data(B=48, D=18, A=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    obs = (torch.rand(B, D, generator=g, dtype=torch.float64) * 2.6 - 1.0)
    label = torch.randint(-1, A, (B,), generator=g).to(torch.float64)
    label[:6] = torch.tensor([-1.0, 0.0, A - 1.0, A, A + 3.0, -1.0], dtype=torch.float64)      # the edges, and three kinds of "no label"
    target = torch.randn(B, generator=g, dtype=torch.float64)
    return obs, label, target


def test_symbol_in_header_exports_and_library():
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    assert re.search(r"\bint pc_bc_minibatch\(", hdr)
    assert "pc_bc_minibatch" in _capi.EXPORTS and _capi.lib.pc_bc_minibatch is not None
    for word in ("The divisor is always B", "no label", "target == NULL needs vf_coef == 0"):
        assert word in hdr, word


def test_bc_loss_is_cross_entropy_with_ignored_labels_in_float64():
    torch.manual_seed(1)
    A, vf, ec = 9, 0.5, 0.01
    agent = Agent(18, A).double()
    obs, label, target = _data(A=A)
    B = obs.shape[0]
    with torch.no_grad():
        return _check_bc_loss(agent, obs, label, target, vf, ec, A, B)


def _check_bc_loss(agent, obs, label, target, vf, ec, A, B):
    total, ce, vl, ent = bc_loss(agent, obs, label, target, vf, ec)
    logits, v = agent.actor(obs), agent.critic(obs).view(-1)
    mapped = torch.where((label >= 0) & (label < A), label, torch.full_like(label, -1.0)).long()
    assert (mapped[:6] == torch.tensor([-1, 0, A - 1, -1, -1, -1])).all()
    ce_ref = F.cross_entropy(logits, mapped, ignore_index=-1, reduction="sum") / B
    p = torch.softmax(logits, -1)
    ent_ref = (-(p * torch.log(p)).sum(-1) * (mapped >= 0)).sum() / B
    vl_ref = (0.5 * (v - target) ** 2).sum() / B
    for got, ref in ((ce, ce_ref), (ent, ent_ref), (vl, vl_ref), (total, ce_ref + vf * vl_ref - ec * ent_ref)):
        assert abs(float(got) - float(ref)) <= 1e-12, (float(got), float(ref))
    # float32 labels (act_buf's layout) and integer labels give the same loss
    assert float(bc_loss(agent, obs, label.long(), target, vf, ec)[0]) == float(total)
    assert float(bc_loss(agent, obs, label.float(), target, vf, ec)[0]) == float(total)
    # no targets: no value term
    t0, _, vl0, _ = bc_loss(agent, obs, label, None, 0.0, ec)
    assert float(vl0) == 0.0 and abs(float(t0) - float(ce_ref - ec * ent_ref)) <= 1e-12


def test_bc_loss_all_ignored_is_zero_with_zero_gradients():
    torch.manual_seed(2)
    agent = Agent(18, 9).double()
    obs, label, _ = _data()
    label = torch.where(torch.arange(label.numel()) % 3 == 0, torch.full_like(label, 9.0), torch.full_like(label, -1.0))
    total, ce, vl, ent = bc_loss(agent, obs, label, None, 0.0, 0.01)
    assert all(float(x.detach()) == 0.0 for x in (total, ce, vl, ent))
    total.backward()
    for p in agent.parameters():
        assert p.grad is None or not p.grad.any()


def _fixed_set(M=64, D=18, A=9):
    g = torch.Generator().manual_seed(7)
    obs = torch.rand(M, D, generator=g) * 2.6 - 1.0
    label = torch.randint(0, A, (M,), generator=g).float()
    label[::9] = -1.0
    return obs, label


def test_cpu_learner_learns_and_leaves_the_critic_alone():
    torch.manual_seed(3)
    agent = Agent(18, 9)
    critic0 = [p.detach().clone() for p in agent.critic.parameters()]
    actor0 = [p.detach().clone() for p in agent.actor.parameters()]
    L = BCLearner(agent, batch_size=32, seed=4, device="cpu")
    assert L.path == "torch" and isinstance(L.optimizer, torch.optim.Adam)
    obs, label = _fixed_set()
    agent._image_ok = True
    rows = [L.fit(obs, label, epochs=1) for _ in range(20)]
    assert agent._image_ok is False
    assert set(rows[0]) == {"bc/ce", "bc/value_loss", "bc/entropy", "bc/loss", "bc/steps"} and rows[0]["bc/steps"] == 2 and L.steps == 40
    assert rows[-1]["bc/ce"] < rows[0]["bc/ce"]
    assert all(r["bc/value_loss"] == 0.0 for r in rows)
    for p, q in zip(agent.critic.parameters(), critic0):
        assert torch.equal(p.detach(), q)
    assert any(not torch.equal(p.detach(), q) for p, q in zip(agent.actor.parameters(), actor0))
    with pytest.raises(ValueError, match="no full minibatch"):
        L.fit(obs[:31], label[:31])


def test_cpu_learner_is_deterministic_and_restores_its_state():
    obs, label = _fixed_set()
    target = obs[:, 0].clone()

    def run(split):
        torch.manual_seed(5)
        agent = Agent(18, 9)
        L = BCLearner(agent, batch_size=32, vf_coef=0.5, ent_coef=0.01, seed=9, device="cpu")
        L.fit(obs, label, target, epochs=2)
        if split:
            sd = L.state_dict()
            torch.manual_seed(6)
            agent = Agent(18, 9)
            L = BCLearner(agent, batch_size=32, vf_coef=0.5, ent_coef=0.01, seed=1, device="cpu")
            L.load_state_dict(sd)
        out = L.fit(obs, label, target, epochs=2)
        return L.flat_param.clone(), out

    (a, oa), (b, ob) = run(False), run(True)
    assert torch.equal(a, b) and oa == ob and oa["bc/value_loss"] > 0.0


def test_learner_refusals():
    agent = Agent(18, 9)
    with pytest.raises(ValueError, match="batch_size"):
        BCLearner(agent, batch_size=0, device="cpu")
    with pytest.raises(ValueError, match=">= 0"):
        BCLearner(agent, ent_coef=-0.1, device="cpu")
    with pytest.raises(ValueError, match=">= 0"):
        BCLearner(agent, vf_coef=-1.0, device="cpu")
    L = BCLearner(agent, batch_size=32, vf_coef=0.5, device="cpu")
    obs, label = _fixed_set()
    with pytest.raises(ValueError, match="targets"):
        L.fit(obs, label)
    with pytest.raises(ValueError, match="targets"):
        L.step(torch.arange(32), obs, label)


@pytest.mark.parametrize("n", [1, 7, 64, 1000])
def test_teacher_share_is_exact_and_nested(n):
    sets = []
    for beta in (0.0, 0.3, 0.5, 1.0):
        m = teacher_envs(n, beta)
        assert m.dtype == np.bool_ and m.shape == (n,) and int(m.sum()) == round(beta * n), (n, beta)
        assert np.array_equal(m, teacher_envs(n, beta))      # a pure function
        sets.append(m)
    for small, large in zip(sets, sets[1:]):
        assert not (small & ~large).any()
    assert not sets[0].any() and sets[-1].all()
    with pytest.raises(ValueError):
        teacher_envs(n, 1.5)


def _bc(device=0, idx=P, B=64, D=23, H=256, A=9, obs=P, label=P, target=P, param=P, grad=P, state=(P,) * 4, vf=0.5, metrics=P, ws=P, apply=1):
    return _capi.lib.pc_bc_minibatch(device, idx, B, D, H, A, obs, label, target, param, grad, *state, vf, 0.01, 0.5, 0.9, 0.999, 1e-5, metrics, ws,
                                     apply, None)


@pytest.mark.parametrize("kw", [dict(obs=None), dict(label=None), dict(param=None), dict(ws=None), dict(idx=None), dict(grad=None),
                                dict(metrics=None), dict(target=None, vf=0.5), dict(apply=3), dict(apply=-1), dict(state=(None, P, P, P)),
                                dict(apply=2, state=(P, P, None, P))])
def test_bc_minibatch_argument_checks(kw):
    assert _bc(**kw) == INV
    assert _bc(device=-1, **kw) == INV      # (before any device call)


@pytest.mark.parametrize("kw", [dict(B=1), dict(B=1025), dict(H=128), dict(A=16), dict(D=41)])
def test_bc_minibatch_shape_limits_come_before_the_device(kw):
    assert _bc(**kw) == UNS
    assert _bc(device=-1, **kw) == UNS
    assert _bc(target=None, vf=0.0, **kw) == UNS      # no targets and no value term: a valid call as far as the arguments go
    assert _bc(param=None, **kw) == INV               # pc_ppo_minibatch's order: NULL / apply checks first


def test_bc_minibatch_without_a_device():
    assert _bc(device=-1) == _capi.PC_ERR_NO_DEVICE
    assert _bc(device=-1, target=None, vf=0.0, apply=0, state=(None,) * 4) == _capi.PC_ERR_NO_DEVICE


def _distill():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import distill
    return distill


def test_distill_cli_parses_and_refuses(capsys):
    distill = _distill()
    with pytest.raises(SystemExit) as ex:
        distill.parse_args(["--help"])
    assert ex.value.code == 0 and "--teacher-checkpoint" in capsys.readouterr().out
    cem = ["--out", "o.dat", "--planner", "cem", "--plan-iterations", "4", "--plan-elites", "8"]
    a = distill.parse_args(cem + ["--plan-horizon", "8", "--plan-candidates", "64", "--rounds", "8", "--steps-per-round", "250"])
    assert (a.plan_horizon, a.plan_candidates, a.plan_iterations, a.plan_elites, a.rounds, a.steps_per_round) == (8, 64, 4, 8, 8, 250)
    assert a.checkpoint is None and a.num_rays == 16 and a.envs == 1024
    with pytest.raises(SystemExit) as ex:
        distill.parse_args(cem + ["--plan-bootstrap", "running"])
    assert ex.value.code == 2 and "--teacher-checkpoint" in capsys.readouterr().err
    a = distill.parse_args(cem + ["--plan-bootstrap", "running", "--plan-gamma", "0.99", "--teacher-checkpoint", "m.dat"])
    assert a.plan_bootstrap == "running" and a.plan_gamma == 0.99
    with pytest.raises(SystemExit):      # evaluate.py's rule: cem names both options of the budget's split, shooting neither
        distill.parse_args(["--out", "o.dat", "--planner", "cem", "--plan-iterations", "4"])
    with pytest.raises(SystemExit):
        distill.parse_args(["--out", "o.dat", "--planner", "shooting", "--plan-elites", "4"])
    with pytest.raises(SystemExit):
        distill.parse_args(cem[2:])      # --out is required
