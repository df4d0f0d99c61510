"""Soft imitation targets without a GPU: PlannerDistiller's labels / label_temperature validation, the planners' temperature check,
distill.py's flags, BCLearner's routing of a 2-D label on the torch path, and -- on the constructor's argument handling, with the env
and planner construction stubbed -- that labels="best" asks the planner for no action values and allocates no soft buffer while
labels="soft" asks for both."""
import sys

import pytest
import torch

import ppo_car_amd as pc
from ppo_car_amd import Agent, BCLearner, bc_soft_loss
from ppo_car_amd import imitation, planner
from conftest import ROOT

sys.path.insert(0, ROOT)
import distill  # noqa: E402


@pytest.mark.parametrize("kw,match", [(dict(labels="hard"), "labels"), (dict(labels="soft", label_temperature=-0.1), "label_temperature"),
                                      (dict(labels="soft", label_temperature=float("nan")), "label_temperature"),
                                      (dict(labels="soft", label_temperature=float("inf")), "label_temperature"),
                                      (dict(labels="best", label_temperature=0.5), "label_temperature")])
def test_distiller_refuses(kw, match):
    with pytest.raises(ValueError, match=match):      # (before anything touches a device)
        pc.PlannerDistiller(Agent(23, 9), "tracks/big_track.json", device="cpu", **kw)


@pytest.mark.parametrize("cls", [pc.Planner, pc.CEMPlanner])
@pytest.mark.parametrize("T", [-1.0, float("nan"), float("inf")])
def test_planners_refuse_a_temperature(cls, T):
    with pytest.raises(ValueError, match="temperature"):
        cls(None, action_values=True, temperature=T)


def test_distill_flags_parse():
    base = ["--out", "x.dat", "--plan-iterations", "2", "--plan-elites", "4"]
    a = distill.parse_args(base)
    assert a.labels == "best" and a.label_temperature == 0.0
    a = distill.parse_args(base + ["--labels", "soft", "--label-temperature", "0.02"])
    assert a.labels == "soft" and a.label_temperature == 0.02
    for bad in (["--labels", "hard"], ["--label-temperature", "0.5"], ["--labels", "soft", "--label-temperature", "-1"]):
        with pytest.raises(SystemExit):
            distill.parse_args(base + bad)


class _Env:
    num_envs, obs_dim, act_dim, device = 8, 23, 9, torch.device("cpu")

    def __init__(self, *a, **kw):
        pass

    def close(self):
        pass


class _Planner:
    seen = None

    def __init__(self, envs, **kw):
        type(self).seen = kw


@pytest.mark.parametrize("labels,kind", [("best", "cem"), ("best", "shooting"), ("soft", "cem"), ("soft", "shooting")])
def test_only_soft_labels_ask_for_action_values(monkeypatch, labels, kind):
    monkeypatch.setattr(imitation, "VecCarEnv", _Env)
    monkeypatch.setattr(imitation, "CEMPlanner", _Planner)
    monkeypatch.setattr(imitation, "Planner", _Planner)
    extra = dict(labels="soft", label_temperature=0.25) if labels == "soft" else {}
    ds = pc.PlannerDistiller(Agent(23, 9), "unused", n_envs=8, planner=dict(kind=kind, horizon=4), steps_per_round=3, rounds=2, device="cpu",
                             learner=dict(batch_size=4), **extra)
    if labels == "best":
        assert "action_values" not in _Planner.seen and "temperature" not in _Planner.seen
        assert not hasattr(ds, "soft_buf") and not hasattr(ds, "_soft_stats")
    else:
        assert _Planner.seen["action_values"] is True and _Planner.seen["temperature"] == 0.25
        assert ds.soft_buf.shape == (2, 3, 8, 9) and ds.soft_buf.dtype == torch.float32
    assert ds.label_buf.shape == (2, 3, 8)


def test_planner_out_keys_follow_the_switch():
    assert planner._action_value_out(False, 4, torch.device("cpu")) == {}
    on = planner._action_value_out(True, 4, torch.device("cpu"))
    assert {k: (tuple(v.shape), v.dtype) for k, v in on.items()} == {"q": ((4, 9), torch.float64), "q_count": ((4, 9), torch.int32),
                                                                   "q_alive": ((4, 9), torch.uint8), "soft": ((4, 9), torch.float32)}


def test_learner_routes_a_two_dimensional_label_to_the_soft_loss():
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(4)
    obs = torch.rand(64, 23, generator=g)
    soft = torch.softmax(torch.randn(64, 9, generator=g), -1)
    soft[5] = 0.0
    a, b = Agent(23, 9), Agent(23, 9)
    b.load_state_dict(a.state_dict())
    L = BCLearner(a, batch_size=32, seed=1, device="cpu")
    assert L.path == "torch"
    out = L.fit(obs, soft, epochs=1)
    assert out["bc/steps"] == 2 and out["bc/ce"] > 0.0
    opt = torch.optim.Adam(b.parameters(), lr=3e-4, eps=1e-5)
    idx = BCLearner(Agent(23, 9), batch_size=32, seed=1, device="cpu").draw_indices(64)[0]
    for m in range(2):
        ix = idx[m * 32:(m + 1) * 32]
        opt.zero_grad()
        bc_soft_loss(b, obs[ix], soft[ix], None, 0.0, 0.0)[0].backward()
        torch.nn.utils.clip_grad_norm_(b.parameters(), 0.5)
        opt.step()
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in b.parameters()]), L.flat_param.detach())
    with pytest.raises(ValueError, match="label"):
        L.step(idx[:32], obs, soft[:, :8])
    with pytest.raises(ValueError, match="label"):
        L.step(idx[:32], obs, soft.view(64, 3, 3))
