"""Soft imitation targets end to end on the GPU: the planners' action_values switch, PlannerDistiller(labels="soft") beside labels="best",
and one round on both learner paths.  64 envs, 16 rays, 8 steps per round, 2 rounds; CEM with H = 4, K = 16, 2 iterations and the
shooting planner with H = 4, K = 16."""
import os

import numpy as np
import pytest
import torch

import ppo_car_amd as pc
from ppo_car_amd.imitation import PlannerDistiller
from conftest import ROOT

pytestmark = pytest.mark.gpu

TRACK = os.path.join(ROOT, "tracks", "big_track.json")
N, T, ROUNDS = 64, 8, 2
PLANNERS = {"cem": dict(kind="cem", horizon=4, candidates=16, elites=4, iterations=2), "shooting": dict(kind="shooting", horizon=4, candidates=16)}
BASE_KEYS = {"ret", "steps", "status", "best_k", "best_action", "best_ret"}


def _distiller(kind, labels, temperature=0.0, beta0=1.0, custom_mlp=True, rounds=ROUNDS):
    torch.manual_seed(21)
    agent = pc.Agent(23, 9).cuda()
    extra = dict(labels="soft", label_temperature=temperature) if labels == "soft" else {}
    return PlannerDistiller(agent, TRACK, n_envs=N, num_rays=16, planner=PLANNERS[kind], steps_per_round=T, beta0=beta0, beta_decay=1.0,
                            epochs_per_round=2, learner=dict(batch_size=256, custom_mlp=custom_mlp), seed=0, rounds=rounds, **extra)


def _rounds(ds):
    try:
        outs = [ds.round(r) for r in range(ds.rounds)]
        torch.cuda.synchronize()
        bufs = {k: getattr(ds, k).cpu() for k in ("obs_buf", "label_buf", "soft_buf") if hasattr(ds, k)}
        return outs, bufs, ds.learner.flat_param.detach().cpu().clone()
    finally:
        ds.close()


@pytest.mark.parametrize("temperature", [0.0, 0.02])
@pytest.mark.parametrize("kind", ["cem", "shooting"])
def test_soft_labels_beside_best_labels(kind, temperature):
    best_out, best, _ = _rounds(_distiller(kind, "best"))
    soft_out, soft, _ = _rounds(_distiller(kind, "soft", temperature))
    assert "soft_buf" not in best and not any(k in best_out[0] for k in ("bc/ties", "bc/label_entropy"))
    # beta0 = 1 and no decay: the teacher drives in both rounds, and it drives as it does under "best" (with a share of the envs the
    # student's draws would differ, since it is trained on other targets)
    for k in ("obs_buf", "label_buf"):
        assert torch.equal(soft[k].view(torch.int32), best[k].view(torch.int32)), k
    p, label = soft["soft_buf"].double(), soft["label_buf"]
    assert p.shape == (ROUNDS, T, N, 9) and (p >= 0).all()
    total, top = p.sum(-1), p.max(-1).values
    zero = (p == 0).all(-1)
    assert ((total - 1.0).abs() <= 9 * 2.0 ** -24)[~zero].all()
    # wherever label_buf carries a label, that action's entry is the row's maximum (and the row is not empty)
    on = label >= 0
    assert on.any() and not zero[on].any()
    picked = p.gather(-1, label.clamp(min=0).long().unsqueeze(-1)).squeeze(-1)
    assert torch.equal(picked[on], top[on])
    for r, out in enumerate(soft_out):
        rows = ~zero[r]
        tied = ((p[r] == top[r].unsqueeze(-1)).sum(-1) >= 2) & rows
        assert out["bc/ties"] == int(tied.sum()) / int(rows.sum())
        ent = -(p[r] * torch.log(torch.where(p[r] > 0, p[r], torch.ones_like(p[r])))).sum(-1)
        assert out["bc/label_entropy"] == pytest.approx(float(ent[rows].sum()) / int(rows.sum()), rel=1e-5, abs=1e-7)
        assert 0.0 <= out["bc/agreement"] <= 1.0 and out["bc/labelled"] == int(rows.sum()) / (T * N)
        if temperature == 0.0:      # all mass on the maximal actions: the entropy of a row is log(number of them)
            n = (p[r] == top[r].unsqueeze(-1)).sum(-1).double()
            assert torch.allclose(ent[rows], torch.log(n[rows]), atol=1e-6)
        print(f"{kind} T={temperature:g} round {r}: bc/ties {out['bc/ties']:.3f}, bc/label_entropy {out['bc/label_entropy']:.3f}, "
              f"bc/agreement {out['bc/agreement']:.3f}")


@pytest.mark.parametrize("kind", ["cem", "shooting"])
def test_one_round_on_both_learner_paths(kind):
    outs, params = [], []
    for custom in (True, False):
        ds = _distiller(kind, "soft", 0.02, custom_mlp=custom, rounds=1)
        assert ds.learner.path == ("custom" if custom else "torch")
        out, bufs, param = _rounds(ds)
        outs.append((out[0], bufs))
        params.append(param)
    assert torch.equal(outs[0][1]["soft_buf"], outs[1][1]["soft_buf"]) and outs[0][0]["bc/ties"] == outs[1][0]["bc/ties"]
    steps = outs[0][0]["bc/steps"]
    worst = float((params[0] - params[1]).abs().max())
    print(f"{kind}: custom against torch after {steps} soft steps: {worst:.3e}")
    assert steps == 2 * (T * N // 256) and worst <= 3e-6 * steps      # (tests/test_imitation_gpu.py's bar)
    assert outs[0][0]["bc/ce"] == pytest.approx(outs[1][0]["bc/ce"], rel=1e-4)


@pytest.mark.parametrize("kind", ["cem", "shooting"])
def test_the_switch_changes_nothing_else(kind):
    kw = {k: v for k, v in PLANNERS[kind].items() if k != "kind"}
    cls = pc.CEMPlanner if kind == "cem" else pc.Planner
    got = []
    for on in (False, True):
        env = pc.VecCarEnv(N, TRACK, num_rays=16, reward_scaling=0.1, device="cuda", dtype="f32")
        try:
            env.reset()
            p = cls(env, seed=0, **(dict(kw, action_values=True, temperature=0.02) if on else kw))
            assert set(p.out) == (BASE_KEYS | {"q", "q_count", "q_alive", "soft"} if on else BASE_KEYS)
            acts = []
            for t in range(6):
                a = p.act(t)
                acts.append(a.clone())
                env.step(a)
            if on:
                q, best = p.out["q"], p.out["best_ret"]
                assert torch.equal(q.max(-1).values, best)
                assert torch.equal(q.gather(1, p.out["best_action"].view(-1, 1)).view(-1).view(torch.int64), best.view(torch.int64))
                assert int(p.out["q_count"].sum(-1).min()) == int(p.out["q_count"].sum(-1).max()) == p.candidates * (p.iterations if kind == "cem" else 1)
            got.append(torch.stack(acts).cpu())
        finally:
            env.close()
    assert torch.equal(got[0], got[1])
