"""Imitation on the device: pc_bc_minibatch (K27 + K11 + K12) against bc_loss in float64 and against pc_ppo_minibatch where the two
share code, the ignore rule, the applied step, BCLearner's custom path, and PlannerDistiller against a plain CEMPlanner.drive."""
import os

import numpy as np
import pytest
import torch

import ppo_car_amd as pc
from ppo_car_amd.imitation import BCLearner, PlannerDistiller, bc_loss
from conftest import ROOT
from ppo_update_reference import EC, LR, MAX_NORM, VF, Call

pytestmark = pytest.mark.gpu
TRACK = os.path.join(ROOT, "tracks", "big_track.json")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _critic_offset(D, A):
    return 256 * D + 256 + A * 256 + A


def _agent(D, A, scale=1.0, seed=0):
    torch.manual_seed(seed)
    a = pc.Agent(D, A)
    with torch.no_grad():
        a.actor[2].weight *= scale
        a.actor[2].bias *= scale
    return a


def _flat(agent, dtype=torch.float32):
    return torch.cat([p.detach().reshape(-1) for p in agent.parameters()]).to("cuda", dtype).contiguous()


def _batch(B, D, A, seed=0):
    """obs [M][D], label / target [M], idx [B] with a duplicate; the batch holds the labels -1, 0 and A-1 (B = 2: -1 and A-1)"""
    g = torch.Generator().manual_seed(100 + seed)
    M = B + 7
    obs = torch.rand(M, D, generator=g) * 2.6 - 1.0
    label = torch.randint(-1, A, (M,), generator=g).float()
    target = torch.randn(M, generator=g)
    idx = torch.randint(0, M, (B,), generator=g)
    if B >= 4:
        idx[:3] = torch.tensor([0, 1, 2])
        idx[3] = 1                                   # a duplicate
        label[:3] = torch.tensor([-1.0, 0.0, A - 1.0])
    else:
        idx[:2] = torch.tensor([0, 2])
        label[0], label[2] = -1.0, A - 1.0
    return obs, label, target, idx


def _cuda(*ts):
    return tuple(t.cuda().contiguous() for t in ts)


def _reference(agent, obs, label, target, idx, vf=VF, ec=EC):
    """bc_loss in float64 with the parameters cast up, through autograd: (flat gradient, (ce, vl, ent, total)) as numpy float64"""
    a64 = pc.Agent(obs.shape[1], agent.actor[2].out_features).double()
    a64.load_state_dict({k: v.double() for k, v in agent.state_dict().items()})
    total, ce, vl, ent = bc_loss(a64, obs.double()[idx], label.double()[idx], None if target is None else target.double()[idx], vf, ec)
    total.backward()
    g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in a64.parameters()]).numpy()
    return g, np.array([float(ce.detach()), float(vl.detach()), float(ent.detach()), float(total.detach())])


@pytest.mark.parametrize("scale", [1.0, 40.0, 4000.0])
@pytest.mark.parametrize("B,D,A", [(2, 18, 9), (8, 23, 9), (9, 23, 9), (1024, 39, 9), (64, 10, 5)])
def test_gradient_and_metrics_against_float64(B, D, A, scale):
    """apply = 0 against bc_loss in float64 at the project's tolerance for this forward / backward pass (rtol 2e-4, atol 2e-7); the
    metric sums at rel 1e-5, abs 1e-6.  Shapes: the minimum B; one full workgroup; one workgroup with a single live sample; 128
    partials at the widest compiled observation; the run-time-shape form.  The actor's output layer scaled by 40 keeps these
    observations' logits below 1 (its initial std is 0.01), so a third scale, 4000, is the saturated softmax: logit magnitudes of
    14 .. 46 over the five shapes.  The same tolerance holds there: a float32 torch restatement of bc_loss on the CPU stays within
    0.36 of the allowance at every shape and scale (0.04 at scales 1 and 40)."""
    agent = _agent(D, A, scale)
    obs, label, target, idx = _batch(B, D, A)
    lab = label[idx]
    assert (lab == -1).any() and (lab == A - 1).any() and (B < 4 or (lab == 0).any()) and (B < 4 or len(set(idx.tolist())) < B)
    gref, mref = _reference(agent, obs, label, target, idx)
    c = Call(_flat(agent), B, D, A).bc(*_cuda(idx, obs, label, target))
    g, m = c.grad.cpu().numpy().astype(np.float64), c.metrics.cpu().numpy()
    ratio = float((np.abs(g - gref) / (2e-7 + 2e-4 * np.abs(gref))).max())
    print(f"B={B} D={D} A={A} scale={scale}: worst error / allowance = {ratio:.3f}; metrics {m} reference {mref}")
    assert np.allclose(g, gref, rtol=2e-4, atol=2e-7), ratio
    for got, ref, key in zip(m, mref, ("ce", "vl", "ent", "total")):
        assert float(got) == pytest.approx(float(ref), rel=1e-5, abs=1e-6), key
    assert torch.equal(c.step, torch.zeros(1, device="cuda")) and torch.equal(c.param, _flat(agent))      # apply = 0 moves nothing


@pytest.mark.parametrize("B", [9, 512])
def test_the_halves_shared_with_the_ppo_step_are_bit_equal(B):
    """Same obs, idx, parameters and coefficients, target = ret, every label live and equal to the PPO call's act: the critic's four
    gradient slices and the value-loss and entropy sums are the same code in both kernels -- the same bits."""
    D, A = 23, 9
    agent = _agent(D, A, seed=1)
    obs, label, ret, idx = _batch(B, D, A, seed=1)
    g = torch.Generator().manual_seed(5)
    act = torch.randint(0, A, label.shape, generator=g).float()
    old_lp = -2.2 + 0.3 * torch.randn(label.shape, generator=g)
    adv = torch.randn(label.shape, generator=g)
    idx, obs, act, old_lp, adv, ret = _cuda(idx, obs, act, old_lp, adv, ret)
    p = _flat(agent)
    bc = Call(p, B, D, A).bc(idx, obs, act, ret)
    ppo = Call(p, B, D, A).ppo(idx, obs, act, old_lp, adv, ret)
    o = _critic_offset(D, A)
    assert torch.equal(bc.grad[o:], ppo.grad[o:]) and bc.grad[o:].abs().max() > 0
    assert torch.equal(bc.metrics[1:3], ppo.metrics[1:3]) and (bc.metrics[1:3] > 0).all()
    assert not torch.equal(bc.grad[:o], ppo.grad[:o])      # (the actor's loss is another one)


def test_the_ignore_rule():
    B, D, A = 64, 23, 9
    agent = _agent(D, A, seed=2)
    obs, label, target, idx = _batch(B, D, A, seed=2)
    none = torch.full_like(label, -1.0)
    none[1::3] = float(A)          # (every kind of "no label")
    none[2::3] = A + 3.0
    live = label.clamp_min(0.0)
    idx, obs, none, live, target = _cuda(idx, obs, none, live, target)
    p = _flat(agent)
    # no label anywhere, no targets: nothing at all
    c = Call(p, B, D, A)
    c.metrics.copy_(torch.tensor([1.5, 2.5, 3.5, 4.5]))
    c.bc(idx, obs, none, None, vf=0.0)
    assert torch.equal(c.grad, torch.zeros_like(c.grad)) and torch.equal(c.metrics.cpu(), torch.tensor([1.5, 2.5, 3.5, 4.5]))
    assert not torch.signbit(c.grad[_critic_offset(D, A):]).any()      # the critic's gradient is +0.0f
    # no label anywhere, with the value term: the actor rests, the critic's gradient is the all-live call's
    a = Call(p, B, D, A).bc(idx, obs, none, target)
    b = Call(p, B, D, A).bc(idx, obs, live, target)
    o = _critic_offset(D, A)
    assert torch.equal(a.grad[:o], torch.zeros_like(a.grad[:o]))
    assert torch.equal(a.grad[o:], b.grad[o:]) and a.grad[o:].abs().max() > 0 and b.grad[:o].abs().max() > 0
    assert float(a.metrics[0]) == 0.0 and float(a.metrics[2]) == 0.0 and torch.equal(a.metrics[1], b.metrics[1])


def test_the_applied_step_against_float64_clip_and_adam():
    B, D, A = 512, 23, 9
    agent = _agent(D, A, seed=3)
    obs, label, target, idx = _batch(B, D, A, seed=3)
    gref, _ = _reference(agent, obs, label, target, idx)
    p0 = _flat(agent, torch.float64).cpu().numpy()
    norm = float(np.sqrt((gref ** 2).sum()))
    gc = gref * min(1.0, MAX_NORM / (norm + 1e-6))          # clip_grad_norm_
    m, v = 0.1 * gc, 0.001 * gc * gc                          # Adam's first step from zero moments
    p1 = p0 - LR * (m / (1 - 0.9)) / (np.sqrt(v / (1 - 0.999)) + 1e-5)
    c = Call(_flat(agent), B, D, A).bc(*_cuda(idx, obs, label, target), apply=1)
    got = c.param.cpu().numpy().astype(np.float64)
    assert np.abs(got - p1).max() <= 3e-6
    assert np.abs(p1 - p0).max() > 1e-4
    assert float(c.step) == 1.0
    assert np.allclose(c.grad.cpu().numpy(), gc, rtol=2e-4, atol=2e-7)      # grad holds the clipped gradient


def test_applied_steps_without_targets_leave_the_critic_and_repeat_bit_for_bit():
    B, D, A = 512, 23, 9
    agent = _agent(D, A, seed=4)
    obs, label, _, _ = _batch(B, D, A, seed=4)
    g = torch.Generator().manual_seed(9)
    idxs = [torch.randint(0, obs.shape[0], (B,), generator=g).cuda() for _ in range(3)]
    obs, label = _cuda(obs, label)
    p = _flat(agent)
    o = _critic_offset(D, A)

    def run():
        c = Call(p, B, D, A)
        for idx in idxs:
            c.bc(idx, obs, label, None, vf=0.0, apply=1)
        return c

    a, b = run(), run()
    assert float(a.step) == 3.0
    assert torch.equal(a.param[o:], p[o:]) and not torch.equal(a.param[:o], p[:o])
    assert not a.m[o:].any() and not a.v[o:].any()
    for x, y in ((a.param, b.param), (a.grad, b.grad), (a.m, b.m), (a.v, b.v), (a.metrics, b.metrics), (a.step, b.step)):
        assert torch.equal(x, y)


def _fixed_set(M=256, D=23, A=9):
    g = torch.Generator().manual_seed(17)
    obs = torch.rand(M, D, generator=g) * 2.6 - 1.0
    label = torch.randint(0, A, (M,), generator=g).float()
    label[::11] = -1.0
    return _cuda(obs, label)


def test_learner_on_the_device():
    obs, label = _fixed_set()
    agent = _agent(23, 9, seed=5).cuda()
    L = BCLearner(agent, batch_size=64, seed=3)
    assert L.path == "custom"
    twin = _agent(23, 9, seed=5).cuda()
    T = BCLearner(twin, batch_size=64, seed=3, custom_mlp=False)
    assert T.path == "torch" and torch.equal(T.flat_param, L.flat_param)
    first = L.fit(obs, label, epochs=1)
    T.fit(obs, label, epochs=1)
    steps = first["bc/steps"]
    assert steps == 4 and float(L.step_count) == 4.0
    worst = float((L.flat_param - T.flat_param).abs().max())
    print(f"custom against torch after {steps} steps: {worst:.3e}")
    assert worst <= 3e-6 * steps
    # the packed policy image follows the weights
    logits0, logits1 = torch.empty(256, 9, device="cuda"), torch.empty(256, 9, device="cuda")
    agent.act(obs, out_logits=logits0, greedy=True, repack=False)
    assert agent._image_ok
    L.step(torch.arange(64, device="cuda"), obs, label)
    assert agent._image_ok is False
    agent.act(obs, out_logits=logits1, greedy=True, repack=False)
    assert agent._image_ok and not torch.equal(logits0, logits1)
    for _ in range(29):
        last = L.fit(obs, label, epochs=1)
    assert last["bc/ce"] < first["bc/ce"], (first, last)
    assert last["bc/value_loss"] == 0.0


CEM = dict(kind="cem", horizon=4, candidates=16, elites=4, iterations=2)


def _distiller(beta0, beta_decay, seed=0):
    torch.manual_seed(21)
    agent = pc.Agent(23, 9).cuda()
    return PlannerDistiller(agent, TRACK, n_envs=64, num_rays=16, planner=CEM, steps_per_round=40, beta0=beta0, beta_decay=beta_decay,
                            epochs_per_round=2, learner=dict(batch_size=256), seed=seed, rounds=2)


def test_distiller_with_the_teacher_driving_is_the_planners_drive():
    T, N = 40, 64
    env = pc.VecCarEnv(N, TRACK, num_rays=16, reward_scaling=0.1, device="cuda", dtype="f32")
    ds = _distiller(1.0, 1.0)
    try:
        env.reset()
        planner = pc.CEMPlanner(env, horizon=4, candidates=16, elites=4, iterations=2, seed=0)
        acts, step = [], env.step

        def recording_step(a, out=None):
            acts.append(a.clone())
            return step(a, out=out)

        env.step = recording_step
        rew, term, trunc = planner.drive(T)
        out0 = ds.round(0)
        labels, want = ds.label_buf[0].cpu(), torch.stack(acts).float().cpu()
        live = labels >= 0
        assert labels.shape == (T, N) and torch.equal(labels[live], want[live])
        assert ((labels >= -1) & (labels <= 8) & (labels == labels.round())).all()
        assert torch.equal(ds.rew, rew) and torch.equal(ds.term, term) and torch.equal(ds.trunc, trunc)
        assert 0.0 < out0["bc/labelled"] <= 1.0 and out0["bc/labelled"] == int(live.sum()) / (T * N)
        assert 0.0 <= out0["bc/agreement"] <= 1.0 and out0["bc/beta"] == 1.0
        out1 = ds.round(1)
        assert out1["bc/beta"] == 1.0 and out1["bc/steps"] == 2 * (2 * T * N // 256) and out0["bc/steps"] == 2 * (T * N // 256)
        assert 0.0 <= out1["bc/agreement"] <= 1.0
    finally:
        ds.close()
        env.close()


def test_distiller_with_a_mixed_share_is_deterministic():
    outs = []
    for _ in range(2):
        ds = _distiller(0.5, 0.5, seed=3)
        try:
            rows = [ds.round(r) for r in range(2)]
            outs.append((ds.learner.flat_param.clone(), rows, ds.label_buf.clone()))
        finally:
            ds.close()
    (pa, ra, la), (pb, rb, lb) = outs
    assert torch.equal(pa, pb) and ra == rb and torch.equal(la, lb)
    assert [r["bc/beta"] for r in ra] == [0.5, 0.25]
    for r in ra:
        assert 0.0 <= r["bc/agreement"] <= 1.0 and 0.0 < r["bc/labelled"] <= 1.0 and np.isfinite(r["bc/ce"])


def test_a_critic_bootstrapped_teacher_stays_frozen():
    f = np.load(os.path.join(GOLDEN, "policy_trained.npz"))
    teacher = pc.Agent(23, 9)
    teacher.load_state_dict({k: torch.from_numpy(f[k.replace(".", "_")]) for k in teacher.state_dict()})
    teacher = teacher.cuda().requires_grad_(False)
    t0 = _flat(teacher)
    torch.manual_seed(22)
    student = pc.Agent(23, 9).cuda()
    s0 = _flat(student)
    ds = PlannerDistiller(student, TRACK, n_envs=32, num_rays=16, steps_per_round=10, rounds=1, learner=dict(batch_size=64),
                          planner=dict(kind="cem", horizon=2, candidates=16, elites=4, iterations=2, agent=teacher, gamma=0.99, bootstrap="running"))
    try:
        out = ds.round(0)
        assert "end_value" in ds.planner.out      # the teacher did consult the critic
    finally:
        ds.close()
    assert out["bc/steps"] == 4 * 5 and np.isfinite(out["bc/loss"])
    assert torch.equal(_flat(teacher), t0) and not torch.equal(_flat(student), s0)


def test_distill_cli_writes_a_checkpoint_evaluate_reads(tmp_path, capsys):
    import json
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import distill
    import evaluate
    out = str(tmp_path / "student.dat")
    lines = distill.main(["--track", TRACK, "--num-rays", "16", "--envs", "64", "--out", out, "--rounds", "2", "--steps-per-round", "16",
                          "--planner", "cem", "--plan-horizon", "4", "--plan-candidates", "16", "--plan-iterations", "2", "--plan-elites", "4",
                          "--batch-size", "256", "--epochs", "1", "--eval-every", "2", "--eval-envs", "64"])
    printed = [json.loads(s) for s in capsys.readouterr().out.strip().split("\n")]
    assert printed == lines and [p["round"] for p in printed] == [0, 1]
    assert "eval/gates_per_episode" in printed[1] and "eval/gates_per_episode" not in printed[0]
    assert all(k in printed[0] for k in ("bc/ce", "bc/value_loss", "bc/entropy", "bc/loss", "bc/steps", "bc/agreement", "bc/beta", "bc/labelled"))
    sd = torch.load(out, map_location="cuda", weights_only=True)
    agent = pc.Agent(23, 9).cuda()
    agent.load_state_dict(sd)
    res = evaluate.main(["--checkpoint", out, "--track", TRACK, "--num-rays", "16", "--envs", "64"])
    assert res["eval/episodes"] == 64
