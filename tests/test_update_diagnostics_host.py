"""Update diagnostics and the target-KL stop (the pc_*_diag entry points, pc_explained_variance, PPOConfig.update_diagnostics /
target_kl): the C-ABI surface and its argument checks, the config / CLI switches, and the torch path on CPU tensors -- the
restatement the kernels are tested against (test_update_diagnostics_gpu.py) -- against float64 numpy.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from ppo_car_amd import Agent, _capi
from ppo_car_amd.ppo import PPOConfig, PPOLearner
from conftest import ROOT

INV, UNS, NODEV = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_UNSUPPORTED, _capi.PC_ERR_NO_DEVICE
P = 4096      # a non-NULL address: the checks run before any device call, nothing is dereferenced
NEW = ("pc_ppo_diag_workspace_floats", "pc_ppo_minibatch_diag", "pc_ppo_minibatch_prepared_diag", "pc_ppo_loss_diag", "pc_clip_adam_diag",
       "pc_explained_variance_workspace_doubles", "pc_explained_variance")


def test_symbols_in_header_exports_and_library():
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    assert re.search(r"#define PC_DIAG_FLOATS 8\b", hdr) and _capi.PC_DIAG_FLOATS == 8
    for name in NEW:
        assert re.search(r"\b(int|int64_t) " + name + r"\(", hdr), name
        assert name in _capi.EXPORTS
        assert getattr(_capi.lib, name) is not None
    for word in ("approx_kl = mean_i((ratio_i - 1) - logratio_i)", "clipfrac = mean_i(|ratio_i - 1| > clip_ratio)",
                 "1 - Var(ret - val) / Var(ret)", "1.5 * target_kl"):
        assert word in hdr, word      # the header states the definitions


def test_diag_workspace_holds_the_plain_layout_and_a_second_partial():
    for B, D in ((2, 18), (64, 23), (512, 23), (1024, 39)):
        plain = _capi.lib.pc_ppo_workspace_floats(B, D, 256, 9)
        assert _capi.lib.pc_ppo_diag_workspace_floats(B, D, 256, 9) == plain + 2 * ((B + 7) // 8)
    assert _capi.lib.pc_ppo_diag_workspace_floats(1, 23, 256, 9) == UNS
    assert _capi.lib.pc_ppo_diag_workspace_floats(64, 23, 128, 9) == UNS


def _mb(device=0, idx=P, data=(P,) * 5, param=P, grad=P, state=(P,) * 4, metrics=P, ws=P, apply=1, diag=P, kl=0.01, B=64, D=23, H=256, A=9):
    return _capi.lib.pc_ppo_minibatch_diag(device, idx, B, D, H, A, *data, param, grad, *state, 0.2, 0.5, 0.001, 1.0, 0.9, 0.999, 1e-5, metrics,
                                           ws, apply, diag, kl, None)


def _mbp(device=0, prep=P, param=P, grad=P, state=(P,) * 4, metrics=P, ws=P, apply=1, diag=P, kl=0.01, B=64, D=23, H=256, A=9):
    return _capi.lib.pc_ppo_minibatch_prepared_diag(device, prep, B, D, H, A, param, grad, *state, 0.2, 0.5, 0.001, 1.0, 0.9, 0.999, 1e-5,
                                                    metrics, ws, apply, diag, kl, None)


@pytest.mark.parametrize("kw", [dict(diag=None), dict(idx=None), dict(param=None), dict(grad=None), dict(metrics=None), dict(ws=None),
                                dict(data=(P, None, P, P, P)), dict(state=(None, P, P, P)), dict(state=(P, P, None, P)), dict(apply=3),
                                dict(apply=-1)])
def test_minibatch_diag_argument_checks(kw):
    assert _mb(**kw) == INV


@pytest.mark.parametrize("kw", [dict(diag=None), dict(prep=None), dict(param=None), dict(grad=None), dict(metrics=None), dict(ws=None),
                                dict(state=(P, None, P, P)), dict(apply=3)])
def test_minibatch_prepared_diag_argument_checks(kw):
    assert _mbp(**kw) == INV


@pytest.mark.parametrize("fn", [_mb, _mbp])
def test_minibatch_diag_refuses_the_multi_rank_form_and_unsupported_shapes(fn):
    assert fn(apply=2) == UNS
    assert fn(H=128) == UNS and fn(B=1) == UNS and fn(B=1025) == UNS and fn(D=41) == UNS and fn(A=16) == UNS


@pytest.mark.parametrize("fn", [_mb, _mbp])
@pytest.mark.parametrize("kl", [0.01, 0.0, -1.0, float("nan")])
def test_minibatch_diag_valid_arguments_reach_the_device_check(fn, kl):
    assert fn(device=-1, kl=kl) == NODEV
    assert fn(device=-1, kl=kl, apply=0, state=(None,) * 4) == NODEV      # apply == 0 needs no optimizer state


def _loss(device=0, ptrs=(P,) * 9, diag=P, B=64, A=9, kl=0.01):
    lg, v, a, lp, adv, ret, dl, dv, m = ptrs
    return _capi.lib.pc_ppo_loss_diag(device, lg, v, a, lp, adv, ret, B, A, 0.2, 0.5, 0.001, dl, dv, m, diag, kl, None)


def _adam(device=0, ptrs=(P,) * 6, n=1000, diag=P):
    return _capi.lib.pc_clip_adam_diag(device, *ptrs, n, 1.0, 1.0, 0.9, 0.999, 1e-5, diag, None)


@pytest.mark.parametrize("which", list(range(9)))
def test_loss_diag_null_arguments(which):
    assert _loss(ptrs=tuple(None if i == which else P for i in range(9))) == INV


@pytest.mark.parametrize("which", list(range(6)))
def test_clip_adam_diag_null_arguments(which):
    assert _adam(ptrs=tuple(None if i == which else P for i in range(6))) == INV


def test_loss_and_clip_adam_diag_other_checks():
    assert _loss(diag=None) == INV and _adam(diag=None) == INV
    assert _adam(n=0) == INV and _adam(n=(1 << 26) + 1) == INV
    assert _loss(B=1) == UNS and _loss(B=1025) == UNS and _loss(A=17) == UNS
    assert _loss(device=-1) == NODEV and _adam(device=-1) == NODEV


def _ev(device=0, val=P, ret=P, M=100, ws=P, out=P):
    return _capi.lib.pc_explained_variance(device, val, ret, M, ws, out, None)


@pytest.mark.parametrize("kw", [dict(val=None), dict(ret=None), dict(ws=None), dict(out=None), dict(M=0), dict(M=-5)])
def test_explained_variance_argument_checks(kw):
    assert _ev(**kw) == INV


def test_explained_variance_valid_arguments_reach_the_device_check():
    assert _ev(device=-1) == NODEV and _ev(device=-1, M=1) == NODEV and _ev(device=-1, M=1 << 27) == NODEV
    assert _capi.lib.pc_explained_variance_workspace_doubles(0) >= 5


def test_config_validation():
    c = PPOConfig()
    assert c.update_diagnostics is False and c.target_kl is None
    assert PPOConfig(update_diagnostics=True).target_kl is None
    c = PPOConfig(target_kl=0.02)
    assert c.update_diagnostics is True and c.target_kl == 0.02          # target_kl implies diagnostics
    for bad in (0.0, -0.1, float("nan"), "0.01", True):
        with pytest.raises(ValueError, match="target_kl"):
            PPOConfig(target_kl=bad)
    for kw in (dict(update_diagnostics=True), dict(target_kl=0.01)):
        with pytest.raises(ValueError, match="deferred_adam"):
            PPOConfig(deferred_adam=True, **kw)
        with pytest.raises(ValueError, match="force_collective"):
            PPOConfig(force_collective=True, **kw)
        with pytest.raises(ValueError, match="single rank"):           # (raised before any collective is touched)
            PPOLearner(Agent(D, A), PPOConfig(n_envs=4, n_steps=64, batch_size=32, **kw), "cpu", rank=0, world_size=2)
    PPOConfig(deferred_adam=True)
    PPOConfig(force_collective=True)


def test_cli_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_cli", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["--run-name", "x"])
    assert a.update_diagnostics is False and a.target_kl is None
    assert mod.parse_args(["--run-name", "x", "--update-diagnostics"]).update_diagnostics is True
    assert mod.parse_args(["--run-name", "x", "--target-kl", "0.015"]).target_kl == 0.015


# ---- the torch path on CPU tensors -------------------------------------------------------------------------------------------
D, A, M, B = 23, 9, 256, 32
CFG = dict(n_envs=4, n_steps=64, batch_size=B, train_iters=3, seed=3, learning_rate=3e-3)     # 2 minibatches x 3 iterations = 6 steps


def _learner(**kw):
    torch.manual_seed(50)
    return PPOLearner(Agent(D, A), PPOConfig(**CFG, **kw), "cpu")


def _rollout(agent):
    """A synthetic rollout whose behaviour policy IS the agent at its initial parameters (ratio = 1 at the first step, as in a
    real epoch), with a few percent of the old log-probs disturbed so that some ratios start outside the clip range."""
    g = torch.Generator().manual_seed(1000)
    obs = torch.randn(M, D, generator=g)
    act = torch.randint(0, A, (M,), generator=g).float()
    with torch.no_grad():
        _, lp, _, _ = agent.get_action_and_value(obs, act)
    lp = lp + (torch.rand(M, generator=g) < 0.1).float() * torch.randn(M, generator=g) * 0.5
    return obs, act, lp.contiguous(), torch.randn(M, generator=g), torch.randn(M, generator=g)


def logratio_f64(flat_param, obs, act, old_lp):
    """new_logprob - old_logprob of model.py's Agent in float64 numpy, from the flat parameter bucket (module.parameters() order)."""
    p = flat_param.detach().cpu().numpy().astype(np.float64)
    Dn = obs.shape[1]
    An = (p.size - 2 * (256 * Dn + 256) - 257) // 257
    o = 0
    W1 = p[o:o + 256 * Dn].reshape(256, Dn); o += 256 * Dn
    b1 = p[o:o + 256]; o += 256
    W2 = p[o:o + An * 256].reshape(An, 256); o += An * 256
    b2 = p[o:o + An]
    x = obs.detach().cpu().numpy().astype(np.float64)
    logits = np.maximum(x @ W1.T + b1, 0.0) @ W2.T + b2
    logits -= logits.max(axis=1, keepdims=True)
    logp = logits - np.log(np.exp(logits).sum(axis=1, keepdims=True))
    a = act.detach().cpu().numpy().astype(np.int64)
    return logp[np.arange(len(a)), a] - old_lp.detach().cpu().numpy().astype(np.float64)


def diag_f64(logratio, clip):
    """(approx_kl, clip count, margin of every sample to the clip boundary) of CleanRL's definitions in float64."""
    r = np.exp(logratio)
    return float(((r - 1.0) - logratio).mean()), int((np.abs(r - 1.0) > clip).sum()), np.abs(np.abs(r - 1.0) - clip)


def _recorded_run(**kw):
    L = _learner(**kw)
    data = _rollout(L.agent)
    steps = []
    book = L._book_diag

    def spy():
        steps.append((L.flat_param.clone(), L._diag_terms.clone()))
        return book()
    L._book_diag = spy
    L.update(*data)
    return L, data, steps


def _step_indices(L, j):
    n_mb = L.n_minibatches
    return L._idx_dev[j // n_mb, (j % n_mb) * B:(j % n_mb + 1) * B]


def test_torch_path_matches_the_float64_restatement():
    L, (obs, act, lp, adv, ret), steps = _recorded_run(update_diagnostics=True)
    assert len(steps) == 6
    kl_sum = cf_sum = 0.0
    for j, (param, terms) in enumerate(steps):
        idx = _step_indices(L, j)
        kl, n_clip, margin = diag_f64(logratio_f64(param, obs[idx], act[idx], lp[idx]), L.cfg.clip_ratio)
        # float32 torch against float64: the log-prob of a 23 x 256 x 9 MLP in float32 is good to ~1e-6, and d kl / d logratio = ratio - 1
        # (|.| < 2 here), the float32 mean adds ~1e-7 relative: 1e-5 leaves a factor of a few
        assert float(terms[0]) == pytest.approx(kl, abs=1e-5), j
        assert margin.min() > 1e-5, "the restatement's own clip decisions must not hang on rounding"
        assert float(terms[1]) * B == n_clip, j
        kl_sum += float(terms[0])
        cf_sum += float(terms[1])
    assert float(steps[0][1][1]) > 0.0                                           # some samples start outside the clip range
    assert float(steps[-1][1][0]) > float(steps[1][1][0]) > 0.0                  # ... and the policy moves away
    d = L.diag.tolist()
    assert d[2] == 6.0 and d[3] == 6.0 and d[4] == 0.0
    assert d[0] == pytest.approx(kl_sum, rel=1e-6) and d[1] == pytest.approx(cf_sum, rel=1e-6) and d[5] == float(steps[-1][1][0])


def _opt_state(L):
    out = []
    for p in L.agent.parameters():
        st = L.optimizer.state[p]
        out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone(), torch.as_tensor(st["step"]).clone().reshape(1).float()]
    return out


def test_target_kl_stops_at_step_k_with_the_state_of_k_plain_steps():
    _, _, steps = _recorded_run(update_diagnostics=True)
    kls = [float(t[0]) for _, t in steps]
    # the first step k (1 < k < last) whose approx_kl exceeds every earlier one: a threshold between the two makes the stop fire there
    k = next((j for j in range(2, len(kls) - 1) if kls[j] > max(kls[:j]) * 1.05), None)
    assert k is not None, f"no step with a new maximum of approx_kl among steps 2..{len(kls) - 2}: {kls}"      # (a condition on the inputs)
    thr = 0.5 * (kls[k] + max(kls[:k]))
    L, data, stopped_steps = _recorded_run(target_kl=thr / 1.5)
    assert len(stopped_steps) == k + 1                                           # k applied, one evaluated and refused, none after
    d = L.diag.tolist()
    assert d[3] == k and d[2] == k + 1 and d[4] == 1.0 and d[5] == np.float32(kls[k])
    # exactly k plain minibatch steps on the same indices
    R = _learner()
    assert R.diag is None and not R.diag_on
    idx_all = R.draw_indices(M)
    assert torch.equal(idx_all, L._idx_dev)
    for j in range(k):
        idx = _step_indices(R, j)
        R.minibatch_step(*[t[idx] for t in data])
    assert torch.equal(L.flat_param, R.flat_param)
    for a, b in zip(_opt_state(L), _opt_state(R)):
        assert torch.equal(a, b)
    assert torch.equal(L.metrics, R.metrics)                                     # the refused step adds nothing to the logged sums
    assert not torch.equal(L.flat_param, stopped_steps[0][0])                    # (steps were applied)


def test_options_off_leave_the_learner_as_it_was():
    L = _learner()
    data = _rollout(L.agent)
    L.update(*data)
    Ldiag, _, _ = _recorded_run(update_diagnostics=True)
    assert torch.equal(L.flat_param, Ldiag.flat_param) and torch.equal(L.metrics, Ldiag.metrics)     # diagnostics alone change nothing
    for a, b in zip(_opt_state(L), _opt_state(Ldiag)):
        assert torch.equal(a, b)
