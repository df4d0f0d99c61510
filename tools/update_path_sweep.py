"""Developer probe (GPU box): every path of the PPO update, a few minibatch steps each, one line per case with a SHA-256 of what the
case left behind.  Two builds that keep behaviour print the same lines; run it once per tree and compare the outputs.

Trainer cases (32 envs, 40 or 64 steps, train_iters 2, two epochs, seed 0): the torch-op step, the fused loss / Adam kernels around
torch's GEMMs, the hand-written step (per minibatch, prepared, deferred chain, with an exchange step, with diagnostics and target_kl,
full_sweep, the three compiled shapes) and the large-minibatch step (a full and a ragged last group, with and without an exchange step
and graphs).  Hashed: flat_param, metrics, the Adam state, and `diag` where the case has one.

Direct C calls, for the generic kernels the Trainer never reaches: pc_ppo_minibatch, _diag, _prepared, _prepared_diag and
pc_ppo_epoch_prepared at (D 7, A 3) and (D 30, A 5) with B = 9 (two workgroups, the second holding one sample) and apply 0 / 1 / 2,
pc_ppo_minibatch_large at (D 7, A 3) and B = 1029, pc_ppo_loss / _diag at B 2 / 65 and A 1 / 16, pc_clip_adam / _diag at n 1 / 1025.
Hashed: the return code, param, grad, the moments, the step counter, metrics and `diag`.

The cases with an exchange step (force_collective) run inside a one-rank gloo process group, as the tests set one up.

    python tools/update_path_sweep.py [--root DIR] [--skip-large] [--dry-run]     (DIR: the tree whose package is imported; default: this one)

--dry-run needs no GPU: every PPOConfig is built, and every direct C call is made with device -1 on host tensors, so the keywords, the
argument counts and the argument types are checked (the calls fail at the device, before any launch); no hash means anything.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import torch
import torch.distributed as dist

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--skip-large", action="store_true", help="leave the large-minibatch cases out")
ap.add_argument("--dry-run", action="store_true", help="no GPU: build the configurations, make the C calls with device -1")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
from ppo_car_amd import _capi  # noqa: E402
from ppo_car_amd.ppo import PPOConfig, Trainer  # noqa: E402

lib = _capi.lib
DRY = args.dry_run
DEV, H = (-1 if DRY else 0), 256
TDEV = "cpu" if DRY else "cuda"
TRACK = os.path.join(ROOT, "tracks", "big_track.json")
COEF = (0.2, 0.5, 0.001, 1.0, 0.9, 0.999, 1e-5)      # clip, vf, ent | max_norm, beta1, beta2, eps


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:32]


def ptr(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def zeros(n, dtype=torch.float32):
    return torch.zeros(max(int(n), 1), dtype=dtype, device=TDEV)      # (dry run: a size query that needs the device answers < 0)


def sync():
    if not DRY:
        torch.cuda.synchronize()


def launched(rc):
    """A call that must succeed; in a dry run it must get past its argument checks and fail at the device"""
    assert rc in ((_capi.PC_ERR_NO_DEVICE, _capi.PC_ERR_HIP) if DRY else (_capi.PC_OK,)), rc


# ---- Trainer cases ---------------------------------------------------------------------------------------------------------------
def trainer_case(name, **kw):
    base = dict(n_envs=32, n_steps=40, batch_size=16, train_iters=2, track=TRACK, seed=0)
    base.update(kw)
    cfg = PPOConfig(**base)
    if DRY:
        print(f"trainer {name}: config ok", flush=True)
        return
    group = bool(cfg.force_collective)      # the exchange step is an all-reduce: it needs a process group, one rank here
    if group:
        dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        tr = Trainer(cfg, device="cuda:0")
        for _ in range(2):
            tr.run_epoch()
        torch.cuda.synchronize()
        L = tr.learner
        if L.flat_adam:
            state = [L.exp_avg, L.exp_avg_sq, L.step_count, L.lr_dev]
        else:
            state = [v for p in tr.agent.parameters() for _, v in sorted(L.optimizer.state[p].items()) if torch.is_tensor(v)]
            state.append(torch.tensor([L.current_lr()], dtype=torch.float64))
        path = (f"fused={int(L.fused)} custom={int(L.custom)} large={int(L.large)} flat_adam={int(L.flat_adam)} "
                f"graph={int(L._epoch_graph is not None)}")
        line = f"trainer {name}: {path} param={sha(L.flat_param)} metrics={sha(L.metrics)} adam={sha(*state)}"
        if L.diag is not None:
            line += f" diag={sha(L.diag)}"
        print(line, flush=True)
        tr.close()
    finally:
        if group:
            dist.destroy_process_group()


def trainer_cases():
    for graphs in (True, False):
        g = dict(use_graphs=graphs)
        trainer_case(f"torch graphs={graphs}", fused_update=False, **g)
        trainer_case(f"fused graphs={graphs}", custom_mlp=False, **g)
        trainer_case(f"fused diag graphs={graphs}", custom_mlp=False, update_diagnostics=True, **g)
        trainer_case(f"custom prepared graphs={graphs}", **g)
        trainer_case(f"custom unprepared graphs={graphs}", prepared_minibatches=False, **g)
        trainer_case(f"custom diag prepared graphs={graphs}", update_diagnostics=True, **g)
        trainer_case(f"custom diag unprepared graphs={graphs}", update_diagnostics=True, prepared_minibatches=False, **g)
        trainer_case(f"custom deferred graphs={graphs}", deferred_adam=True, **g)
        trainer_case(f"custom collective prepared graphs={graphs}", force_collective=True, **g)
        trainer_case(f"custom collective unprepared graphs={graphs}", force_collective=True, prepared_minibatches=False, **g)
    for tk in (1e-6, 1e3):
        trainer_case(f"torch target_kl={tk}", fused_update=False, target_kl=tk)
        trainer_case(f"fused target_kl={tk}", custom_mlp=False, target_kl=tk)
        trainer_case(f"custom target_kl={tk}", target_kl=tk)
        trainer_case(f"custom unprepared target_kl={tk}", target_kl=tk, prepared_minibatches=False)
    trainer_case("custom full_sweep", full_sweep=True, batch_size=256)
    trainer_case("torch full_sweep", full_sweep=True, batch_size=256, fused_update=False)
    for rays in (12, 16, 32):
        trainer_case(f"custom rays={rays}", num_rays=rays, batch_size=64)
        trainer_case(f"custom diag rays={rays}", num_rays=rays, batch_size=64, update_diagnostics=True)
        trainer_case(f"custom deferred rays={rays}", num_rays=rays, batch_size=64, deferred_adam=True)
    if not args.skip_large:
        for B in (1032, 1029):
            for coll in (False, True):
                for graphs in (True, False):
                    trainer_case(f"large B={B} collective={coll} graphs={graphs}", large_minibatch=True, batch_size=B, n_steps=64,
                                 force_collective=coll, use_graphs=graphs)


# ---- direct C calls --------------------------------------------------------------------------------------------------------------
def rnd(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(TDEV)


def mb_inputs(D, A, B, M, seed):
    """One pool of M samples, three index rows of B, parameters and Adam state of the (D, 256, A) pair: all from `seed`"""
    gen = torch.Generator().manual_seed(seed)
    n = 2 * (H * D + H) + A * H + A + H + 1
    s = dict(obs=rnd(gen, M, D), act=torch.randint(0, A, (M,), generator=gen).float().to(TDEV), lp=rnd(gen, M, scale=0.3) - 1.0,
             adv=rnd(gen, M), ret=rnd(gen, M), param=rnd(gen, n, scale=0.1), grad=zeros(n), m=rnd(gen, n, scale=0.01),
             v=rnd(gen, n, scale=0.01).abs(), step=torch.full((1,), 3.0, device=TDEV), lr=torch.full((1,), 3e-4, device=TDEV),
             metrics=zeros(4), diag=zeros(_capi.PC_DIAG_FLOATS))
    s["idx"] = torch.stack([torch.randperm(M, generator=gen)[:B] for _ in range(3)]).to(TDEV)
    return s


def samples(s):
    return [ptr(s[k]) for k in ("obs", "act", "lp", "adv", "ret")]


def state_coef(s, ws):
    """param .. lr_dev, the seven coefficients, metrics, workspace: what the minibatch entry points share (apply follows)"""
    return [ptr(s[k]) for k in ("param", "grad", "m", "v", "step", "lr")] + list(COEF) + [ptr(s["metrics"]), ptr(ws)]


def prepared(s, D, B):
    pf = lib.pc_ppo_prepared_floats(B, D)
    prep = zeros(3 * pf)
    rc = lib.pc_ppo_prepare(DEV, ptr(s["idx"]), B, 3, B, D, *samples(s), ptr(prep), None)
    launched(rc)
    return pf, prep


def mb_hash(rc, s, diag=False):
    sync()
    out = f"rc={rc} grad={sha(s['grad'])} state={sha(s['param'], s['m'], s['v'], s['step'])} metrics={sha(s['metrics'])}"
    return out + (f" diag={sha(s['diag'])}" if diag else "")


def small_cases(D, A, B=9, M=50):
    ws_plain, ws_diag = lib.pc_ppo_workspace_floats(B, D, H, A), lib.pc_ppo_diag_workspace_floats(B, D, H, A)
    for apply in (0, 1, 2):
        s = mb_inputs(D, A, B, M, 1)
        rc = lib.pc_ppo_minibatch(DEV, ptr(s["idx"][0]), B, D, H, A, *samples(s), *state_coef(s, zeros(ws_plain)), apply, None)
        print(f"pc_ppo_minibatch D={D} A={A} B={B} apply={apply} {mb_hash(rc, s)}", flush=True)
        for tk in (0.0, 1e-6):
            s = mb_inputs(D, A, B, M, 1)
            ws = zeros(ws_diag)
            for it in range(2):     # (the second call finds the flag up when the first one stopped)
                rc = lib.pc_ppo_minibatch_diag(DEV, ptr(s["idx"][it]), B, D, H, A, *samples(s), *state_coef(s, ws), apply, ptr(s["diag"]), tk,
                                               None)
            print(f"pc_ppo_minibatch_diag D={D} A={A} B={B} apply={apply} target_kl={tk} {mb_hash(rc, s, True)}", flush=True)
        s = mb_inputs(D, A, B, M, 2)
        pf, prep = prepared(s, D, B)
        rc = lib.pc_ppo_minibatch_prepared(DEV, C.c_void_p(prep.data_ptr() + 4 * pf), B, D, H, A, *state_coef(s, zeros(ws_plain)), apply, None)
        print(f"pc_ppo_minibatch_prepared D={D} A={A} B={B} apply={apply} prep={sha(prep)} {mb_hash(rc, s)}", flush=True)
        s = mb_inputs(D, A, B, M, 2)
        rc = lib.pc_ppo_minibatch_prepared_diag(DEV, C.c_void_p(prep.data_ptr() + 8 * pf), B, D, H, A, *state_coef(s, zeros(ws_diag)), apply,
                                                ptr(s["diag"]), 0.5, None)
        print(f"pc_ppo_minibatch_prepared_diag D={D} A={A} B={B} apply={apply} {mb_hash(rc, s, True)}", flush=True)
    s = mb_inputs(D, A, B, M, 3)
    pf, prep = prepared(s, D, B)
    state2 = zeros(lib.pc_ppo_epoch_state_floats(D, H, A))
    rc = lib.pc_ppo_epoch_prepared(DEV, ptr(prep), 3, B, D, H, A, *state_coef(s, zeros(ws_plain)), ptr(state2), None)
    print(f"pc_ppo_epoch_prepared D={D} A={A} B={B} n_mb=3 {mb_hash(rc, s)}", flush=True)


def large_cases(D=7, A=3, B=1029, M=1500):
    for apply in (0, 1, 2):
        s = mb_inputs(D, A, B, M, 4)
        stats = zeros(6)
        sws = zeros(lib.pc_ppo_adv_stats_workspace_doubles(3, B), torch.float64)
        rc = lib.pc_ppo_adv_stats(DEV, ptr(s["idx"]), B, 3, B, ptr(s["adv"]), ptr(stats), ptr(sws), None)
        launched(rc)
        ws = zeros(lib.pc_ppo_large_workspace_floats(DEV, B, D, H, A))
        rc = lib.pc_ppo_minibatch_large(DEV, ptr(s["idx"][1]), B, D, H, A, *samples(s), C.c_void_p(stats.data_ptr() + 8), *state_coef(s, ws),
                                        apply, None)
        print(f"pc_ppo_minibatch_large D={D} A={A} B={B} apply={apply} stats={sha(stats)} {mb_hash(rc, s)}", flush=True)


def loss_cases():
    for B in (2, 65):
        for A in (1, 16):
            gen = torch.Generator().manual_seed(100 * B + A)
            logits, values, lp, adv, ret = rnd(gen, B, A), rnd(gen, B), rnd(gen, B, scale=0.3) - 1.0, rnd(gen, B), rnd(gen, B)
            act = torch.randint(0, A, (B,), generator=gen).float().to(TDEV)
            inp = [ptr(x) for x in (logits, values, act, lp, adv, ret)] + [B, A, 0.2, 0.5, 0.001]
            out = [zeros(B * A), zeros(B), zeros(4)]
            rc = lib.pc_ppo_loss(DEV, *inp, *[ptr(x) for x in out], None)
            sync()
            print(f"pc_ppo_loss B={B} A={A} rc={rc} out={sha(*out)}", flush=True)
            for tk in (0.0, 1e-6):
                out = [zeros(B * A), zeros(B), zeros(4), zeros(_capi.PC_DIAG_FLOATS)]
                for _ in range(2):
                    rc = lib.pc_ppo_loss_diag(DEV, *inp, *[ptr(x) for x in out], tk, None)
                sync()
                print(f"pc_ppo_loss_diag B={B} A={A} target_kl={tk} rc={rc} out={sha(*out)}", flush=True)


def clip_adam_cases():
    for n in (1, 1025):
        for flag in (None, 0.0, 1.0):      # None: pc_clip_adam; else pc_clip_adam_diag with the stop flag down / up
            gen = torch.Generator().manual_seed(n)
            st = [rnd(gen, n, scale=0.1), rnd(gen, n), rnd(gen, n, scale=0.01), rnd(gen, n, scale=0.01).abs(),
                  torch.full((1,), 3.0, device=TDEV), torch.full((1,), 3e-4, device=TDEV)]
            num = [n, 1.0, 0.5, 0.9, 0.999, 1e-5]
            if flag is None:
                rc = lib.pc_clip_adam(DEV, *[ptr(x) for x in st], *num, None)
            else:
                diag = zeros(_capi.PC_DIAG_FLOATS)
                diag[4] = flag
                rc = lib.pc_clip_adam_diag(DEV, *[ptr(x) for x in st], *num, ptr(diag), None)
            sync()
            print(f"pc_clip_adam{'' if flag is None else '_diag flag=' + str(flag)} n={n} rc={rc} state={sha(*st)}", flush=True)


trainer_cases()
for D, A in ((7, 3), (30, 5)):
    small_cases(D, A)
if not args.skip_large:
    large_cases()
loss_cases()
clip_adam_cases()
print("done", flush=True)
