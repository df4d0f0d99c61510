"""Timing of the large-minibatch update (PPOConfig.large_minibatch) against the path the same configuration takes without the flag
(the torch-op step under HIP graphs), on one box, the two sides alternating.

  python tools/large_minibatch_timing.py epoch [pairs] [out.json]   one epoch's update (device events around Trainer.update) at
        n_envs 65536, n_steps 1024, train_iters 40, batch_size 2048 / 8192 / 65536, flag off and on alternating; the host time of
        PPOLearner.draw_indices per epoch at each size; medians and ranges -> profiles/large_minibatch_timing.json
  python tools/large_minibatch_timing.py kernels <batch_size>       three updates with the flag on and nothing else: the target of a
        `rocprofv3 --kernel-trace --stats -- python tools/large_minibatch_timing.py kernels B` run of its own (per-kernel times)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ppo_car_amd._capi import lib  # noqa: E402
from ppo_car_amd.ppo import PPOConfig, Trainer  # noqa: E402

N_ENVS, N_STEPS, ITERS = 65536, 1024, 40
SIZES = (2048, 8192, 65536)


def trainer(B, flag):
    cfg = PPOConfig(n_envs=N_ENVS, n_steps=N_STEPS, batch_size=B, train_iters=ITERS, track=os.path.join(ROOT, "tracks", "big_track.json"),
                    num_rays=16, seed=3, large_minibatch=flag)
    tr = Trainer(cfg, device="cuda:0")
    tr.rollout()
    torch.cuda.synchronize()
    return tr


def timed_update(tr):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    tr.update()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "runs": [round(x, 4) for x in xs]}


def epoch(pairs, out):
    res = {"shape": {"n_envs": N_ENVS, "n_steps": N_STEPS, "train_iters": ITERS, "num_rays": 16}, "pairs": pairs,
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for B in SIZES:
        off, on = trainer(B, False), trainer(B, True)
        assert on.learner.large and not off.learner.large and not off.learner.fused
        for tr in (off, on):          # graph capture and warm-up outside the timed runs
            for _ in range(2):
                timed_update(tr)
        t_off, t_on = [], []
        for _ in range(pairs):
            t_off.append(timed_update(off))
            t_on.append(timed_update(on))
        draws = []
        for _ in range(pairs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            on.learner.draw_indices(N_ENVS * N_STEPS)
            draws.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        res["sizes"][str(B)] = {"minibatches_per_epoch": ITERS * on.learner.n_minibatches, "workgroups": lib.pc_ppo_large_parts(0, B),
                                "flag_off_torch_graphs": summary(t_off), "flag_on_kernels": summary(t_on),
                                "draw_indices_host": summary(draws)}
        print(B, json.dumps(res["sizes"][str(B)]), flush=True)
        off.close()
        on.close()
        del off, on
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def kernels(B):
    tr = trainer(B, True)
    for _ in range(3):
        tr.update()
    torch.cuda.synchronize()
    tr.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "epoch"
    if mode == "epoch":
        epoch(int(sys.argv[2]) if len(sys.argv) > 2 else 5, sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "large_minibatch_timing.json"))
    elif mode == "kernels":
        kernels(int(sys.argv[2]))
    else:
        raise SystemExit(__doc__)
