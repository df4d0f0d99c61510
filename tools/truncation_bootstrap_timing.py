"""Timing of the truncation bootstrap (PPOConfig.truncation_bootstrap = "final_obs") against the reference bootstrap, on one device,
the two variants alternating.

  python tools/truncation_bootstrap_timing.py rollout [N] [T] [reps]   the persistent rollout with and without the final-observation
                                                                     capture (pc_rollout_final_obs / pc_rollout), the trained policy
                                                                     (tests/golden/policy_trained.npz) from staggered time steps, so
                                                                     that every env that survives truncates once per 1000 steps
  python tools/truncation_bootstrap_timing.py kernels [T] [N] [reps]   K3 gae_kernel<1,0,0,0> against K3b gae_kernel<1,1,0,0> (and
                                                                     <1,1,1,0> against K3e <1,0,1,0>) on the same rows
  python tools/truncation_bootstrap_timing.py epoch [N] [epochs]       Trainer epochs at the benchmark's shape, off and on

One JSON line per mode on stdout; times are medians of HIP-event intervals.  The JSON keys keep the names the kernels had when
profiles/truncation_bootstrap_timing.json was recorded: gae_kernel = K3, gae_bootstrap_kernel = K3b, gae_episode_kernel = K3e,
gae_bootstrap_episode_kernel = K3b with the episode statistics."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ppo_car_amd import _capi  # noqa: E402

TRACK = os.path.join(ROOT, "tracks", "big_track.json")


def _timed(f):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def rollout(N=65536, T=1024, reps=6):
    from oracle.scenarios import load_trained_policy
    from ppo_car_amd.ppo import PPOConfig, Trainer
    tr = {}
    for on in (False, True):
        cfg = PPOConfig(n_envs=N, n_steps=T, num_rays=16, track=TRACK, rollout_kernel="mega", seed=5,
                        truncation_bootstrap="final_obs" if on else "reference")
        t = Trainer(cfg, device="cuda")
        load_trained_policy(t.agent)
        st = t.envs.get_state()
        st["time_step"] = np.arange(N) % 1000      # staggered: the truncations spread over the rollout's steps
        t.envs.set_state(**st)
        tr[on] = t
    for t in tr.values():
        t.rollout()
    times = {False: [], True: []}
    truncs = {False: [], True: []}
    kernel = None
    for i in range(reps):
        for on in ((False, True) if i % 2 == 0 else (True, False)):
            times[on].append(_timed(tr[on].rollout))
            b = tr[on].buffer
            truncs[on].append(int(b.trunc_buf[1:].sum() + tr[on].next_trunc.sum()))
            kernel = tr[on].envs.last_rollout_kernel()
    for t in tr.values():
        t.close()
    off, on = statistics.median(times[False]), statistics.median(times[True])
    return {"mode": "rollout", "N": N, "T": T, "reps": reps, "kernel": kernel, "off_ms": off, "on_ms": on, "on_over_off": on / off,
            "off_all_ms": times[False], "on_all_ms": times[True], "truncations_per_rollout": truncs[True]}


def kernels(T=1024, N=65536, reps=20):
    g = torch.Generator(device="cuda").manual_seed(0)
    rew = (torch.randint(0, 3, (T, N), generator=g, device="cuda").float() * 0.1).contiguous()
    val = torch.randn(T, N, generator=g, device="cuda")
    term = (torch.rand(T, N, generator=g, device="cuda") < 0.002).float()
    trunc = (torch.rand(T, N, generator=g, device="cuda") < 0.001).float()
    lv, lt, ltr = torch.randn(N, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    K = -(-T // _capi.PC_TIME_LIMIT)
    fv = torch.randn(K, N, generator=g, device="cuda")
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    carry = torch.zeros(4, N, dtype=torch.float64, device="cuda")
    out = torch.zeros(7, N, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    calls = {
        "gae_kernel": lambda: _capi.lib.pc_gae(0, p(rew), p(val), p(term), p(trunc), p(lv), p(lt), p(ltr), 0.99, 0.95, T, N, p(adv), p(ret), s),
        "gae_bootstrap_kernel": lambda: _capi.lib.pc_gae_bootstrap(0, p(rew), p(val), p(term), p(trunc), p(lv), p(lt), p(ltr), p(fv), K, 0.99,
                                                                   0.95, T, N, p(adv), p(ret), 1.0, None, None, s),
        "gae_episode_kernel": lambda: _capi.lib.pc_gae_episodes(0, p(rew), p(val), p(term), p(trunc), p(lv), p(lt), p(ltr), 0.99, 0.95, T, N,
                                                                p(adv), p(ret), 0.1, p(carry), p(out), s),
        "gae_bootstrap_episode_kernel": lambda: _capi.lib.pc_gae_bootstrap(0, p(rew), p(val), p(term), p(trunc), p(lv), p(lt), p(ltr), p(fv),
                                                                           K, 0.99, 0.95, T, N, p(adv), p(ret), 0.1, p(carry), p(out), s),
    }
    times = {k: [] for k in calls}
    for _ in range(3):
        for f in calls.values():
            _capi.check(f(), "warm-up")
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _capi.check(f(), k)
            e1.record()
            times[k].append((e0, e1))
    torch.cuda.synchronize()
    res = {"mode": "kernels", "T": T, "N": N, "reps": reps, "truncated_fraction": float(trunc.mean())}
    for k, ev in times.items():
        res[k] = {"median_ms": statistics.median(a.elapsed_time(b) for a, b in ev)}
    res["bootstrap_over_gae"] = res["gae_bootstrap_kernel"]["median_ms"] / res["gae_kernel"]["median_ms"]
    res["bootstrap_episodes_over_episodes"] = res["gae_bootstrap_episode_kernel"]["median_ms"] / res["gae_episode_kernel"]["median_ms"]
    return res


def epoch(N=65536, epochs=8):
    from ppo_car_amd.ppo import PPOConfig, Trainer
    base = dict(n_envs=N, n_steps=1024, num_rays=16, batch_size=512, train_iters=40, track=TRACK)
    tr = {False: Trainer(PPOConfig(**base), device="cuda"), True: Trainer(PPOConfig(truncation_bootstrap="final_obs", **base), device="cuda")}
    for _ in range(2):
        for t in tr.values():
            t.run_epoch()
    times = {False: [], True: []}
    for i in range(epochs):
        for on in ((False, True) if i % 2 == 0 else (True, False)):
            times[on].append(_timed(lambda: tr[on].run_epoch(sync=False)))
    for t in tr.values():
        t.close()
    off, on = statistics.median(times[False]), statistics.median(times[True])
    return {"mode": "epoch", "N": N, "epochs": epochs, "off_ms": off, "on_ms": on, "on_over_off": on / off,
            "off_all_ms": times[False], "on_all_ms": times[True]}


if __name__ == "__main__":
    mode, args = sys.argv[1], [int(a) for a in sys.argv[2:]]
    print(json.dumps({"rollout": rollout, "kernels": kernels, "epoch": epoch}[mode](*args)), flush=True)
