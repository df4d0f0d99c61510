"""Timing of the episode statistics (K3e) against the GAE scan it rides on, and of a whole epoch with and without them.

  python tools/episode_stats_timing.py kernels [T] [N] [reps]   pc_gae, pc_gae_episodes and pc_episode_stats (Buffer layout) launched in
                                                               turn on the same rows (gae_kernel<1,0,0,0>, <1,0,1,0>, <0,0,1,0>),
                                                               device-event times per launch (run it under `rocprofv3
                                                               --kernel-trace --stats` for the kernel times themselves)
  python tools/episode_stats_timing.py epoch [N] [epochs]       Trainer epochs at the benchmark's shape with PPOConfig.episode_stats off
                                                               and on, alternating on one device

One JSON line per mode on stdout.  HBM bytes are counted from the shapes: K3 reads rew, val, term, trunc and writes adv, ret (24 B per
transition); K3e fused adds 88 B per env (carry in / out, out in / out); K3e alone reads 12 B per transition.  The JSON keys keep the
names the kernels had when profiles/episode_stats_timing.json was recorded: gae_kernel = K3, gae_episode_kernel = K3e fused,
episode_kernel = K3e alone."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ppo_car_amd import _capi  # noqa: E402

HBM_BYTES_PER_S = 8.0e12      # MI355X peak HBM3E bandwidth


def kernels(T=1024, N=65536, reps=20):
    g = torch.Generator(device="cuda").manual_seed(0)
    rew = (torch.randint(0, 3, (T, N), generator=g, device="cuda").float() * 0.1).contiguous()
    val = torch.randn(T, N, generator=g, device="cuda")
    term = (torch.rand(T, N, generator=g, device="cuda") < 0.002).float()
    trunc = (torch.rand(T, N, generator=g, device="cuda") < 0.001).float()
    lv, lt, ltr = torch.randn(N, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    carry = torch.zeros(4, N, dtype=torch.float64, device="cuda")
    out = torch.zeros(7, N, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    calls = {
        "gae_kernel": lambda: _capi.lib.pc_gae(0, p(rew), p(val), p(term), p(trunc), p(lv), p(lt), p(ltr), 0.99, 0.95, T, N, p(adv), p(ret), s),
        "gae_episode_kernel": lambda: _capi.lib.pc_gae_episodes(0, p(rew), p(val), p(term), p(trunc), p(lv), p(lt), p(ltr), 0.99, 0.95, T, N,
                                                                p(adv), p(ret), 0.1, p(carry), p(out), s),
        "episode_kernel": lambda: _capi.lib.pc_episode_stats(0, p(rew), p(term), p(trunc), p(lt), p(ltr), T, N, _capi.PC_EPISODE_BUFFER, 0.1,
                                                             p(carry), p(out), s),
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
    nbytes = {"gae_kernel": 24 * T * N, "gae_episode_kernel": 24 * T * N + 88 * N, "episode_kernel": 12 * T * N + 88 * N + 8 * N}
    res = {"mode": "kernels", "T": T, "N": N, "reps": reps}
    for k, ev in times.items():
        ms = statistics.median(a.elapsed_time(b) for a, b in ev)
        res[k] = {"median_ms": ms, "bytes": nbytes[k], "hbm_share": nbytes[k] / HBM_BYTES_PER_S / (ms * 1e-3)}
    res["fused_over_gae"] = res["gae_episode_kernel"]["median_ms"] / res["gae_kernel"]["median_ms"]
    res["fused_over_sum"] = res["gae_episode_kernel"]["median_ms"] / (res["gae_kernel"]["median_ms"] + res["episode_kernel"]["median_ms"])
    return res


def epoch(N=65536, epochs=8):
    from ppo_car_amd.ppo import PPOConfig, Trainer
    base = dict(n_envs=N, n_steps=1024, num_rays=16, batch_size=512, train_iters=40, track=os.path.join(ROOT, "tracks", "big_track.json"))
    tr = {False: Trainer(PPOConfig(**base), device="cuda"), True: Trainer(PPOConfig(episode_stats=True, **base), device="cuda")}
    for _ in range(2):
        for t in tr.values():
            t.run_epoch()
    times = {False: [], True: []}
    rows = {}
    for i in range(epochs):
        for on in ((False, True) if i % 2 == 0 else (True, False)):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr[on].run_epoch(sync=False)
            e1.record()
            torch.cuda.synchronize()
            times[on].append(e0.elapsed_time(e1))
    rows = tr[True].run_epoch()
    for t in tr.values():
        t.close()
    off, on = statistics.median(times[False]), statistics.median(times[True])
    return {"mode": "epoch", "N": N, "epochs": epochs, "off_ms": off, "on_ms": on, "on_over_off": on / off,
            "off_all_ms": times[False], "on_all_ms": times[True],
            "last_row": {k: v for k, v in rows.items() if k.startswith("charts/episod") or k.endswith("per_episode")}}


if __name__ == "__main__":
    mode, args = sys.argv[1], [int(a) for a in sys.argv[2:]]
    print(json.dumps(kernels(*args) if mode == "kernels" else epoch(*args)), flush=True)
