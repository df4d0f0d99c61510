"""Time of the cross-entropy planner's two kernels, pc_cem_sample (K23) and pc_cem_refit (K24), beside the pc_env_rollout_sequences (K22)
launch they stand around, of one act() of each planner at equal simulation budget, and the eval/* scalars of both planners.  big_track,
16 rays, F32 handles.  The method is tools/sequences_timing.py's.

  python tools/cem_timing.py [out.json] [reps]

  (a) M = 1024 and 16384 freshly reset envs, K = 64 and 256, H = 16, E = K / 8: pc_cem_sample on uniform weights (constant columns and
      the kept column in), pc_env_rollout_sequences_state on that table (one table per state, the best_* arrays in), pc_cem_refit on
      its returns -- each timed alone, in one session, on the same tensors (the refit restarts from a copy of the weights inside the
      window; the copy is timed alone and subtracted);
  (b) one act() at 1024 and 16384 envs: Planner(candidates=256) against CEMPlanner(candidates=64, iterations=4, elites=8), horizon 16:
      256 sequences per env and step either way;
  (c) one evaluation of 1024 envs (1000 steps) under each of those two planners, its time and its eval/* scalars.
Per item: the host clock around the enqueue of a few calls and a device synchronise, two warm-up windows and `reps` timed ones (median
and all), per call.  Writes profiles/cem_timing.json by default; progress on stderr, one JSON line on stdout.  No pass / fail gate."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ppo_car_amd as pc  # noqa: E402
from ppo_car_amd._capi import check, lib  # noqa: E402

TRACK = os.path.join(ROOT, "tracks", "big_track.json")
RAYS, H = 16, 16


def _wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _times(f, reps, warmup=2, inner=1):
    """Seconds per call: `inner` calls enqueued back to back inside one timed window (a launch of tens of microseconds is not timed alone)."""
    def g():
        for _ in range(inner):
            f()
    for _ in range(warmup):
        _wall(g)
    ts = [_wall(g)[0] / inner for _ in range(reps)]
    return {"median_s": statistics.median(ts), "min_s": min(ts), "all_s": ts, "calls_per_window": inner}


def _say(*a):
    print(*a, file=sys.stderr, flush=True)


def kernel_times(M, K, reps):
    env = pc.VecCarEnv(M, TRACK, num_rays=RAYS, reward_scaling=0.1, dtype="f32")
    env.reset()
    p = pc.CEMPlanner(env, horizon=H, candidates=K, elites=K // 8, iterations=1, seed=0)
    stream = torch.cuda.current_stream().cuda_stream
    w0 = p.weights.clone()
    p.best_seq.zero_()
    sample = lambda: check(lib.pc_cem_sample(0, p.weights.data_ptr(), M, H, K, 0, 0, 1, p.best_seq.data_ptr(), None, p.table.data_ptr(), stream),
                           "pc_cem_sample")
    score = lambda: env.score_sequences(p.table, out=p.out)
    restore = lambda: p.weights.copy_(w0)

    def refit():
        restore()
        check(lib.pc_cem_refit(0, p.weights.data_ptr(), p.out["ret"].data_ptr(), p.table.data_ptr(), M, H, K, p.elites, 1, 64, None,
                               p.best_seq.data_ptr(), stream), "pc_cem_refit")

    sample(); score()
    inner = 5
    s, q, c, r = _times(sample, reps, inner=inner), _times(score, reps, inner=inner), _times(restore, reps, inner=inner), _times(refit, reps, inner=inner)
    r["weights_copy_median_s"] = c["median_s"]
    r["net_median_s"] = r["median_s"] - c["median_s"]
    both = s["median_s"] + r["net_median_s"]
    res = {"states": M, "candidates": K, "horizon": H, "elites": p.elites, "pc_cem_sample": s, "pc_env_rollout_sequences_state": q,
           "pc_cem_refit": r, "sample_plus_refit_over_rollout_sequences": both / q["median_s"],
           "running_share": float((p.out["status"] == 0).float().mean())}
    _say(f"M {M} K {K}: sample {s['median_s'] * 1e6:.1f} us, K22 {q['median_s'] * 1e6:.1f} us, refit {r['net_median_s'] * 1e6:.1f} us net of the "
         f"copy ({c['median_s'] * 1e6:.1f} us)")
    env.close()
    return res


def act_times(reps):
    res = {"horizon": H, "dtype": "f32", "shooting": {"candidates": 256}, "cem": {"candidates": 64, "iterations": 4, "elites": 8}}
    for N in (1024, 16384):
        env = pc.VecCarEnv(N, TRACK, num_rays=RAYS, reward_scaling=0.1, dtype="f32")
        env.reset()
        a = _times(lambda pl=pc.Planner(env, horizon=H, candidates=256, seed=0): pl.act(0), reps, inner=5)
        b = _times(lambda pl=pc.CEMPlanner(env, horizon=H, candidates=64, elites=8, iterations=4, seed=0): pl.act(0), reps, inner=5)
        res["shooting"][f"envs_{N}"], res["cem"][f"envs_{N}"] = a, b
        env.close()
        _say(f"act() at {N} envs: shooting {a['median_s'] * 1e6:.1f} us, cem {b['median_s'] * 1e6:.1f} us")
    return res


def evaluation_times(reps):
    res = {"n_envs": 1024, "steps": 1000, "horizon": H}
    for kind, kw in (("shooting", dict(candidates=256)), ("cem", dict(candidates=64, iterations=4, elites=8))):
        ev = pc.PlannerEvaluator(TRACK, n_envs=1024, num_rays=RAYS, reward_scaling=0.1, horizon=H, seed=0, kind=kind, **kw)
        r = _times(ev.run, max(3, reps // 3), warmup=1)
        r["scalars"] = ev.evaluate()
        r.update(kw)
        res[kind] = r
        ev.close()
        _say(kind, "evaluation", f"{r['median_s'] * 1e3:.1f} ms", r["scalars"])
    return res


def main(out_path=os.path.join(ROOT, "profiles", "cem_timing.json"), reps=10):
    if not torch.cuda.is_available():
        raise SystemExit("cem_timing.py measures on the GPU: there is none")
    reps = int(reps)
    res = {"track": "big_track", "num_rays": RAYS, "reps": reps, "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around calls_per_window enqueues and a device synchronise, per call; 2 warm-up windows",
           "kernels": {f"envs_{M}_K_{K}": kernel_times(M, K, reps) for M in (1024, 16384) for K in (64, 256)},
           "act": act_times(reps), "evaluation_f32": evaluation_times(reps)}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(*sys.argv[1:3])
