"""Time of pc_env_observe_poses (K17, VecCarEnv.observe_poses) and of a whole PolicyLandscape.compute(), next to one pc_env_step on the
same handle as the yardstick -- big_track, 16 rays, both handle dtypes.

  python tools/observe_timing.py [out.json] [reps]

  (a) observe_poses at M = 65536 and M = 2^20 poses drawn uniformly over the 1280 x 720 frame (seed 0), every heading, half speed;
  (b) one pc_env_step of 65536 envs on the same handle (after a reset and 64 steps of random actions);
  (c) PolicyLandscape.compute() at cell_px 8 (72 x 90 x 160 = 1 036 800 poses: four chunks of observe + greedy act), F32 handle.
Per item: the host clock around the enqueue of a few calls and a device synchronise, two warm-up windows and `reps` timed ones (median
and all), per call.  Every timed observe call is checked to leave the bytes of the first.  Writes profiles/observe_timing.json by
default; one JSON line on stdout.  No pass / fail gate."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ppo_car_amd as pc  # noqa: E402

TRACK = os.path.join(ROOT, "tracks", "big_track.json")
N_ENVS, RAYS = 65536, 16


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


def poses(M, gen):
    px = torch.rand(M, generator=gen, dtype=torch.float64, device="cuda") * 1280.0
    py = torch.rand(M, generator=gen, dtype=torch.float64, device="cuda") * 720.0
    turns = torch.randint(0, 72, (M,), generator=gen, device="cuda").to(torch.int32)
    a = torch.deg2rad(5.0 * turns.to(torch.float64))
    return px, py, turns, 5.0 * torch.cos(a), 5.0 * torch.sin(a)


def handle_times(dtype, reps):
    env = pc.VecCarEnv(N_ENVS, TRACK, num_rays=RAYS, reward_scaling=0.1, dtype=dtype)
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {}
    for M in (65536, 1 << 20):
        px, py, turns, vx, vy = poses(M, gen)
        obs = torch.empty(M, env.obs_dim, device="cuda")
        col = torch.empty(M, dtype=torch.uint8, device="cuda")
        call = lambda: env.observe_poses(px, py, turns, vx=vx, vy=vy, out=obs, collides=col)
        call()
        torch.cuda.synchronize()
        first, first_col = obs.clone(), col.clone()
        r = _times(call, reps, inner=5)
        r.update({"poses": M, "per_pose_ns": r["median_s"] / M * 1e9, "collides_share": float(first_col.float().mean()),
                  "every_call_gave_the_same_bytes": bool(torch.equal(obs.view(torch.int32), first.view(torch.int32)) and torch.equal(col, first_col))})
        res[f"observe_poses_{M}"] = r
        del px, py, turns, vx, vy, obs, col, first, first_col
    env.reset()
    g2 = torch.Generator(device="cuda").manual_seed(1)
    out = (torch.empty(N_ENVS, env.obs_dim, device="cuda"), torch.empty(N_ENVS, device="cuda"), torch.empty(N_ENVS, device="cuda"),
           torch.empty(N_ENVS, device="cuda"))
    acts = torch.randint(0, 9, (64, N_ENVS), generator=g2, device="cuda")
    for t in range(64):
        env.step(acts[t], out=out)
    step = _times(lambda: env.step(acts[0], out=out), reps, inner=5)
    step.update({"n_envs": N_ENVS, "kernel": env.last_step_kernel()})
    res["env_step_65536"] = step
    res["ratios"] = {"observe_65536_over_step": res["observe_poses_65536"]["median_s"] / step["median_s"]}
    env.close()
    return res


def landscape_time(reps):
    agent = pc.Agent(6 + pc.env.ray_count(RAYS), 9).cuda()
    ls = pc.PolicyLandscape(agent, TRACK, RAYS, cell_px=8, speed=0.5, dtype="f32", device="cuda")
    r = _times(ls.compute, reps)
    torch.cuda.synchronize()
    r.update({"poses": ls.poses_per_track, "cell_px": 8, "chunks": -(-ls.poses_per_track // (1 << 18)),
              "drivable_share": float(ls.drivable.float().mean())})
    ls.close()
    return r


def main(out_path=os.path.join(ROOT, "profiles", "observe_timing.json"), reps=10):
    if not torch.cuda.is_available():
        raise SystemExit("observe_timing.py measures on the GPU: there is none")
    reps = int(reps)
    res = {"track": "big_track", "num_rays": RAYS, "reps": reps, "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around calls_per_window enqueues and a device synchronise, per call; 2 warm-up windows",
           "f32": handle_times("f32", reps), "f64": handle_times("f64", reps), "landscape_compute_f32": landscape_time(reps)}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(*sys.argv[1:3])
