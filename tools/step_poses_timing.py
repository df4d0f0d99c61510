"""Time of pc_env_step_poses (K20, VecCarEnv.step_poses) next to pc_env_observe_poses on the very same poses and one pc_env_step on the
same handle, and of PolicyLandscape.survival(64) / lookahead() -- big_track, 16 rays, both handle dtypes.  The method is
tools/observe_timing.py's.

  python tools/step_poses_timing.py [out.json] [reps]

  (a) step_poses at M = 65536 and M = 2^20 states drawn uniformly over the 1280 x 720 frame (seed 0), every heading, half speed, random
      actions; every timed call steps fresh copies of the same states (the copies are made outside the timed window's kernel, but their
      cost is inside it: it is measured alone and reported beside, as `state_copy`);
  (b) observe_poses on those poses, in the same session;
  (c) one pc_env_step of 65536 envs on the same handle (after a reset and 64 steps of random actions);
  (d) PolicyLandscape.survival(64) and lookahead() at cell_px 8 (1 036 800 poses, four chunks), F32 handle.
Per item: the host clock around the enqueue of a few calls and a device synchronise, two warm-up windows and `reps` timed ones (median
and all), per call.  Writes profiles/step_poses_timing.json by default; one JSON line on stdout.  No pass / fail gate."""
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
        acts = torch.randint(0, 9, (M,), generator=gen, device="cuda")
        obs = torch.empty(M, env.obs_dim, device="cuda")
        col = torch.empty(M, dtype=torch.uint8, device="cuda")
        out = (obs, torch.empty(M, device="cuda")) + tuple(torch.empty(M, dtype=torch.uint8, device="cuda") for _ in range(3))
        src = (px, py, vx, vy, turns)
        work = [t.clone() for t in src]
        ng, ts = torch.zeros(M, dtype=torch.int32, device="cuda"), torch.zeros(M, dtype=torch.int32, device="cuda")

        def refill():
            for w, s in zip(work, src):
                w.copy_(s)
            ng.zero_()
            ts.zero_()

        def step():
            refill()
            env.step_poses(work[0], work[1], work[2], work[3], work[4], acts, next_gate=ng, time_step=ts, out=out)

        step()
        torch.cuda.synchronize()
        first = [t.clone() for t in out] + [w.clone() for w in work]
        r = _times(step, reps, inner=5)
        same = all(torch.equal(a, b) for a, b in zip(first, list(out) + work))
        copy = _times(refill, reps, inner=5)
        net = r["median_s"] - copy["median_s"]
        r.update({"states": M, "state_copy_median_s": copy["median_s"], "net_median_s": net, "net_per_state_ns": net / M * 1e9,
                  "terminated_share": float(out[2].float().mean()), "every_call_gave_the_same_bytes": bool(same)})
        res[f"step_poses_{M}"] = r
        o = _times(lambda: env.observe_poses(px, py, turns, vx=vx, vy=vy, out=obs, collides=col), reps, inner=5)
        o.update({"poses": M, "per_pose_ns": o["median_s"] / M * 1e9})
        res[f"observe_poses_{M}"] = o
        # (the seven small copies are launch-bound and overlap the step kernel: the truth lies between the two ratios)
        res.setdefault("ratios", {})[f"step_net_over_observe_{M}"] = net / o["median_s"]
        res["ratios"][f"step_with_copies_over_observe_{M}"] = r["median_s"] / o["median_s"]
        del px, py, turns, vx, vy, obs, col, out, work, first, acts
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
    res["ratios"]["step_poses_net_65536_over_env_step"] = res["step_poses_65536"]["net_median_s"] / step["median_s"]
    env.close()
    return res


def landscape_times(reps):
    agent = pc.Agent(6 + pc.env.ray_count(RAYS), 9).cuda()
    ls = pc.PolicyLandscape(agent, TRACK, RAYS, cell_px=8, speed=0.5, dtype="f32", device="cuda")
    ls.compute()
    s = _times(lambda: ls.survival(64), reps)
    s.update({"horizon": 64, "surviving_share": float((ls.survived == 64).float().mean())})
    la = _times(ls.lookahead, reps)
    torch.cuda.synchronize()
    la.update({"avoidable_poses": int(ls.avoidable.sum())})
    res = {"poses": ls.poses_per_track, "cell_px": 8, "chunks": -(-ls.poses_per_track // (1 << 18)), "survival_64": s, "lookahead": la,
           "policy": "untrained Agent (default initialisation)"}
    ls.close()
    return res


def main(out_path=os.path.join(ROOT, "profiles", "step_poses_timing.json"), reps=10):
    if not torch.cuda.is_available():
        raise SystemExit("step_poses_timing.py measures on the GPU: there is none")
    reps = int(reps)
    res = {"track": "big_track", "num_rays": RAYS, "reps": reps, "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around calls_per_window enqueues and a device synchronise, per call; 2 warm-up windows",
           "f32": handle_times("f32", reps), "f64": handle_times("f64", reps), "landscape_f32": landscape_times(reps)}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(*sys.argv[1:3])
