"""Time of pc_env_safe_actions (K21, VecCarEnv.safe_actions) at depths 1 .. 4 next to what did the depth-1 job before it -- nine
pc_env_step_poses launches on the same handle and states, PolicyLandscape.lookahead()'s way --, of PolicyLandscape.viability(3), and of
a shielded next to an unshielded greedy evaluation.  big_track, 16 rays.  The method is tools/step_poses_timing.py's.

  python tools/safe_actions_timing.py [out.json] [reps]

  (a) safe_actions at M = 65536 and M = 2^20 states, depths 1 .. 4, F32 and F64 handles, for two populations:
        frame     states drawn uniformly over the 1280 x 720 frame (seed 0), every heading, half speed along the heading;
        drivable  the drivable poses of the PolicyLandscape grid at cell_px 8 (half speed along the heading), in grid order, repeated
                  cyclically up to M
  (b) the yardstick at depth 1: for each of the 9 actions, fresh copies of the seven state arrays and one pc_env_step_poses (the copies
      are timed alone as well and reported beside: they are launch-bound and overlap the kernels);
  (c) one PolicyLandscape.viability(3) at cell_px 8 (1 036 800 poses, four chunks), F32 handle, next to one lookahead();
  (d) one greedy evaluation of 1024 envs on the per-step path (1000 steps) with shield_depth 0 and 2, the trained policy fixture.
Per item: the host clock around the enqueue of a few calls and a device synchronise, two warm-up windows and `reps` timed ones (median
and all), per call.  Writes profiles/safe_actions_timing.json by default; progress on stderr, one JSON line on stdout.  No pass / fail gate."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ppo_car_amd as pc  # noqa: E402

TRACK = os.path.join(ROOT, "tracks", "big_track.json")
RAYS = 16


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


def frame_states(M, gen):
    px = torch.rand(M, generator=gen, dtype=torch.float64, device="cuda") * 1280.0
    py = torch.rand(M, generator=gen, dtype=torch.float64, device="cuda") * 720.0
    turns = torch.randint(0, 72, (M,), generator=gen, device="cuda").to(torch.int32)
    a = torch.deg2rad(5.0 * turns.to(torch.float64))
    return px, py, 5.0 * torch.cos(a), 5.0 * torch.sin(a), turns


def drivable_states(M, grid):
    idx = torch.arange(M, device="cuda") % grid[0].numel()
    return tuple(t[idx].contiguous() for t in grid)


def population_times(env, name, src, reps):
    """safe_actions at depths 1 .. 4 and the nine-launch yardstick on the states `src` = (px, py, vx, vy, turns)."""
    M = src[0].numel()
    res = {"states": M}
    safe = torch.empty(M, 9, dtype=torch.uint8, device="cuda")
    for d in (1, 2, 3, 4):
        f = lambda: env.safe_actions(*src, depth=d, out=safe)
        f()
        torch.cuda.synchronize()
        first = safe.clone()
        r = _times(f, reps, inner=5 if d == 1 else 1)
        count = first.sum(1)
        r.update({"per_state_ns": r["median_s"] / M * 1e9, "every_call_gave_the_same_bytes": bool(torch.equal(first, safe)),
                  "empty_share": float((count == 0).float().mean()), "full_share": float((count == 9).float().mean())})
        res[f"safe_actions_depth_{d}"] = r
        _say(name, M, "depth", d, f"{r['median_s'] * 1e6:.1f} us")
        if d == 1:
            mask1 = first.clone()
    # the yardstick: lookahead()'s nine launches, each on fresh copies of the state
    work = [t.clone() for t in src]
    ng, ts = torch.zeros(M, dtype=torch.int32, device="cuda"), torch.zeros(M, dtype=torch.int32, device="cuda")
    acts = torch.empty(M, dtype=torch.int64, device="cuda")
    out = (torch.empty(M, env.obs_dim, device="cuda"), torch.empty(M, device="cuda")) + tuple(torch.empty(M, dtype=torch.uint8, device="cuda")
                                                                                              for _ in range(3))
    term = torch.empty(M, 9, dtype=torch.uint8, device="cuda")

    def refill(a):
        for w, s in zip(work, src):
            w.copy_(s)
        ng.zero_()
        ts.zero_()
        acts.fill_(a)

    def nine_steps():
        for a in range(9):
            refill(a)
            env.step_poses(*work, acts, next_gate=ng, time_step=ts, out=out)
            term[:, a].copy_(out[2])

    def nine_refills():
        for a in range(9):
            refill(a)
            term[:, a].copy_(out[2])

    nine_steps()
    torch.cuda.synchronize()
    agree = bool(torch.equal(term == 0, mask1 != 0))
    y = _times(nine_steps, reps)
    c = _times(nine_refills, reps)
    y.update({"copies_median_s": c["median_s"], "net_median_s": y["median_s"] - c["median_s"], "same_mask_as_depth_1": agree})
    res["nine_step_poses"] = y
    d1 = res["safe_actions_depth_1"]["median_s"]
    res["ratios"] = {"nine_step_poses_with_copies_over_depth_1": y["median_s"] / d1, "nine_step_poses_net_over_depth_1": y["net_median_s"] / d1}
    for d in (2, 3, 4):
        res["ratios"][f"depth_{d}_over_depth_1"] = res[f"safe_actions_depth_{d}"]["median_s"] / d1
    _say(name, M, "nine step_poses", f"{y['median_s'] * 1e6:.1f} us, net {y['net_median_s'] * 1e6:.1f} us, agree {agree}")
    return res


def handle_times(dtype, grid, reps):
    env = pc.VecCarEnv(1, TRACK, num_rays=RAYS, reward_scaling=0.1, dtype=dtype)
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {}
    for M in (65536, 1 << 20):
        res[f"frame_{M}"] = population_times(env, f"{dtype} frame", frame_states(M, gen), reps)
        res[f"drivable_{M}"] = population_times(env, f"{dtype} drivable", drivable_states(M, grid), reps)
    env.close()
    return res


def trained_agent():
    """tests/golden/policy_trained.npz (the trained fixture: 17 rays, laps big_track) into an Agent(23, 9)"""
    agent = pc.Agent(6 + pc.env.ray_count(RAYS), 9)
    f = np.load(os.path.join(ROOT, "tests", "golden", "policy_trained.npz"))
    with torch.no_grad():
        agent.load_state_dict({k: torch.from_numpy(f[k.replace(".", "_")]) for k in agent.state_dict()})
    return agent.cuda()


def landscape(agent):
    ls = pc.PolicyLandscape(agent, TRACK, RAYS, cell_px=8, speed=0.5, dtype="f32", device="cuda")
    ls.compute()
    torch.cuda.synchronize()
    ok = ls.drivable.view(-1)
    grid = tuple(t[ok].contiguous() for t in ls.poses()[:5])
    return ls, grid


def landscape_times(ls, reps):
    v = _times(lambda: ls.viability(3), reps)
    v.update({"depth": 3, "doomed_poses": int(ls.doomed.sum()), "avoidable_late_poses": int(ls.avoidable_late.sum())})
    la = _times(ls.lookahead, reps)
    v1 = _times(lambda: ls.viability(1), reps)
    torch.cuda.synchronize()
    return {"poses": ls.poses_per_track, "drivable_poses": int(ls.drivable.sum()), "cell_px": 8, "chunks": -(-ls.poses_per_track // (1 << 18)),
            "viability_3": v, "viability_1": v1, "lookahead": la, "lookahead_over_viability_1": la["median_s"] / v1["median_s"],
            "policy": "tests/golden/policy_trained.npz"}


def evaluation_times(agent, reps):
    res = {"n_envs": 1024, "steps": 1000, "greedy": True, "path": "steps", "policy": "tests/golden/policy_trained.npz"}
    for depth in (0, 2):
        ev = pc.Evaluator(agent, TRACK, n_envs=1024, num_rays=RAYS, reward_scaling=0.1, device="cuda", greedy=True, rollout_kernel="auto",
                          shield_depth=depth)
        r = _times(ev.run, max(3, reps // 2), warmup=1)
        r["scalars"] = ev.evaluate()
        res[f"shield_depth_{depth}"] = r
        ev.close()
        _say("evaluation, shield", depth, f"{r['median_s'] * 1e3:.1f} ms")
    res["shielded_over_unshielded"] = res["shield_depth_2"]["median_s"] / res["shield_depth_0"]["median_s"]
    return res


def main(out_path=os.path.join(ROOT, "profiles", "safe_actions_timing.json"), reps=10):
    if not torch.cuda.is_available():
        raise SystemExit("safe_actions_timing.py measures on the GPU: there is none")
    reps = int(reps)
    agent = trained_agent()
    ls, grid = landscape(agent)
    res = {"track": "big_track", "num_rays": RAYS, "reps": reps, "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around calls_per_window enqueues and a device synchronise, per call; 2 warm-up windows",
           "f32": handle_times("f32", grid, reps), "f64": handle_times("f64", grid, reps), "landscape_f32": landscape_times(ls, reps),
           "evaluation_f32": evaluation_times(agent, reps)}
    ls.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(*sys.argv[1:3])
