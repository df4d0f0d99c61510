"""Time of pc_env_rollout_sequences (K22, VecCarEnv.rollout_sequences) next to the only way to score action sequences without it -- H
chained pc_env_step_poses launches on the M x K replicated rows, the ended rows frozen with `active`, plus the tensor ops that sum the
rewards --, of one Planner.act(), and of one planner evaluation beside the trained policy fixture's.  big_track, 16 rays.  The method is
tools/safe_actions_timing.py's.

  python tools/sequences_timing.py [out.json] [reps]

  (a) rollout_sequences at M x K = 2^16 and 2^20 lanes, K = 256, H in {1, 8, 16}, F32 and F64 handles, with and without the best_*
      arrays (the second launch); states drawn uniformly over the 1280 x 720 frame (seed 0), every heading, half speed along the
      heading; the table default_rng(5).integers(0, 9, (H, K)) with the nine constant columns;
  (b) the yardstick on the same handle, states and table: the replicated rows refilled, then H x (pc_env_step_poses with `active`; the
      float64 sum of the live rows' rewards; the new `active`).  The refill alone is timed and reported beside, and so are the H
      launches alone (every row active, nothing summed: a lower bound of the chain);
  (c) one Planner.act() (horizon 16, 256 candidates) at 1024 and 16384 freshly reset envs, F32 handle;
  (d) one planner evaluation at 1024 envs (1000 steps), its eval/* scalars beside those of the trained policy fixture (sampled and
      greedy) on the same track.
Per item: the host clock around the enqueue of a few calls and a device synchronise, two warm-up windows and `reps` timed ones (median
and all), per call.  Writes profiles/sequences_timing.json by default; progress on stderr, one JSON line on stdout.  No pass / fail gate."""
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
K = 256
HORIZONS = (1, 8, 16)


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


def table(H):
    t = np.random.default_rng(5).integers(0, 9, (H, K)).astype(np.uint8)
    t[:, :9] = np.arange(9, dtype=np.uint8)
    return t


def shape_times(env, name, src, H, reps):
    """rollout_sequences and the chained yardstick on the states `src` = (px, py, vx, vy, turns) under table(H)"""
    M = src[0].numel()
    L = M * K
    tab = table(H)
    dtab = torch.from_numpy(tab).cuda()
    res = {"states": M, "candidates": K, "horizon": H, "lanes": L}
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda")
    lanes = dict(ret=new((M, K), torch.float64), steps=new((M, K), torch.int32), status=new((M, K), torch.uint8))
    full = dict(lanes, best_k=new(M, torch.int32), best_action=new(M, torch.int64), best_ret=new(M, torch.float64))
    inner = 5 if L * H <= 1 << 19 else 1
    f = lambda: env.rollout_sequences(*src, dtab, out=full)
    f()
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in full.items()}
    r = _times(f, reps, inner=inner)
    r.update({"per_lane_step_ns": r["median_s"] / (L * H) * 1e9, "every_call_gave_the_same_bits": all(torch.equal(first[k], full[k]) for k in full),
              "terminated_share": float((first["status"] == 1).float().mean()), "running_share": float((first["status"] == 0).float().mean()),
              "mean_steps": float(first["steps"].float().mean())})
    res["rollout_sequences"] = r
    res["rollout_sequences_without_best"] = _times(lambda: env.rollout_sequences(*src, dtab, out=lanes), reps, inner=inner)
    _say(name, L, "H", H, f"{r['median_s'] * 1e6:.1f} us")
    # the yardstick: H chained pc_env_step_poses launches on the replicated rows
    rep = [t.repeat_interleave(K).contiguous() for t in src]
    work = [t.clone() for t in rep]
    ng, ts = torch.zeros(L, dtype=torch.int32, device="cuda"), torch.zeros(L, dtype=torch.int32, device="cuda")
    acts = [torch.from_numpy(np.tile(tab[t], M).astype(np.int64)).cuda() for t in range(H)]
    out = (new((L, env.obs_dim), torch.float32), new(L, torch.float32)) + tuple(new(L, torch.uint8) for _ in range(3))
    ret, zero = torch.zeros(L, dtype=torch.float64, device="cuda"), torch.zeros(L, dtype=torch.float64, device="cuda")
    live, active = torch.ones(L, dtype=torch.bool, device="cuda"), torch.ones(L, dtype=torch.uint8, device="cuda")

    def refill():
        for w, s in zip(work, rep):
            w.copy_(s)
        ng.zero_()
        ts.zero_()
        ret.zero_()
        live.fill_(True)
        active.fill_(1)

    def chain():
        refill()
        for t in range(H):
            env.step_poses(*work, acts[t], next_gate=ng, time_step=ts, active=active, out=out)
            ret.add_(torch.where(live, out[1].to(torch.float64), zero))
            live.logical_and_((out[2] | out[3]) == 0)
            active.copy_(live)

    def launches():
        refill()
        for t in range(H):
            env.step_poses(*work, acts[t], next_gate=ng, time_step=ts, out=out)

    chain()
    torch.cuda.synchronize()
    agree = bool(torch.equal(ret.view(M, K), first["ret"]))
    y, c, k = _times(chain, reps), _times(refill, reps), _times(launches, reps)
    y.update({"refill_median_s": c["median_s"], "net_median_s": y["median_s"] - c["median_s"], "same_returns_as_rollout_sequences": agree,
              "launches_alone_net_median_s": k["median_s"] - c["median_s"]})
    res["chained_step_poses"] = y
    res["ratios"] = {"chain_with_refill_over_rollout_sequences": y["median_s"] / r["median_s"],
                     "chain_net_over_rollout_sequences": y["net_median_s"] / r["median_s"],
                     "launches_alone_net_over_rollout_sequences": y["launches_alone_net_median_s"] / r["median_s"]}
    _say(name, L, "H", H, f"chain {y['median_s'] * 1e6:.1f} us, net {y['net_median_s'] * 1e6:.1f} us, launches alone "
         f"{y['launches_alone_net_median_s'] * 1e6:.1f} us, agree {agree}")
    return res


def handle_times(dtype, reps):
    env = pc.VecCarEnv(1, TRACK, num_rays=RAYS, reward_scaling=0.1, dtype=dtype)
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {}
    for L in (1 << 16, 1 << 20):
        src = frame_states(L // K, gen)
        for H in HORIZONS:
            res[f"lanes_{L}_H_{H}"] = shape_times(env, dtype, src, H, reps)
    env.close()
    return res


def act_times(reps):
    res = {"horizon": 16, "candidates": K, "dtype": "f32"}
    for N in (1024, 16384):
        env = pc.VecCarEnv(N, TRACK, num_rays=RAYS, reward_scaling=0.1, dtype="f32")
        env.reset()
        planner = pc.Planner(env, horizon=16, candidates=K, seed=0)
        r = _times(lambda: planner.act(0), reps, inner=5)
        t = _times(lambda: planner.candidate_table(0), reps, inner=5)
        r["candidate_table_median_s"] = t["median_s"]
        res[f"envs_{N}"] = r
        env.close()
        _say("Planner.act", N, f"{r['median_s'] * 1e6:.1f} us, the table {t['median_s'] * 1e6:.1f} us")
    return res


def trained_agent():
    """tests/golden/policy_trained.npz (the trained fixture: 17 rays, laps big_track) into an Agent(23, 9)"""
    agent = pc.Agent(6 + pc.env.ray_count(RAYS), 9)
    f = np.load(os.path.join(ROOT, "tests", "golden", "policy_trained.npz"))
    with torch.no_grad():
        agent.load_state_dict({k: torch.from_numpy(f[k.replace(".", "_")]) for k in agent.state_dict()})
    return agent.cuda()


def evaluation_times(reps):
    res = {"n_envs": 1024, "steps": 1000, "horizon": 16, "candidates": K, "policy": "tests/golden/policy_trained.npz"}
    ev = pc.PlannerEvaluator(TRACK, n_envs=1024, num_rays=RAYS, reward_scaling=0.1, horizon=16, candidates=K, seed=0)
    r = _times(ev.run, max(3, reps // 3), warmup=1)
    r["scalars"] = ev.evaluate()
    res["planner"] = r
    ev.close()
    _say("planner evaluation", f"{r['median_s'] * 1e3:.1f} ms", r["scalars"])
    agent = trained_agent()
    for greedy in (False, True):
        pe = pc.Evaluator(agent, TRACK, n_envs=1024, num_rays=RAYS, reward_scaling=0.1, device="cuda", greedy=greedy)
        p = _times(pe.run, max(3, reps // 3), warmup=1)
        p["scalars"] = pe.evaluate()
        p["path"] = pe.last_path
        res["policy_greedy" if greedy else "policy_sampled"] = p
        pe.close()
        _say("policy evaluation, greedy" if greedy else "policy evaluation, sampled", f"{p['median_s'] * 1e3:.1f} ms", p["scalars"])
    return res


def main(out_path=os.path.join(ROOT, "profiles", "sequences_timing.json"), reps=10):
    if not torch.cuda.is_available():
        raise SystemExit("sequences_timing.py measures on the GPU: there is none")
    reps = int(reps)
    res = {"track": "big_track", "num_rays": RAYS, "reps": reps, "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around calls_per_window enqueues and a device synchronise, per call; 2 warm-up windows",
           "f32": handle_times("f32", reps), "f64": handle_times("f64", reps), "planner_act": act_times(reps),
           "evaluation_f32": evaluation_times(reps)}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(*sys.argv[1:3])
