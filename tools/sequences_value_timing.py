"""Time of pc_env_rollout_sequences_value (K25, the policy step, K26; VecCarEnv.rollout_sequences with gamma, bootstrap, agent) next to
its parts, and whether a short horizon with the critic's value does what a long one does without.  big_track, 16 rays, the trained
fixture (tests/golden/policy_trained.npz).  The method is tools/sequences_timing.py's.

  python tools/sequences_value_timing.py [out.json] [reps]

  (a) the new call at M x K = 2^16 and 2^20 lanes, K = 256, H in {4, 16}, F32 and F64 handles, gamma 0.99, bootstrap running; states drawn
      uniformly over the 1280 x 720 frame (seed 0), every heading, half speed along the heading; the table
      default_rng(5).integers(0, 9, (H, K)) with the nine constant columns.  Beside it on the same handle, states and table:
        - pc_env_rollout_sequences (K22) alone, which computes no discount, no observation and no value;
        - the new call without a policy (K25 + K26: the discount and the end observation, no value);
        - the only way to the same numbers without the new entry point: the replicated rows refilled, H x (pc_env_step_poses with `active`;
          the discounted float64 sum and the last live observation kept with tensor ops; the new `active`), the policy step
          (Agent.act(greedy=True), the image packed beforehand) and the combination and argmax in torch.  The refill alone is timed and
          reported beside.  Its `ret` bits are compared with the new call's once;
  (b) PlannerEvaluator(kind="cem") at 1024 envs (64 sequences, 8 elites, 4 rounds per step): H = 16 without a critic beside H = 4 and
      H = 8 with gamma 0.99, bootstrap running, and H = 4 and H = 8 without a critic (what the shorter horizon alone does): the eval/*
      scalars and the wall time of one evaluation (1000 planning steps).
Per item: the host clock around the enqueue of a few calls and a device synchronise, two warm-up windows and `reps` timed ones (median
and all), per call.  Writes profiles/sequences_value_timing.json by default; progress on stderr, one JSON line on stdout.  No pass / fail
gate."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ppo_car_amd as pc  # noqa: E402
from sequences_timing import K, RAYS, TRACK, _say, _times, frame_states, trained_agent  # noqa: E402

HORIZONS = (4, 16)
GAMMA, BOOTSTRAP = 0.99, "running"


def table(H):
    t = np.random.default_rng(5).integers(0, 9, (H, K)).astype(np.uint8)
    t[:, :9] = np.arange(9, dtype=np.uint8)
    return t


def shape_times(env, agent, name, src, H, reps):
    M = src[0].numel()
    L, D = M * K, env.obs_dim
    tab = table(H)
    dtab = torch.from_numpy(tab).cuda()
    res = {"states": M, "candidates": K, "horizon": H, "lanes": L, "gamma": GAMMA, "bootstrap": BOOTSTRAP}
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda")
    k22 = dict(ret=new((M, K), torch.float64), steps=new((M, K), torch.int32), status=new((M, K), torch.uint8), best_k=new(M, torch.int32),
               best_action=new(M, torch.int64), best_ret=new(M, torch.float64))
    nop = dict({k: torch.empty_like(v) for k, v in k22.items()}, end_obs=new((M, K, D), torch.float32))
    full = dict({k: torch.empty_like(v) for k, v in nop.items()}, end_value=new((M, K), torch.float32))
    inner = 5 if L * H <= 1 << 19 else 1
    agent.pack_policy()
    f = lambda: env.rollout_sequences(*src, dtab, out=full, gamma=GAMMA, bootstrap=BOOTSTRAP, agent=agent)
    f()
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in full.items()}
    r = _times(f, reps, inner=inner)
    r.update({"per_lane_step_ns": r["median_s"] / (L * H) * 1e9, "every_call_gave_the_same_bits": all(torch.equal(first[k], full[k]) for k in full),
              "terminated_share": float((first["status"] == 1).float().mean()), "running_share": float((first["status"] == 0).float().mean()),
              "mean_steps": float(first["steps"].float().mean())})
    res["value_call"] = r
    res["value_call_packed_beforehand"] = _times(lambda: env.rollout_sequences(*src, dtab, out=full, gamma=GAMMA, bootstrap=BOOTSTRAP, agent=agent,
                                                                               repack=False), reps, inner=inner)
    res["value_call_without_a_policy"] = _times(lambda: env.rollout_sequences(*src, dtab, out=nop, gamma=GAMMA), reps, inner=inner)
    res["k22_alone"] = _times(lambda: env.rollout_sequences(*src, dtab, out=k22), reps, inner=inner)
    x = first["end_obs"].view(L, D)
    pol = (new(L, torch.int64), new(L, torch.float32), new(L, torch.float32))
    res["policy_step_alone"] = _times(lambda: agent.act(x, out_action=pol[0], out_logprob=pol[1], out_value=pol[2], repack=False, greedy=True),
                                      reps, inner=inner)
    _say(name, L, "H", H, f"value call {r['median_s'] * 1e6:.1f} us, without a policy {res['value_call_without_a_policy']['median_s'] * 1e6:.1f} us, "
         f"K22 {res['k22_alone']['median_s'] * 1e6:.1f} us, policy step {res['policy_step_alone']['median_s'] * 1e6:.1f} us")
    # the yardstick: H chained pc_env_step_poses launches on the replicated rows, the policy step, the combination in torch
    rep = [t.repeat_interleave(K).contiguous() for t in src]
    work = [t.clone() for t in rep]
    ng, ts = torch.zeros(L, dtype=torch.int32, device="cuda"), torch.zeros(L, dtype=torch.int32, device="cuda")
    acts = [torch.from_numpy(np.tile(tab[t], M).astype(np.int64)).cuda() for t in range(H)]
    out = (new((L, D), torch.float32), new(L, torch.float32)) + tuple(new(L, torch.uint8) for _ in range(3))
    ret, disc, zero = (torch.zeros(L, dtype=torch.float64, device="cuda") for _ in range(3))
    live, active = torch.ones(L, dtype=torch.bool, device="cuda"), torch.ones(L, dtype=torch.uint8, device="cuda")
    end_obs = new((L, D), torch.float32)
    best = {}

    def refill():
        for w, s in zip(work, rep):
            w.copy_(s)
        ng.zero_()
        ts.zero_()
        ret.zero_()
        disc.fill_(1.0)
        live.fill_(True)
        active.fill_(1)

    def chain():
        refill()
        for t in range(H):
            env.step_poses(*work, acts[t], next_gate=ng, time_step=ts, active=active, out=out)
            ret.add_(torch.where(live, disc * out[1].to(torch.float64), zero))      # a rounded product, then a rounded sum
            disc.copy_(torch.where(live, disc * GAMMA, disc))
            end_obs.copy_(torch.where(live[:, None], out[0], end_obs))
            live.logical_and_((out[2] | out[3]) == 0)
            active.copy_(live)
        agent.act(end_obs, out_action=pol[0], out_logprob=pol[1], out_value=pol[2], repack=False, greedy=True)
        total = torch.where(live, ret + disc * pol[2].to(torch.float64), ret).view(M, K)      # bootstrap running: the lanes still live
        best["ret"] = total
        best["best_ret"], best["best_k"] = total.max(1)

    chain()
    torch.cuda.synchronize()
    agree = bool(torch.equal(best["ret"], first["ret"]))
    agree_obs = bool(torch.equal(end_obs.view(M, K, D), first["end_obs"]))
    y, c = _times(chain, reps), _times(refill, reps)
    y.update({"refill_median_s": c["median_s"], "net_median_s": y["median_s"] - c["median_s"], "same_ret_bits_as_the_value_call": agree,
              "same_end_obs_bits_as_the_value_call": agree_obs,
              "ret_entries_that_differ": int((best["ret"] != first["ret"]).sum())})
    res["chained_step_poses_policy_step_and_torch"] = y
    res["ratios"] = {"value_call_over_k22_alone": r["median_s"] / res["k22_alone"]["median_s"],
                     "chain_with_refill_over_value_call": y["median_s"] / r["median_s"],
                     "chain_net_over_value_call": y["net_median_s"] / r["median_s"]}
    _say(name, L, "H", H, f"chain {y['median_s'] * 1e6:.1f} us, net {y['net_median_s'] * 1e6:.1f} us, same ret bits {agree}, same end_obs bits {agree_obs}")
    return res


def handle_times(dtype, agent, reps):
    env = pc.VecCarEnv(1, TRACK, num_rays=RAYS, reward_scaling=0.1, dtype=dtype)
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {}
    for L in (1 << 16, 1 << 20):
        src = frame_states(L // K, gen)
        for H in HORIZONS:
            res[f"lanes_{L}_H_{H}"] = shape_times(env, agent, dtype, src, H, reps)
    env.close()
    return res


def horizon_times(agent, reps):
    res = {"n_envs": 1024, "steps": 1000, "candidates": 64, "elites": 8, "iterations": 4, "dtype": "f32", "gamma": GAMMA, "bootstrap": BOOTSTRAP,
           "policy": "tests/golden/policy_trained.npz"}
    cases = (("H16_no_critic", 16, {}), ("H8_no_critic", 8, {}), ("H4_no_critic", 4, {}),
             ("H8_critic", 8, dict(agent=agent, gamma=GAMMA, bootstrap=BOOTSTRAP)), ("H4_critic", 4, dict(agent=agent, gamma=GAMMA, bootstrap=BOOTSTRAP)))
    for name, H, kw in cases:
        ev = pc.PlannerEvaluator(TRACK, n_envs=1024, num_rays=RAYS, reward_scaling=0.1, horizon=H, candidates=64, seed=0, kind="cem", elites=8,
                                 iterations=4, **kw)
        r = _times(ev.run, max(3, reps // 3), warmup=1)
        r["scalars"] = ev.evaluate()
        r["horizon"] = H
        res[name] = r
        ev.close()
        _say(name, f"{r['median_s'] * 1e3:.1f} ms", r["scalars"])
    return res


def main(out_path=os.path.join(ROOT, "profiles", "sequences_value_timing.json"), reps=10):
    if not torch.cuda.is_available():
        raise SystemExit("sequences_value_timing.py measures on the GPU: there is none")
    reps = int(reps)
    agent = trained_agent()
    res = {"track": "big_track", "num_rays": RAYS, "reps": reps, "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around calls_per_window enqueues and a device synchronise, per call; 2 warm-up windows",
           "f32": handle_times("f32", agent, reps), "f64": handle_times("f64", agent, reps), "cem_evaluation_f32": horizon_times(agent, reps)}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(*sys.argv[1:3])
