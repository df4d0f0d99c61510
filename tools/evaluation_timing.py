"""Wall time of one batched evaluation (ppo_car_amd.Evaluator: 1000 steps from reset, the first episode of every env) on big_track at
16 rays with the trained policy fixture, next to evaluate.py's per-step Python loop.

  python tools/evaluation_timing.py [out.json] [reps]

Per batch size (1024 and 16384 envs) and path -- "mega" (one pc_rollout per window of 250 steps), "steps" (sampled: pc_policy_act +
pc_env_step per step) and "greedy" (pc_policy_act + pc_greedy + pc_env_step per step) --: the host clock around Evaluator.run() and
the fetch of its totals (the fetch synchronises), one warm-up run and `reps` timed ones (median and all), and the construction time
of the Evaluator beside it.  `evaluate_py`: the whole of evaluate.main with --episodes 1024 (env and agent construction, the 1000-step
loop of torch MLP + VecCarEnv.step + five torch ops with its per-step host read, the fetch), which this change leaves as it was.
Writes profiles/evaluation_timing.json by default; one JSON line on stdout."""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ppo_car_amd as pc  # noqa: E402

TRACK = os.path.join(ROOT, "tracks", "big_track.json")
PATHS = {"mega": dict(), "steps": dict(rollout_kernel="steps"), "greedy": dict(greedy=True)}


def _wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def evaluator_times(agent, N, reps):
    res = {}
    for name, kw in PATHS.items():
        build_s, ev = _wall(lambda: pc.Evaluator(agent, TRACK, n_envs=N, num_rays=16, reward_scaling=0.1, device="cuda", seed=1, **kw))
        ev.evaluate(index=0)          # warm-up: code objects, allocator
        times, scalars = [], None
        for i in range(reps):
            dt, scalars = _wall(lambda: ev.evaluate(index=1 + i))
            times.append(dt)
        res[name] = {"path": ev.last_path, "rollout_kernel": ev.envs.last_rollout_kernel(), "step_kernel": ev.envs.last_step_kernel(),
                     "construct_s": build_s, "run_and_fetch_s": statistics.median(times), "run_and_fetch_all_s": times,
                     "last_scalars": scalars}
        ev.close()
    return res


def evaluate_py_time(agent, N, reps):
    import evaluate
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "model.dat")
        torch.save(agent.state_dict(), path)
        argv = ["--checkpoint", path, "--track", TRACK, "--num-rays", "16", "--episodes", str(N)]
        evaluate.main(argv)           # warm-up
        times = [_wall(lambda: evaluate.main(argv))[0] for _ in range(reps)]
    return {"episodes": N, "main_s": statistics.median(times), "main_all_s": times}


def main(out_path=os.path.join(ROOT, "profiles", "evaluation_timing.json"), reps=3):
    from oracle.scenarios import load_trained_policy
    if not torch.cuda.is_available():
        raise SystemExit("evaluation_timing.py measures on the GPU: there is none")
    agent = pc.Agent(23, 9).cuda()
    load_trained_policy(agent)
    res = {"track": "big_track", "num_rays": 16, "policy": "tests/golden/policy_trained.npz", "steps_per_evaluation": 1000, "chunk": 250,
           "reps": int(reps), "device": torch.cuda.get_device_name(0), "clock": "host perf_counter around run + fetch, synchronised",
           "evaluator": {str(N): evaluator_times(agent, N, int(reps)) for N in (1024, 16384)},
           "evaluate_py": evaluate_py_time(agent, 1024, int(reps))}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(*sys.argv[1:3])
