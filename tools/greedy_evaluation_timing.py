"""Wall time of one GREEDY batched evaluation (ppo_car_amd.Evaluator(greedy=True): 1000 steps from reset, the first episode of every env) on
big_track at 16 rays with the trained policy fixture -- tools/evaluation_timing.py's fixture, track, ray count and method.

  python tools/greedy_evaluation_timing.py [out.json] [reps] [parent_tree]

Per batch size (1024 and 16384 envs): greedy on "steps" (pc_policy_act_greedy + pc_env_step per step) and on "mega" (one pc_rollout_greedy
per window of 250 steps), with the sampled "mega" evaluation (one pc_rollout per window) beside them: the host clock around Evaluator.run()
and the fetch of its totals (the fetch synchronises), one warm-up run and `reps` timed ones (median and all).
`parent_tree`: a checkout of the PARENT commit with its library built.  Its greedy evaluation -- pc_policy_act + pc_greedy + pc_env_step per
step, what Evaluator(greedy=True) was before the policy kernels had a greedy form -- is timed first, in a fresh child process that imports
the package from that tree, on the same device in the same session: the "before" of this change (this tree's own "steps" path is not: it has
lost a launch per step).  Writes profiles/greedy_evaluation_timing.json by default; one JSON line on stdout."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1024, 16384)


def _wall(torch, f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def evaluator_times(tree, paths, reps):
    """{N: {name: figures}} for the Evaluator of the package under `tree`"""
    sys.path.insert(0, tree)
    import torch

    import ppo_car_amd as pc
    from oracle.scenarios import load_trained_policy
    if not torch.cuda.is_available():
        raise SystemExit("greedy_evaluation_timing.py measures on the GPU: there is none")
    agent = pc.Agent(23, 9).cuda()
    load_trained_policy(agent)
    track = os.path.join(tree, "tracks", "big_track.json")
    res = {"device": torch.cuda.get_device_name(0)}
    for N in SIZES:
        res[str(N)] = {}
        for name, kw in paths.items():
            ev = pc.Evaluator(agent, track, n_envs=N, num_rays=16, reward_scaling=0.1, device="cuda", seed=1, **kw)
            ev.evaluate(index=0)          # warm-up: code objects, allocator
            times, scalars = [], None
            for i in range(reps):
                dt, scalars = _wall(torch, lambda: ev.evaluate(index=1 + i))
                times.append(dt)
            res[str(N)][name] = {"path": ev.last_path, "rollout_kernel": ev.envs.last_rollout_kernel(), "step_kernel": ev.envs.last_step_kernel(),
                                 "run_and_fetch_s": statistics.median(times), "run_and_fetch_all_s": times, "last_scalars": scalars}
            ev.close()
    return res


PARENT_PATHS = {"greedy": dict(greedy=True)}
PATHS = {"greedy_steps": dict(greedy=True, rollout_kernel="steps"), "greedy_mega": dict(greedy=True, rollout_kernel="mega"), "sampled_mega": dict()}


def main(out_path=os.path.join(ROOT, "profiles", "greedy_evaluation_timing.json"), reps=3, parent_tree=None):
    reps = int(reps)
    parent = None
    if parent_tree:        # first, and in a process of its own: one package per process, one process on the device at a time
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", os.path.abspath(parent_tree), str(reps)], check=True,
                             capture_output=True, text=True).stdout
        parent = json.loads(out.strip().splitlines()[-1])
    cur = evaluator_times(ROOT, PATHS, reps)
    res = {"track": "big_track", "num_rays": 16, "policy": "tests/golden/policy_trained.npz", "steps_per_evaluation": 1000, "chunk": 250,
           "reps": reps, "device": cur.pop("device"), "clock": "host perf_counter around run + fetch, synchronised",
           "evaluator": {str(N): cur[str(N)] for N in SIZES},
           "parent_commit_greedy": None if parent is None else {str(N): parent[str(N)]["greedy"] for N in SIZES}}
    if parent is not None:
        res["summary_ms"] = {str(N): {"parent_greedy": 1e3 * parent[str(N)]["greedy"]["run_and_fetch_s"],
                                      **{k: 1e3 * v["run_and_fetch_s"] for k, v in cur[str(N)].items()}} for N in SIZES}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--tree":
        print(json.dumps(evaluator_times(sys.argv[2], PARENT_PATHS, int(sys.argv[3]))), flush=True)
    else:
        main(*sys.argv[1:4])
