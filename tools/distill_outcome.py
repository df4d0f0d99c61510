"""What distilling the planner does to the trained policy fixture (tests/golden/policy_trained.npz): its eval/* scalars on big_track,
1024 envs, 16 rays, sampled and greedy, before and after `rounds` DAgger rounds (ppo_car_amd.PlannerDistiller: 250 steps per round,
4 epochs per round on all rounds so far, batch 512, the teacher's share halving every round) against the CEM teacher with H = 8,
64 sequences x 4 rounds, 8 elites, gamma 0.99, bootstrapped from the FIXTURE's critic (a frozen copy); the teacher's own evaluation
and the wall time of the distillation.

  python tools/distill_outcome.py [out.json] [rounds] [--labels soft --label-temperature T [T ...]]

Writes profiles/distill_outcome.json by default; progress on stderr, one JSON line on stdout.  No pass / fail gate: the file says
what came out.  With --labels soft the same distillation runs on the teacher's soft rows (PlannerDistiller(labels="soft")), once per
temperature from the same start, and the file is profiles/distill_soft_outcome.json: {"runs": [one such result per temperature]}, the
rounds' scalars with bc/ties and bc/label_entropy among them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import ppo_car_amd as pc  # noqa: E402
from sequences_timing import RAYS, TRACK, trained_agent  # noqa: E402

N, SCALE = 1024, 0.1
TEACHER = dict(horizon=8, candidates=64, elites=8, iterations=4, gamma=0.99, bootstrap="running")


def _say(*a):
    print(*a, file=sys.stderr, flush=True)


def evaluate(agent):
    out = {}
    for name, greedy in (("sampled", False), ("greedy", True)):
        ev = pc.Evaluator(agent, TRACK, n_envs=N, num_rays=RAYS, reward_scaling=SCALE, greedy=greedy, seed=0)
        try:
            out[name] = ev.evaluate()
        finally:
            ev.close()
    return out


def run(rounds, labels="best", label_temperature=0.0, teacher_eval=True):
    student, teacher = trained_agent(), trained_agent().requires_grad_(False)
    res = {"track": "big_track", "num_rays": RAYS, "n_envs": N, "reward_scaling": SCALE, "device": torch.cuda.get_device_name(0),
           "policy": "tests/golden/policy_trained.npz", "teacher": dict(TEACHER, kind="cem"), "rounds": rounds, "steps_per_round": 250,
           "epochs_per_round": 4, "batch_size": 512, "beta0": 1.0, "beta_decay": 0.5}
    soft = {} if labels == "best" else dict(labels=labels, label_temperature=label_temperature)      # (the default run's file keeps its keys)
    res.update(soft)
    if teacher_eval:
        tv = pc.PlannerEvaluator(TRACK, n_envs=N, num_rays=RAYS, reward_scaling=SCALE, kind="cem", seed=0, agent=teacher, **TEACHER)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res["teacher_eval"] = tv.evaluate()
            res["teacher_eval_s"] = time.perf_counter() - t0
        finally:
            tv.close()
        _say("teacher", res["teacher_eval"])
    res["before"] = evaluate(student)
    _say("before", res["before"])
    ds = pc.PlannerDistiller(student, TRACK, n_envs=N, num_rays=RAYS, planner=dict(TEACHER, kind="cem", agent=teacher), steps_per_round=250,
                             beta0=1.0, beta_decay=0.5, epochs_per_round=4, learner=dict(batch_size=512), seed=0, rounds=rounds,
                             reward_scaling=SCALE, **soft)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res["rounds_out"] = []
        for r in range(rounds):
            res["rounds_out"].append(ds.round(r))
            _say("round", r, res["rounds_out"][-1])
        torch.cuda.synchronize()
        res["distill_s"] = time.perf_counter() - t0
    finally:
        ds.close()
    res["after"] = evaluate(student)
    _say("after", res["after"], f"{res['distill_s']:.1f} s")
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("rounds", nargs="?", type=int, default=8)
    ap.add_argument("--labels", choices=("best", "soft"), default="best")
    ap.add_argument("--label-temperature", type=float, nargs="+", default=[0.0], metavar="T")
    args = ap.parse_args(argv)
    if args.labels == "best" and args.label_temperature != [0.0]:
        ap.error("--label-temperature needs --labels soft")
    if not torch.cuda.is_available():
        raise SystemExit("distill_outcome.py measures on the GPU: there is none")
    soft = args.labels == "soft"
    out_path = args.out or os.path.join(ROOT, "profiles", "distill_soft_outcome.json" if soft else "distill_outcome.json")
    if soft:
        res = {"runs": [run(args.rounds, "soft", T, teacher_eval=i == 0) for i, T in enumerate(args.label_temperature)]}
    else:
        res = run(args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
