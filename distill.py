#!/usr/bin/env python3
"""distill.py -- distil a planner into the policy: DAgger with behaviour cloning (ppo_car_amd.PlannerDistiller).

    python distill.py --track tracks/big_track.json --num-rays 16 --envs 1024 [--checkpoint in.dat] --out out.dat
                      --rounds 8 --steps-per-round 250 --planner cem --plan-horizon 8 --plan-candidates 64 --plan-iterations 4 --plan-elites 8
                      [--plan-gamma 0.99 --plan-bootstrap running --teacher-checkpoint model.dat] [--eval-every 2 --eval-envs 1024]

Per round: --steps-per-round steps from a reset in which the planner labels every env's state and a share beta_r = beta0 * decay^r of
the envs executes its action (the rest the student's), then --epochs cross-entropy epochs on all labelled states so far.  One JSON
line per round: the bc/* scalars, plus the eval/* scalars of ppo_car_amd.Evaluator (sampled) every --eval-every rounds.  --out is an
agent state_dict as train.py saves it: evaluate.py --checkpoint reads it.  Without --checkpoint the student is a fresh agent.
The --plan-* options are evaluate.py's, with its rules; the critic a bootstrapped teacher consults is --teacher-checkpoint's, a frozen
copy of its own: the teacher does not move while the student learns."""
import argparse
import json

import torch


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--track", default="tracks/big_track.json")
    ap.add_argument("--num-rays", type=int, default=16)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--checkpoint", default=None, help="the student's start: an agent state_dict as train.py saves it (default: a fresh agent)")
    ap.add_argument("--out", required=True, help="where the distilled agent's state_dict is written")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps-per-round", type=int, default=250)
    ap.add_argument("--epochs", type=int, default=4, help="cross-entropy epochs per round")
    ap.add_argument("--beta0", type=float, default=1.0, help="the teacher's share of the envs in round 0")
    ap.add_argument("--beta-decay", type=float, default=0.5, help="... multiplied by this every round")
    ap.add_argument("--no-aggregate", action="store_true", help="train on the round's own states only, not on all rounds so far")
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--learning-rate", type=float, default=3e-4)
    ap.add_argument("--ent-coef", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reward-scaling", type=float, default=0.1, help="the scale of the returns the teacher compares: with --plan-bootstrap the "
                    "one --teacher-checkpoint's critic was trained at (train.py's default)")
    ap.add_argument("--planner", choices=("shooting", "cem"), default="cem")
    ap.add_argument("--plan-horizon", type=int, default=argparse.SUPPRESS, metavar="H", help="steps per candidate sequence (default 16)")
    ap.add_argument("--plan-candidates", type=int, default=argparse.SUPPRESS, metavar="K", help="sequences scored per env and step (default 256; "
                    "--planner cem: per iteration, default 64)")
    ap.add_argument("--plan-iterations", type=int, default=argparse.SUPPRESS, metavar="I", help="--planner cem: sample / score / refit rounds per step")
    ap.add_argument("--plan-elites", type=int, default=argparse.SUPPRESS, metavar="E", help="--planner cem: the best sequences the weights are refitted to")
    ap.add_argument("--plan-gamma", type=float, default=argparse.SUPPRESS, metavar="G", help="discount of a sequence's rewards, 0 .. 1 (default 1)")
    ap.add_argument("--plan-bootstrap", choices=("none", "running", "running_truncated"), default=argparse.SUPPRESS, help="add gamma^n * the critic's "
                    "value of the state a sequence ends in; needs --teacher-checkpoint (default none)")
    ap.add_argument("--labels", choices=("best", "soft"), default="best", help="best: the first action of the teacher's best sequence; soft: a "
                    "target over the actions from what the best sequence beginning with each one earned (exact ties share the mass)")
    ap.add_argument("--label-temperature", type=float, default=0.0, metavar="T", help="--labels soft: softmax of the per-action returns / T, in "
                    "units of the scaled return (0: all mass on the maximal actions)")
    ap.add_argument("--teacher-checkpoint", default=None, help="the agent whose critic the teacher bootstraps from (kept frozen)")
    ap.add_argument("--eval-every", type=int, default=0, metavar="R", help="evaluate the student after every R-th round (0 = never)")
    ap.add_argument("--eval-envs", type=int, default=1024)
    args = ap.parse_args(argv)
    cem = args.planner == "cem"
    if cem != hasattr(args, "plan_iterations") or cem != hasattr(args, "plan_elites"):
        ap.error("--planner cem takes --plan-iterations and --plan-elites, both of them, and --planner shooting neither")
    if getattr(args, "plan_bootstrap", "none") != "none" and args.teacher_checkpoint is None:
        ap.error("--plan-bootstrap other than none needs --teacher-checkpoint: the critic that values the end states")
    if args.rounds < 1 or args.steps_per_round < 1 or args.epochs < 1:
        ap.error("--rounds, --steps-per-round and --epochs must be >= 1")
    if not 0.0 <= args.label_temperature < float("inf") or (args.labels == "best" and args.label_temperature != 0.0):
        ap.error("--label-temperature must be finite and >= 0, and needs --labels soft")
    if args.eval_every < 0 or args.eval_envs < 1:
        ap.error("--eval-every must be >= 0 and --eval-envs >= 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("distill.py needs the GPU: the env has no CPU path")
    import ppo_car_amd as pc
    from ppo_car_amd.env import ray_count
    D = 6 + ray_count(args.num_rays)
    agent = pc.Agent(D, 9).cuda()
    if args.checkpoint is not None:
        agent.load_state_dict(torch.load(args.checkpoint, map_location="cuda"))
    cem = args.planner == "cem"
    planner = dict(kind=args.planner, horizon=getattr(args, "plan_horizon", 16), candidates=getattr(args, "plan_candidates", 64 if cem else 256))
    if cem:
        planner.update(iterations=args.plan_iterations, elites=args.plan_elites)
    if hasattr(args, "plan_gamma") or hasattr(args, "plan_bootstrap"):
        planner.update(gamma=getattr(args, "plan_gamma", 1.0), bootstrap=getattr(args, "plan_bootstrap", "none"))
        if planner["bootstrap"] != "none":
            teacher = pc.Agent(D, 9).cuda()
            teacher.load_state_dict(torch.load(args.teacher_checkpoint, map_location="cuda"))
            planner["agent"] = teacher.requires_grad_(False)
    ds = pc.PlannerDistiller(agent, args.track, n_envs=args.envs, num_rays=args.num_rays, planner=planner, steps_per_round=args.steps_per_round,
                             beta0=args.beta0, beta_decay=args.beta_decay, epochs_per_round=args.epochs, aggregate=not args.no_aggregate,
                             learner=dict(learning_rate=args.learning_rate, batch_size=args.batch_size, ent_coef=args.ent_coef), seed=args.seed,
                             rounds=args.rounds, reward_scaling=args.reward_scaling, labels=args.labels, label_temperature=args.label_temperature)
    ev = None
    lines = []
    try:
        if args.eval_every:
            ev = pc.Evaluator(agent, args.track, n_envs=args.eval_envs, num_rays=args.num_rays, reward_scaling=1.0, device="cuda", seed=args.seed)
        for r in range(args.rounds):
            out = {"round": r, **ds.round(r)}
            if ev is not None and (r + 1) % args.eval_every == 0:
                out.update(ev.evaluate())
            print(json.dumps(out), flush=True)
            lines.append(out)
    finally:
        ds.close()
        if ev is not None:
            ev.close()
    torch.save({k: v.detach().clone() for k, v in agent.state_dict().items()}, args.out)
    return lines


if __name__ == "__main__":
    main()
