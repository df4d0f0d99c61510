#!/usr/bin/env python3
"""evaluate.py -- headless evaluation of a trained policy: the episode loop of the reference's
log_video (train.py:23-50) without the renderer: one env, actions from the agent, until the car is destroyed
(`done = terminated`, train.py:45 -- a truncation does not end the loop there; here the episode limit does).

    python evaluate.py --checkpoint checkpoints/<run>/model.dat --track tracks/big_track.json [--num-rays 12] [--episodes 5]
                       [--frames DIR [--frame-every 5]]      # PNG frames of episode 0 (software rasteriser, no pygame)
    python evaluate.py --checkpoint ... --envs 4096 [--greedy]       # batched: the first episodes of 4096 envs (ppo_car_amd.Evaluator),
                                                                     # JSON with the eval/* scalars (lap times in steps) and the path taken
    python evaluate.py --checkpoint ... --envs 4096 --greedy --rollout-kernel mega     # ... the greedy windows as persistent launches
    python evaluate.py --checkpoint ... --envs 4096 --maps out/eval                    # ... plus telemetry maps of those first episodes:
                                                                     # out/eval.npz and a PNG per plane (visits, mean speed, crashes)
    python evaluate.py --checkpoint ... --envs 4096 --greedy --shield 2                # ... shielded: an action that cannot avoid a crash within
                                                                     # 2 steps is replaced by the best one that can (per-step path);
                                                                     # adds eval/shield_interventions and eval/shield_doomed
    python evaluate.py --checkpoint ... --envs 64 --video out.png [--video-envs 4] [--video-scale 4] [--video-fps 30]
                                                                     # ... plus an animated PNG of envs 0 .. 3 driving their first episodes,
                                                                     # rendered on the device (ppo_car_amd.Renderer), side by side
    python evaluate.py --checkpoint ... --landscape out/eval [--landscape-cell 8] [--landscape-speed 0.5]
                                                                     # the policy landscape (ppo_car_amd.PolicyLandscape): value and greedy action
                                                                     # at every cell x 72 headings -> out/eval_landscape.npz and a PNG per track
                      [--landscape-horizon 64] [--landscape-lookahead]
                                                                     # ... plus how many steps the greedy policy survives from every pose
                                                                     # (out/eval_survival_<track>.png) and the one-step look-ahead of all 9 actions
    python evaluate.py --planner shooting --plan-horizon 16 --plan-candidates 256 --envs 1024 [--track ...]
                                                                     # no checkpoint: the first episodes of 1024 envs under a random-shooting
                                                                     # planner on the env's own model (ppo_car_amd.PlannerEvaluator), the same
                                                                     # eval/* scalars: the model-based baseline a policy's figures stand beside
    python evaluate.py --planner cem --plan-iterations 4 --plan-elites 8 [--plan-horizon 16] [--plan-candidates 64] --envs 1024
                                                                     # ... under the cross-entropy planner (ppo_car_amd.CEMPlanner): 4 rounds
                                                                     # of 64 sequences per step, each env's action weights refitted to its 8
                                                                     # best; both options must be given: they are the split of the budget
    python evaluate.py --planner cem ... --plan-horizon 4 --checkpoint model.dat --plan-gamma 0.99 --plan-bootstrap running
                                                                     # ... scoring each sequence by its discounted return plus gamma^n * the
                                                                     # checkpoint's critic at the state it ends in (running_truncated: also
                                                                     # where it ends at the time limit); a bootstrap needs --checkpoint
"""
import argparse
import json

import torch


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None, help="agent state_dict as train.py saves it (checkpoint_<n>.dat / model.dat); required "
                    "unless --planner is given")
    ap.add_argument("--track", default="tracks/big_track.json")
    ap.add_argument("--num-rays", type=int, default=12)
    ap.add_argument("--episodes", type=int, default=5)
    ap.add_argument("--greedy", action="store_true", help="argmax instead of sampling (the reference samples)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", default=None, help="directory for PNG frames of episode 0 (the role of log_video's frames)")
    ap.add_argument("--frame-every", type=int, default=5)
    ap.add_argument("--envs", type=int, default=None, help="batched evaluation: the first episodes of this many envs on the device "
                    "(ppo_car_amd.Evaluator) instead of the --episodes loop; prints the eval/* scalars")
    ap.add_argument("--rollout-kernel", choices=("auto", "mega", "steps"), default="auto",
                    help="--envs: how the Evaluator steps -- 'mega' = persistent launches (pc_rollout; with --greedy pc_rollout_greedy), 'steps' = "
                    "the per-step kernels, 'auto' = mega for sampled evaluations, steps for greedy ones")
    ap.add_argument("--shield", type=int, default=0, metavar="D", help="--envs: shielded evaluation (Evaluator(shield_depth=D), D = 1 .. 4): an action "
                    "that cannot avoid a crash within D steps is replaced by the safe action with the highest logit; per-step path only; 0 = off")
    ap.add_argument("--maps", default=None, metavar="PREFIX", help="--envs: write telemetry maps of the first episodes (ppo_car_amd.TrackMaps: "
                    "visits, mean speed and crashes per cell) to PREFIX.npz and PREFIX_<track>_<plane>.png")
    ap.add_argument("--landscape", default=None, metavar="PREFIX", help="write the policy landscape (ppo_car_amd.PolicyLandscape: the critic's value, "
                    "the greedy action and whether the pose is drivable, per cell and heading) to PREFIX_landscape.npz and "
                    "PREFIX_landscape_<track>.png, instead of running episodes")
    ap.add_argument("--landscape-cell", type=int, default=8, choices=(4, 5, 8, 10, 16, 20, 40, 80), help="cell size of the landscape in pixels")
    ap.add_argument("--landscape-speed", type=float, default=0.5, help="speed of the observed car as a fraction of max_speed, along its heading")
    ap.add_argument("--landscape-horizon", type=int, default=0, metavar="H", help="--landscape: also drive the greedy policy H steps (1 .. 999) from every "
                    "pose (PolicyLandscape.survival): `survived` in the .npz and PREFIX_survival_<track>.png; 0 = off")
    ap.add_argument("--landscape-lookahead", action="store_true", help="--landscape: also step every pose once under each of the 9 actions "
                    "(PolicyLandscape.lookahead): safe_actions, greedy_crashes and avoidable in the .npz")
    ap.add_argument("--video", default=None, metavar="FILE.png", help="--envs: write an animated PNG of the first episodes of envs 0 .. --video-envs - 1 "
                    "(every second step, rendered on the device from the evaluation's own observation rows)")
    ap.add_argument("--video-envs", type=int, default=4, help="envs shown side by side in the video")
    ap.add_argument("--video-scale", type=int, default=4, help="a video frame is 1280 / scale x 720 / scale per env: 1, 2, 4, 5, 8 or 10")
    ap.add_argument("--video-fps", type=int, default=30)
    # the planner's options appear in the namespace only when given: without --planner it is the namespace it always was
    ap.add_argument("--planner", choices=("shooting", "cem"), default=argparse.SUPPRESS, help="--envs: evaluate a planner on the env's own model "
                    "(ppo_car_amd.PlannerEvaluator) instead of a checkpoint's policy: uniform random shooting, or the cross-entropy method "
                    "(which takes --plan-iterations and --plan-elites)")
    ap.add_argument("--plan-horizon", type=int, default=argparse.SUPPRESS, metavar="H", help="--planner: steps per candidate sequence (default 16)")
    ap.add_argument("--plan-candidates", type=int, default=argparse.SUPPRESS, metavar="K", help="--planner: sequences scored per env and step, "
                    "the first 9 hold one action each (default 256; --planner cem: per iteration, default 64)")
    ap.add_argument("--plan-iterations", type=int, default=argparse.SUPPRESS, metavar="I", help="--planner cem: sample / score / refit rounds per step")
    ap.add_argument("--plan-elites", type=int, default=argparse.SUPPRESS, metavar="E", help="--planner cem: the best sequences the weights are refitted to")
    ap.add_argument("--plan-gamma", type=float, default=argparse.SUPPRESS, metavar="G", help="--planner: discount of a sequence's rewards, 0 .. 1 (default 1)")
    ap.add_argument("--plan-bootstrap", choices=("none", "running", "running_truncated"), default=argparse.SUPPRESS, help="--planner: add "
                    "gamma^n * the critic's value of the state a sequence ends in, where it still runs (running) or also where it ended at the "
                    "time limit (running_truncated); needs --checkpoint (default none)")
    args = ap.parse_args(argv)
    if not hasattr(args, "planner"):
        if args.checkpoint is None:
            ap.error("the following arguments are required: --checkpoint")
        if any(hasattr(args, k) for k in ("plan_horizon", "plan_candidates", "plan_iterations", "plan_elites")):
            ap.error("--plan-horizon / --plan-candidates / --plan-iterations / --plan-elites belong to --planner")
        if hasattr(args, "plan_gamma") or hasattr(args, "plan_bootstrap"):
            ap.error("--plan-gamma / --plan-bootstrap belong to --planner")
    elif (args.planner == "cem") != hasattr(args, "plan_iterations") or (args.planner == "cem") != hasattr(args, "plan_elites"):
        # the split of a step's budget into rounds and elites has no default on the command line: cem names both, shooting neither
        ap.error("--planner cem takes --plan-iterations and --plan-elites, both of them, and --planner shooting neither")
    elif args.envs is None:
        raise ValueError("--planner evaluates the batched first episodes: pass --envs N")
    elif getattr(args, "plan_bootstrap", "none") != "none" and args.checkpoint is None:
        ap.error("--plan-bootstrap other than none needs --checkpoint: the critic that values the end states")
    check_video_args(args)
    if args.shield and args.rollout_kernel == "mega":
        raise ValueError("--shield masks the action between the policy step and the env step: --rollout-kernel must be 'auto' or 'steps', not 'mega'")
    return args


def check_video_args(args):
    """ValueError for a --video request that cannot be served (before anything touches the device)."""
    if args.video is None:
        return
    if args.envs is None:
        raise ValueError("--video renders envs of the batched evaluation: pass --envs N")
    if not 1 <= args.video_envs <= args.envs:
        raise ValueError(f"--video-envs must be 1 .. --envs = {args.envs}, not {args.video_envs}")
    if args.video_scale not in (1, 2, 4, 5, 8, 10):
        raise ValueError(f"--video-scale must be one of 1, 2, 4, 5, 8, 10, not {args.video_scale}")
    if not 1 <= args.video_fps <= 65535:
        raise ValueError(f"--video-fps must be 1 .. 65535, not {args.video_fps}")


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("evaluate.py needs the GPU: the env has no CPU path")
    import ppo_car_amd as pc
    if hasattr(args, "planner"):
        return planned(pc, args)
    if args.landscape is not None:
        return landscape(pc, args)
    if args.envs is not None:
        return batched(pc, args)
    torch.manual_seed(args.seed)
    env = pc.VecCarEnv(args.episodes, args.track, num_rays=args.num_rays, reward_scaling=1.0, device="cuda")
    agent = pc.Agent(env.obs_dim, env.act_dim).cuda()
    agent.load_state_dict(torch.load(args.checkpoint, map_location="cuda"))
    obs, _ = env.reset()
    N = args.episodes
    alive = torch.ones(N, dtype=torch.bool, device="cuda")
    ret = torch.zeros(N, device="cuda")
    steps = torch.zeros(N, dtype=torch.int64, device="cuda")
    gates = torch.zeros(N, dtype=torch.int32, device="cuda")
    gp = torch.empty(N, dtype=torch.int32, device="cuda")
    frames = 0
    if args.frames:
        import os
        from ppo_car_amd.env import Track
        from ppo_car_amd.render import rasterise, write_png
        os.makedirs(args.frames, exist_ok=True)
        walls, gate_segs = Track(args.track).geometry()
    with torch.no_grad():
        for t in range(1000):               # CarEnv's own time limit (car_env.py:491)
            if args.frames and bool(alive[0]) and t % args.frame_every == 0:
                st = env.get_state()        # (synchronous test hook: fine for a viewer)
                rot = float(st["rot"][0])
                img = rasterise(walls, gate_segs, float(st["px"][0]), float(st["py"][0]), rot, obs[0, 6:].cpu().numpy(),
                                next_gate=int(st["next_gate"][0]), num_rays_nominal=args.num_rays)
                write_png(os.path.join(args.frames, f"frame_{frames:05d}.png"), img)
                frames += 1
            if args.greedy:
                action = agent.actor(obs).argmax(-1)
            else:
                action, _, _, _ = agent.get_action_and_value(obs)
            obs, r, term, trunc, _ = env.step(action, gates_passed=gp)
            ret += torch.where(alive, r, torch.zeros_like(r))
            steps += alive.long()
            gates = torch.where(alive, gp, gates)
            alive &= ~((term + trunc) > 0)
            if not bool(alive.any()):
                break
    out = {"episodes": N, "mean_return": float(ret.mean()), "mean_steps": float(steps.float().mean()),
           "mean_gates_passed": float(gates.float().mean()), "returns": ret.tolist(), "gates_passed": gates.tolist()}
    if args.frames:
        out["frames"] = frames
    print(json.dumps(out))
    return out


def batched(pc, args):
    """--envs N: N first episodes in 1000 device steps, no host round trip per step."""
    from ppo_car_amd.env import ray_count
    agent = pc.Agent(6 + ray_count(args.num_rays), 9).cuda()
    agent.load_state_dict(torch.load(args.checkpoint, map_location="cuda"))
    ev = pc.Evaluator(agent, args.track, n_envs=args.envs, num_rays=args.num_rays, reward_scaling=1.0, device="cuda", greedy=args.greedy,
                      seed=args.seed, rollout_kernel=args.rollout_kernel, track_maps=args.maps is not None,
                      video_envs=args.video_envs if args.video is not None else 0, video_scale=args.video_scale, shield_depth=args.shield)
    try:
        out = ev.evaluate()
        out["path"] = ev.last_path
        if args.maps is not None:
            out["maps"] = ev.maps.save(args.maps, ev.envs._tracks)
        if args.video is not None:
            from ppo_car_amd.render import write_apng
            frames = ev.video_frames()
            write_apng(args.video, frames, fps=args.video_fps)
            out["video"] = {"file": args.video, "frames": int(frames.shape[0]), "height": int(frames.shape[1]), "width": int(frames.shape[2])}
    finally:
        ev.close()
    print(json.dumps(out))
    return out


def planned(pc, args):
    """--planner shooting | cem --envs N: N first episodes under the planner, the eval/* scalars of batched()."""
    cem = args.planner == "cem"
    more = dict(kind="cem", iterations=args.plan_iterations, elites=args.plan_elites) if cem else {}
    critic = hasattr(args, "plan_gamma") or hasattr(args, "plan_bootstrap")
    if critic:      # (without the two options: the call it always was)
        more.update(gamma=getattr(args, "plan_gamma", 1.0), bootstrap=getattr(args, "plan_bootstrap", "none"))
        if more["bootstrap"] != "none":
            from ppo_car_amd.env import ray_count
            agent = pc.Agent(6 + ray_count(args.num_rays), 9).cuda()
            agent.load_state_dict(torch.load(args.checkpoint, map_location="cuda"))
            more["agent"] = agent
    ev = pc.PlannerEvaluator(args.track, n_envs=args.envs, num_rays=args.num_rays, reward_scaling=1.0, device="cuda",
                             horizon=getattr(args, "plan_horizon", 16), candidates=getattr(args, "plan_candidates", 64 if cem else 256),
                             seed=args.seed, **more)
    try:
        out = ev.evaluate()
        out["path"] = ev.last_path
        out["planner"] = {"kind": args.planner, "horizon": ev.planner.horizon, "candidates": ev.planner.candidates}
        if cem:
            out["planner"].update(iterations=ev.planner.iterations, elites=ev.planner.elites)
        if critic:
            out["planner"].update(gamma=more["gamma"], bootstrap=more["bootstrap"])
    finally:
        ev.close()
    print(json.dumps(out))
    return out


def landscape(pc, args):
    """--landscape PREFIX: value / action / drivable maps of the checkpoint's policy over the whole track."""
    from ppo_car_amd.env import ray_count
    agent = pc.Agent(6 + ray_count(args.num_rays), 9).cuda()
    agent.load_state_dict(torch.load(args.checkpoint, map_location="cuda"))
    ls = pc.PolicyLandscape(agent, args.track, args.num_rays, cell_px=args.landscape_cell, speed=args.landscape_speed, device="cuda")
    try:
        ls.compute()
        if args.landscape_horizon > 0:
            ls.survival(args.landscape_horizon)
        if args.landscape_lookahead:
            ls.lookahead()
        files = ls.save(args.landscape)
        best = ls.best_value()
        out = {"landscape": files, "cells": int(best.numel()), "drivable_cells": int((~best.isnan()).sum()),
               "poses": ls.n_tracks * ls.poses_per_track, "drivable_poses": int(ls.drivable.sum())}
        if args.landscape_horizon > 0:      # cells with a heading from which the greedy policy drives the whole horizon
            out["survival_horizon"] = args.landscape_horizon
            out["cells_surviving"] = int((ls.survived.amax(1) >= args.landscape_horizon).sum())
        if args.landscape_lookahead:
            out["avoidable_poses"] = int(ls.avoidable.sum())
    finally:
        ls.close()
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
