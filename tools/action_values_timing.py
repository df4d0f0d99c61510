"""Time of pc_sequences_action_values (K28) beside the pc_env_rollout_sequences_state (K22) launch that produced its input, and of one
soft-target minibatch step, pc_bc_minibatch_soft, beside pc_bc_minibatch on the same rows, parameters and workspace in the same
session.  The methods are tools/cem_timing.py's and tools/bc_timing.py's.

  python tools/action_values_timing.py [out.json] [reps]

  (a) 16384 freshly reset envs x 64 sequences and 1024 x 256, H = 16, big_track, 16 rays, F32 handles, the planner's shared table: K22
      (the best_* arrays in), then K28 on its ret / steps / status at temperature 0 and at 0.02 (the exponentials), each timed alone;
  (b) D = 23, A = 9, B = 64 / 512 / 1024, apply = 1: pc_bc_minibatch on labels, pc_bc_minibatch_soft on their one-hot rows and on
      softmax rows, and the ratio soft / hard.  The hard-label step of the same session is the yardstick.
Per item: the host clock around the enqueue of `calls_per_window` calls and a device synchronise, two warm-up windows and `reps` timed
ones (default ten), the median per call.  Writes profiles/action_values_timing.json by default; progress on stderr, one JSON line on
stdout.  No pass / fail gate."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ppo_car_amd as pc  # noqa: E402
from ppo_car_amd._capi import check, lib  # noqa: E402

TRACK = os.path.join(ROOT, "tracks", "big_track.json")
RAYS, HORIZON = 16, 16
D, H, A, ROWS = 23, 256, 9, 65536


def _wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _times(f, reps, inner, warmup=2):
    def g():
        for _ in range(inner):
            f()
    for _ in range(warmup):
        _wall(g)
    ts = [_wall(g) / inner for _ in range(reps)]
    return {"median_s": statistics.median(ts), "min_s": min(ts), "all_s": ts, "calls_per_window": inner}


def _say(*a):
    print(*a, file=sys.stderr, flush=True)


def kernel_times(M, K, reps):
    env = pc.VecCarEnv(M, TRACK, num_rays=RAYS, reward_scaling=0.1, dtype="f32")
    env.reset()
    p = pc.Planner(env, horizon=HORIZON, candidates=K, seed=0, action_values=True)
    table = p.candidate_table(0)
    stream = torch.cuda.current_stream().cuda_stream
    o = p.out
    score = lambda: env.score_sequences(table, out=o)

    def values(T):
        return lambda: check(lib.pc_sequences_action_values(0, o["ret"].data_ptr(), table.data_ptr(), 0, o["steps"].data_ptr(), o["status"].data_ptr(),
                                                            None, M, K, 0, T, o["q"].data_ptr(), o["q_count"].data_ptr(), o["q_alive"].data_ptr(),
                                                            o["soft"].data_ptr(), stream), "pc_sequences_action_values")

    score()
    q, v0, v1 = _times(score, reps, 5), _times(values(0.0), reps, 20), _times(values(0.02), reps, 20)
    soft = o["soft"]
    top = soft.max(-1).values
    res = {"states": M, "candidates": K, "horizon": HORIZON, "pc_env_rollout_sequences_state": q, "pc_sequences_action_values": v0,
           "pc_sequences_action_values_T_0.02": v1, "action_values_over_rollout_sequences": v0["median_s"] / q["median_s"],
           "bytes_read": M * K * 13 + K, "tied_rows_share": float(((soft == top.view(-1, 1)).sum(-1) >= 2).float().mean())}
    _say(f"M {M} K {K}: K22 {q['median_s'] * 1e6:.1f} us, K28 {v0['median_s'] * 1e6:.1f} us (T = 0.02: {v1['median_s'] * 1e6:.1f} us)")
    env.close()
    return res


def step_times(B, reps):
    g = torch.Generator().manual_seed(B)
    torch.manual_seed(0)
    param = torch.cat([p.detach().reshape(-1) for p in pc.Agent(D, A).parameters()]).cuda()
    n = param.numel()
    z = lambda k=n: torch.zeros(k, device="cuda")
    obs = (torch.rand(ROWS, D, generator=g) * 2.6 - 1.0).cuda()
    label = torch.randint(0, A, (ROWS,), generator=g)
    one_hot = torch.nn.functional.one_hot(label, A).float().cuda().contiguous()
    soft = torch.softmax(0.3 * torch.randn(ROWS, A, generator=g) / 0.1, -1).cuda().contiguous()
    label, target = label.float().cuda(), torch.randn(ROWS, generator=g).cuda()
    idx = torch.randint(0, ROWS, (B,), generator=g).cuda()
    grad, m, v, step, lr, metrics = z(), z(), z(), z(1), torch.full((1,), 3e-4, device="cuda"), z(4)
    ws = z(lib.pc_ppo_workspace_floats(B, D, H, A))
    st = torch.cuda.current_stream().cuda_stream
    state = (param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), lr.data_ptr())
    tail = (0.5, 0.01, 0.5, 0.9, 0.999, 1e-5, metrics.data_ptr(), ws.data_ptr(), 1, st)
    hard = lambda: check(lib.pc_bc_minibatch(0, idx.data_ptr(), B, D, H, A, obs.data_ptr(), label.data_ptr(), target.data_ptr(), *state, *tail),
                         "pc_bc_minibatch")
    soft_step = lambda rows: lambda: check(lib.pc_bc_minibatch_soft(0, idx.data_ptr(), B, D, H, A, obs.data_ptr(), rows.data_ptr(), target.data_ptr(),
                                                                    *state, *tail), "pc_bc_minibatch_soft")
    res = {"B": B, "pc_bc_minibatch": _times(hard, reps, 20), "pc_bc_minibatch_soft_one_hot": _times(soft_step(one_hot), reps, 20),
           "pc_bc_minibatch_soft": _times(soft_step(soft), reps, 20), "pc_bc_minibatch_again": _times(hard, reps, 20)}
    res["soft_over_hard"] = res["pc_bc_minibatch_soft"]["median_s"] / res["pc_bc_minibatch"]["median_s"]
    res["hard_again_over_hard"] = res["pc_bc_minibatch_again"]["median_s"] / res["pc_bc_minibatch"]["median_s"]
    _say(f"B {B}: hard {res['pc_bc_minibatch']['median_s'] * 1e6:.1f} us, soft {res['pc_bc_minibatch_soft']['median_s'] * 1e6:.1f} us "
         f"(one-hot rows {res['pc_bc_minibatch_soft_one_hot']['median_s'] * 1e6:.1f} us), ratio {res['soft_over_hard']:.3f}; the hard step again "
         f"{res['hard_again_over_hard']:.3f}")
    return res


def main(out_path=os.path.join(ROOT, "profiles", "action_values_timing.json"), reps=10):
    if not torch.cuda.is_available():
        raise SystemExit("action_values_timing.py measures on the GPU: there is none")
    reps = int(reps)
    res = {"track": "big_track", "num_rays": RAYS, "reps": reps, "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around calls_per_window enqueues and a device synchronise, per call; 2 warm-up windows; medians",
           "kernels": {f"envs_{M}_K_{K}": kernel_times(M, K, reps) for M, K in ((16384, 64), (1024, 256))},
           "step": {"D": D, "A": A, "rows": ROWS, "apply": 1, "shapes": [step_times(B, reps) for B in (64, 512, 1024)]}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(*sys.argv[1:3])
