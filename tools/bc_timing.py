"""Time of one supervised minibatch step, pc_bc_minibatch (K27 + K11 + K12), beside pc_ppo_minibatch (K10 + K11 + K12) on the same rows,
parameters and workspace in the same session.  D = 23 (16 rays), A = 9, B = 64 / 512 / 1024, apply = 1.

  python tools/bc_timing.py [out.json] [reps]

Per item: the host clock around synchronises, `calls_per_window` steps enqueued back to back inside one timed window (a step is three
launches of microseconds), two warm-up windows and `reps` timed ones (default ten); the median per call, both figures and their ratio.
The cross-entropy head does strictly less work after the forward pass (no advantage statistics, no ratio), so a ratio above 1 wants
an explanation.  Writes profiles/bc_timing.json by default; progress on stderr, one JSON line on stdout.  No pass / fail gate."""
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

D, H, A, M = 23, 256, 9, 65536
INNER = 20


def _wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _times(f, reps, warmup=2):
    def g():
        for _ in range(INNER):
            f()
    for _ in range(warmup):
        _wall(g)
    ts = [_wall(g) / INNER for _ in range(reps)]
    return {"median_s": statistics.median(ts), "min_s": min(ts), "all_s": ts, "calls_per_window": INNER}


def shape(B, reps):
    g = torch.Generator().manual_seed(B)
    torch.manual_seed(0)
    param = torch.cat([p.detach().reshape(-1) for p in pc.Agent(D, A).parameters()]).cuda()
    n = param.numel()
    z = lambda k=n: torch.zeros(k, device="cuda")
    obs = (torch.rand(M, D, generator=g) * 2.6 - 1.0).cuda()
    act = torch.randint(0, A, (M,), generator=g).float().cuda()
    old_lp, adv, ret = (-2.2 + 0.3 * torch.randn(M, generator=g)).cuda(), torch.randn(M, generator=g).cuda(), torch.randn(M, generator=g).cuda()
    idx = torch.randint(0, M, (B,), generator=g).cuda()
    grad, m, v, step, lr, metrics = z(), z(), z(), z(1), torch.full((1,), 3e-4, device="cuda"), z(4)
    ws = z(lib.pc_ppo_workspace_floats(B, D, H, A))
    st = torch.cuda.current_stream().cuda_stream
    state = (param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), lr.data_ptr())
    tail = (0.5, 0.01, 0.5, 0.9, 0.999, 1e-5, metrics.data_ptr(), ws.data_ptr(), 1, st)
    ppo = lambda: check(lib.pc_ppo_minibatch(0, idx.data_ptr(), B, D, H, A, obs.data_ptr(), act.data_ptr(), old_lp.data_ptr(), adv.data_ptr(),
                                             ret.data_ptr(), *state, 0.2, *tail), "pc_ppo_minibatch")
    bc = lambda: check(lib.pc_bc_minibatch(0, idx.data_ptr(), B, D, H, A, obs.data_ptr(), act.data_ptr(), ret.data_ptr(), *state, *tail),
                       "pc_bc_minibatch")
    bc0 = lambda: check(lib.pc_bc_minibatch(0, idx.data_ptr(), B, D, H, A, obs.data_ptr(), act.data_ptr(), None, *state, 0.0, *tail[1:]),
                        "pc_bc_minibatch")
    res = {"B": B, "pc_ppo_minibatch": _times(ppo, reps), "pc_bc_minibatch": _times(bc, reps), "pc_bc_minibatch_no_target": _times(bc0, reps)}
    res["bc_over_ppo"] = res["pc_bc_minibatch"]["median_s"] / res["pc_ppo_minibatch"]["median_s"]
    print(f"B {B}: ppo {res['pc_ppo_minibatch']['median_s'] * 1e6:.1f} us, bc {res['pc_bc_minibatch']['median_s'] * 1e6:.1f} us "
          f"(no target {res['pc_bc_minibatch_no_target']['median_s'] * 1e6:.1f} us), ratio {res['bc_over_ppo']:.3f}", file=sys.stderr, flush=True)
    return res


def main(out_path=os.path.join(ROOT, "profiles", "bc_timing.json"), reps=10):
    if not torch.cuda.is_available():
        raise SystemExit("bc_timing.py measures on the GPU: there is none")
    reps = int(reps)
    res = {"D": D, "A": A, "rows": M, "apply": 1, "reps": reps, "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around calls_per_window enqueues and a device synchronise, per call; 2 warm-up windows; medians",
           "shapes": [shape(B, reps) for B in (64, 512, 1024)]}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(*sys.argv[1:3])
