"""Time of pc_render_frames (K19, ppo_car_amd.Renderer.frames) on rows of a real evaluation -- the trained fixture
(tests/golden/policy_trained.npz) on big_track at 16 rays, 64 envs, sampled -- next to two yardsticks taken in the same session.

  python tools/render_timing.py [out.json] [reps]

Per (scale, M) in {2, 4} x {1024, 16384}: the host clock around the enqueue and a device synchronise, two warm-up calls and `reps` timed
ones (median and all); the bytes the launch stores and the rate that makes; beside it
  "fill"       a torch fill of a uint8 tensor of the frames' size: the achievable store rate (fill / render is the figure of merit);
  "rasterise"  the numpy line plotter render.rasterise per frame on the host (all there was before the kernel), at the same frame size.
The rows are the first M of the evaluation's [1000, 64, D] rows of what the policy saw, with each row's next gate; K18's one-off background
launch is timed too.  "video": the wall time of one Evaluator(video_envs=4, video_scale=4) evaluation end to end, split into the run,
the render launches, the device-to-host copies and the APNG encode.  Writes profiles/render_timing.json by default; one JSON line on
stdout.  No pass / fail gate."""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ppo_car_amd as pc  # noqa: E402
from ppo_car_amd.render import contact_sheet, rasterise, write_apng  # noqa: E402
from ppo_car_amd.renderer import Renderer  # noqa: E402

TRACK = os.path.join(ROOT, "tracks", "big_track.json")


def _wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _times(f, reps, warmup=2):
    for _ in range(warmup):
        _wall(f)
    ts = [_wall(f)[0] for _ in range(reps)]
    return {"median_s": statistics.median(ts), "min_s": min(ts), "all_s": ts}


def main(out_path=os.path.join(ROOT, "profiles", "render_timing.json"), reps=10):
    if not torch.cuda.is_available():
        raise SystemExit("render_timing.py measures on the GPU: there is none")
    from oracle.scenarios import load_trained_policy
    reps = int(reps)
    agent = pc.Agent(23, 9).cuda()
    load_trained_policy(agent)
    ev = pc.Evaluator(agent, TRACK, n_envs=64, num_rays=16, reward_scaling=0.1, device="cuda", seed=0, video_envs=64, video_scale=4)
    ev.run()
    torch.cuda.synchronize()
    D = ev.envs.obs_dim
    rows = ev._vid["obs"].reshape(-1, D)
    rew = ev._vid["rew"].cpu().numpy().astype(np.float64)
    gate = np.isin(np.rint(rew / ev.reward_scaling), (1.0, 11.0, -2.0, 8.0))
    done = (ev._vid["term"].cpu().numpy() != 0) | (ev._vid["trunc"].cpu().numpy() != 0)
    ng = np.zeros(rew.shape, np.int64)          # the running gate count of the episode in progress, per row
    for t in range(1, len(rew)):
        ng[t] = np.where(done[t - 1], 0, ng[t - 1] + gate[t - 1])
    G = ev.envs._tracks[0].n_gates
    next_gate = torch.from_numpy((ng % G).astype(np.int32).reshape(-1)).cuda()
    walls, gates = ev.envs._tracks[0].geometry()
    res = {"track": "big_track", "num_rays": 16, "policy": "tests/golden/policy_trained.npz", "device": torch.cuda.get_device_name(0),
           "reps": reps, "cases": []}
    for scale in (2, 4):
        r = Renderer(ev.envs, scale)
        res[f"background_scale_{scale}_s"] = _wall(r.background)[0]
        for M in (1024, 16384):
            out = torch.empty(M, r.H, r.W, 3, dtype=torch.uint8, device="cuda")
            o, g = rows[:M], next_gate[:M]
            t = _times(lambda: r.frames(o, next_gate=g, out=out), reps)
            fill = _times(lambda: out.fill_(7), reps)
            t0 = time.perf_counter()
            n_host = 8
            host_rows = o[:n_host].cpu().numpy()
            for k in range(n_host):
                rasterise(walls, gates, float(host_rows[k, 0]) * 1280.0, float(host_rows[k, 1]) * 720.0,
                          float(np.degrees(np.arctan2(host_rows[k, 5], host_rows[k, 4]))), host_rows[k, 6:], next_gate=int(g[k]),
                          num_rays_nominal=16, size=(r.W, r.H))
            host = (time.perf_counter() - t0) / n_host
            nbytes = out.numel()
            res["cases"].append({"scale": scale, "M": M, "frame": [r.H, r.W], "bytes_stored": nbytes, "render": t,
                                 "render_per_frame_s": t["median_s"] / M, "render_store_rate_GBps": nbytes / t["median_s"] / 1e9,
                                 "fill": fill, "fill_rate_GBps": nbytes / fill["median_s"] / 1e9,
                                 "render_over_fill": t["median_s"] / fill["median_s"], "numpy_rasterise_per_frame_s": host,
                                 "numpy_rasterise_frames_timed": n_host})
            del out
    ev.close()
    # one --video evaluation end to end: 64 envs, 4 of them in the video at scale 4, every second step
    ev = pc.Evaluator(agent, TRACK, n_envs=64, num_rays=16, reward_scaling=0.1, device="cuda", seed=0, video_envs=4, video_scale=4)
    t_run = _wall(ev.run)[0]
    steps, ng4, lengths = ev.video_plan()
    F, K = steps.shape
    t_idx = torch.from_numpy(steps.reshape(-1)).cuda()
    k_idx = torch.arange(K, device="cuda").repeat(F)
    sel = ev._vid["obs"][t_idx, k_idx]
    g4 = torch.from_numpy(ng4.reshape(-1)).cuda()
    t_render, dev = _wall(lambda: [ev._renderer.frames(sel[a:a + 256], next_gate=g4[a:a + 256]) for a in range(0, F * K, 256)])
    t_d2h, host = _wall(lambda: np.concatenate([d.cpu().numpy() for d in dev]))
    t0 = time.perf_counter()
    host = host.reshape(F, K, *host.shape[1:])
    sheets = np.stack([contact_sheet(host[f], 2) for f in range(F)])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "video.png")
        write_apng(path, sheets)
        size = os.path.getsize(path)
    t_encode = time.perf_counter() - t0
    t_all = _wall(lambda: (ev.run(), ev.video_frames()))[0]
    res["video"] = {"n_envs": 64, "video_envs": K, "video_scale": 4, "frames": F, "episode_lengths": lengths.tolist(), "run_s": t_run,
                    "render_s": t_render, "device_to_host_s": t_d2h, "sheets_and_encode_s": t_encode, "file_bytes": size,
                    "run_plus_video_frames_s": t_all}
    ev.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "cases"} | {"cases": [
        {k: c[k] for k in ("scale", "M", "render_per_frame_s", "render_store_rate_GBps", "fill_rate_GBps", "render_over_fill",
                           "numpy_rasterise_per_frame_s")} for c in res["cases"]]}))


if __name__ == "__main__":
    main(*sys.argv[1:])
