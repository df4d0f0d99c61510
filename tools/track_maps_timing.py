"""Time of one pc_track_maps launch (K16, ppo_car_amd.TrackMaps.update) at the benchmark's size -- 65536 envs x 1024 steps, 16 rays,
big_track, cell_px 8 -- next to two yardsticks taken in the same session on the same buffer.

  python tools/track_maps_timing.py [out.json] [reps] [n_envs] [n_steps]

  (a) "rollout": the buffer of a real training rollout (the second epoch's: the first one's update has run), all n_steps rows;
  (b) "reset":   32 rows taken straight after a reset -- every env in ONE cell for the first rows, the all-in-one-cell worst case.
Per input: the host clock around the enqueue of a few calls and a device synchronise, two warm-up windows and `reps` timed ones (median and all), the
bytes the launch has to read (every cache line of obs_buf is touched: 4 D bytes per sample, plus one flag row) and the rate that
makes.  Yardsticks on (a): obs_buf.clone() (reads and writes the buffer: twice the bytes) and the epoch's GAE launch
(Buffer.calculate_advantages).  The maps of every timed call are checked against the first call's (integer adds: the same counts,
whatever the order).  Writes profiles/track_maps_timing.json by default; one JSON line on stdout.  No pass / fail gate."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ppo_car_amd as pc  # noqa: E402
from ppo_car_amd.ppo import PPOConfig, Trainer  # noqa: E402

TRACK = os.path.join(ROOT, "tracks", "big_track.json")


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


def maps_times(tr, reps, inner):
    buf = tr.buffer
    T, N, D = buf.obs_buf.shape
    maps = pc.TrackMaps(1, 8, tr.device)
    upd = lambda: maps.update(buf.obs_buf, buf.term_buf, buf.trunc_buf, tr.next_term, tr.next_trunc)
    upd()
    torch.cuda.synchronize()
    first = maps.counts.clone()
    maps.clear()
    res = _times(upd, reps, inner=inner)
    calls = (2 + reps) * inner
    same = bool(torch.equal(maps.counts, first * calls))
    v = first[0, 0]
    read = T * N * (4 * D + 4)
    res.update({"rows": T, "n_envs": N, "obs_dim": D, "per_row_s": res["median_s"] / T, "bytes_read": read,
                "read_rate_GBps": read / res["median_s"] / 1e9, "every_call_gave_the_same_counts": same,
                "visits": int(v.sum()), "cells_visited": int((v > 0).sum()), "largest_cell_share": float(v.max()) / float(v.sum()),
                "crashes": int(first[0, 2].sum())})
    return res


def main(out_path=os.path.join(ROOT, "profiles", "track_maps_timing.json"), reps=10, n_envs=65536, n_steps=1024):
    if not torch.cuda.is_available():
        raise SystemExit("track_maps_timing.py measures on the GPU: there is none")
    reps, N, T = int(reps), int(n_envs), int(n_steps)
    cfg = dict(n_envs=N, batch_size=512, train_iters=40, track=TRACK, num_rays=16, seed=0)
    tr = Trainer(PPOConfig(n_steps=T, **cfg), device="cuda")
    tr.run_epoch()
    tr.rollout()            # the second epoch's rollout: (a)
    torch.cuda.synchronize()
    buf = tr.buffer
    a = maps_times(tr, reps, inner=5)
    clone = _times(lambda: buf.obs_buf.clone(), reps)
    clone["bytes_moved"] = 2 * buf.obs_buf.numel() * 4
    clone["rate_GBps"] = clone["bytes_moved"] / clone["median_s"] / 1e9
    with torch.no_grad():
        nv = tr.agent.get_value(tr.next_obs).reshape(1, -1)
        gae = _times(lambda: buf.calculate_advantages(nv, tr.next_term.reshape(1, -1), tr.next_trunc.reshape(1, -1)), reps)
    mode = tr.rollout_mode
    tr.close()
    del tr, buf
    torch.cuda.empty_cache()
    tr = Trainer(PPOConfig(n_steps=32, **cfg), device="cuda")
    tr.rollout()            # 32 rows from the reset: (b)
    torch.cuda.synchronize()
    b = maps_times(tr, reps, inner=50)
    tr.close()
    res = {"track": "big_track", "num_rays": 16, "cell_px": 8, "reps": reps, "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around calls_per_window enqueues and a device synchronise, per call; 2 warm-up windows", "rollout_mode": mode,
           "rollout": a, "reset_32_rows": b, "obs_buf_clone": clone, "gae_launch": gae,
           "ratios": {"maps_over_clone": a["median_s"] / clone["median_s"], "maps_over_gae": a["median_s"] / gae["median_s"],
                      "reset_per_row_over_rollout_per_row": b["per_row_s"] / a["per_row_s"]}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(*sys.argv[1:5])
