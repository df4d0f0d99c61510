"""Developer probe (GPU box): which kernel the C-ABI launches, over a grid of configurations, T = 2 steps per call.  One line per call:
the configuration, the return code and pc_env_last_rollout_kernel / pc_env_last_step_kernel.  Covers pc_rollout (dtype x track layout x
nominal rays x n_envs x policy precision at default options; each PC_OPT_ROLLOUT_FORM / _EPW / _FAST value singly on a reduced grid; an
F64 state off the rotation table through pc_env_set_state), pc_env_step with each PC_OPT_STEP_FORM, pc_env_step_many, and pc_policy_act
with split -1 / 0 / 1.

Under `rocprofv3 --kernel-trace` against two builds, the printed lines and the ordered trace rows (kernel name with its template
arguments, grid, workgroup, LDS) must be identical for a change to the host-side dispatch that keeps behaviour:

    python tools/dispatch_sweep.py [--pkg DIR] [--quick]     (DIR holds _capi.py and libppocar.so; default: ppo-car_amd/)
"""
import argparse
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(ROOT, "ppo-car_amd"))
ap.add_argument("--quick", action="store_true", help="a small subset (a smoke test of the tool itself)")
args = ap.parse_args()
spec = importlib.util.spec_from_file_location("_capi_sweep", os.path.join(args.pkg, "_capi.py"))
capi = importlib.util.module_from_spec(spec)
spec.loader.exec_module(capi)
lib = capi.lib

DEV, T, A, H = 0, 2, 9, 256
PC_OPT_STEP_FORM = 4
TRACK_FILES = {k: os.path.join(ROOT, "tracks", f"{k}.json") for k in ("track", "big_track", "oval64")}
# track layouts: the track files of the batch and the per-env track id (None: a single track)
LAYOUTS = {
    "track": (["track"], None),
    "big_track": (["big_track"], None),
    "oval64": (["oval64"], None),
    "halves": (["track", "big_track"], lambda n: (np.arange(n) >= n // 2).astype(np.uint8)),
    "inter": (["track", "big_track"], lambda n: (np.arange(n) & 1).astype(np.uint8)),
    "uneven": (["track", "big_track"], lambda n: (np.arange(n) % 3 == 0).astype(np.uint8)),
    "blocks128": (["track", "big_track"], lambda n: ((np.arange(n) >> 7) & 1).astype(np.uint8)),
}
tracks = {}
for k, path in TRACK_FILES.items():
    t = C.c_void_p()
    capi.check(lib.pc_track_load_json(path.encode(), C.byref(t)), f"load {path}")
    tracks[k] = t


def ptr(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def make_env(dtype, layout, rays, n):
    names, tid_fn = LAYOUTS[layout]
    arr = (C.c_void_p * len(names))(*[tracks[k].value for k in names])
    tid = tid_fn(n) if tid_fn else None
    e = C.c_void_p()
    rc = lib.pc_env_create(DEV, n, rays, arr, len(names), tid.ctypes.data_as(C.c_void_p) if tid is not None else None,
                           capi.DTYPES[dtype], C.byref(e))
    if rc != capi.PC_OK:
        return None, rc
    D = lib.pc_env_obs_dim(e)
    obs = torch.empty(n, D, device="cuda")
    capi.check(lib.pc_env_reset(e, ptr(obs), None), "reset")
    return e, D


policies = {}


def policy(D, prec):
    """(handle, image) of a policy with fixed pseudo-random weights for width D, precision prec"""
    if (D, prec) not in policies:
        p = C.c_void_p()
        rc = lib.pc_policy_create(DEV, D, H, A, prec, -1, C.byref(p))
        if rc != capi.PC_OK:
            policies[(D, prec)] = (None, rc)
        else:
            nimg = C.c_int64()
            capi.check(lib.pc_policy_get(p, None, None, C.byref(nimg)), "policy_get")
            g = torch.Generator(device="cuda").manual_seed(D * 10 + prec)
            w = [torch.randn(s, device="cuda", generator=g) * 0.05 for s in ((H, D), (H,), (A, H), (A,), (H, D), (H,), (1, H), (1,))]
            img = torch.zeros(nimg.value, device="cuda")
            capi.check(lib.pc_policy_pack(p, *[ptr(x) for x in w], ptr(img), None), "pack")
            policies[(D, prec)] = (p, img)
    return policies[(D, prec)]


def rollout(e, D, n, prec):
    p, img = policy(D, prec)
    if p is None:
        return f"policy rc={img}"
    f = lambda *s: torch.empty(*s, device="cuda")
    bufs = [f(T, n, D)] + [f(T, n) for _ in range(6)] + [f(n, D), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), f(n), f(n)]
    rc = lib.pc_rollout(e, p, ptr(img), T, 0.1, 7, 0, None, *[ptr(b) for b in bufs], None)
    torch.cuda.synchronize()
    return f"rc={rc} kernel={capi.PC_KERNEL_NAMES.get(lib.pc_env_last_rollout_kernel(e))}"


def steps(e, D, n):
    out = []
    for sf in (0, 1, 2):
        capi.check(lib.pc_env_set_option(e, PC_OPT_STEP_FORM, sf), "step_form")
        act = torch.randint(0, 9, (T, n), device="cuda", dtype=torch.int64, generator=torch.Generator(device="cuda").manual_seed(n))
        obs, rew, term, trunc = (torch.empty(T, n, D, device="cuda"), torch.empty(T, n, device="cuda"), torch.empty(T, n, device="cuda"),
                                 torch.empty(T, n, device="cuda"))
        rc1 = lib.pc_env_step(e, ptr(act[0]), 0.1, ptr(obs[0]), ptr(rew[0]), ptr(term[0]), ptr(trunc[0]), None, None, None)
        k1 = capi.PC_STEP_NAMES.get(lib.pc_env_last_step_kernel(e))
        rc2 = lib.pc_env_step_many(e, ptr(act), T, 0.1, ptr(obs), ptr(rew), ptr(term), ptr(trunc), None)
        k2 = capi.PC_STEP_NAMES.get(lib.pc_env_last_step_kernel(e))
        torch.cuda.synchronize()
        out.append(f"step_form={sf} step rc={rc1} kernel={k1} step_many rc={rc2} kernel={k2}")
    capi.check(lib.pc_env_set_option(e, PC_OPT_STEP_FORM, 0), "step_form")
    return out


quick = args.quick
DTYPES = ("f32", "f64")
RAYS = (12, 16, 32, 20)
NS = (64, 4096, 4100, 8192, 8200, 32768, 32800, 65536) if not quick else (4096, 32768)
PRECS = (0, 1, 2)

# 1. pc_rollout at default options
for dtype in DTYPES:
    for layout in ("track", "big_track", "oval64", "halves", "inter", "uneven"):
        for rays in RAYS:
            for n in NS:
                e, D = make_env(dtype, layout, rays, n)
                if e is None:
                    print(f"rollout {dtype} {layout} rays={rays} n={n} create rc={D}", flush=True)
                    continue
                for prec in PRECS:
                    print(f"rollout {dtype} {layout} rays={rays} n={n} prec={prec} {rollout(e, D, n, prec)}", flush=True)
                lib.pc_env_destroy(e)

# 2. each rollout option value singly, on a reduced grid (blocks128: a batch mixed in blocks of 128 envs, below EPW = 256)
OPTS = [(capi.PC_OPT_ROLLOUT_FORM, v) for v in (-1, 0, 1, 2, 3, 4)] + [(capi.PC_OPT_ROLLOUT_EPW, v) for v in (0, 16, 32, 128, 256)] + \
       [(capi.PC_OPT_ROLLOUT_FAST, v) for v in (0, 1, 2, 3)]
DEFAULTS = ((capi.PC_OPT_ROLLOUT_FORM, -1), (capi.PC_OPT_ROLLOUT_EPW, 0), (capi.PC_OPT_ROLLOUT_FAST, 1))
for dtype in DTYPES:
    for layout in ("track", "big_track", "halves", "inter", "blocks128"):
        for rays in (12, 16, 32):
            for n in ((4096, 16384, 65536) if not quick else (16384,)):
                e, D = make_env(dtype, layout, rays, n)
                for prec in (0, 2):
                    for opt, v in OPTS:
                        capi.check(lib.pc_env_set_option(e, opt, v), "set_option")
                        print(f"rollout {dtype} {layout} rays={rays} n={n} prec={prec} opt{opt}={v} {rollout(e, D, n, prec)}", flush=True)
                        for o, d in DEFAULTS:
                            capi.check(lib.pc_env_set_option(e, o, d), "set_option")
                # form 4 with 256 envs per workgroup
                capi.check(lib.pc_env_set_option(e, capi.PC_OPT_ROLLOUT_FORM, 4), "set_option")
                capi.check(lib.pc_env_set_option(e, capi.PC_OPT_ROLLOUT_EPW, 256), "set_option")
                print(f"rollout {dtype} {layout} rays={rays} n={n} prec=2 form=4 epw=256 {rollout(e, D, n, 2)}", flush=True)
                lib.pc_env_destroy(e)

# 3. an F64 state off the rotation table (2.5 degrees off the 5-degree grid)
for layout in ("track", "big_track"):
    for n in (4096, 32768, 65536):
        e, D = make_env("f64", layout, 16, n)
        info = (C.c_double * 3)()
        capi.check(lib.pc_track_info(tracks[layout], None, None, info), "track_info")
        rot = np.full(n, info[2] + 2.5)
        capi.check(lib.pc_env_set_state(e, None, None, None, None, rot.ctypes.data_as(C.c_void_p), None, None, None), "set_state")
        print(f"rollout f64 {layout} rays=16 n={n} prec=2 offgrid {rollout(e, D, n, 2)}", flush=True)
        for line in steps(e, D, n):
            print(f"steps f64 {layout} rays=16 n={n} offgrid {line}", flush=True)
        lib.pc_env_destroy(e)

# 4. pc_env_step (each step form) and pc_env_step_many
for dtype in DTYPES:
    for layout in ("track", "big_track", "halves", "inter", "blocks128"):
        for rays in RAYS:
            for n in ((64, 4096, 8192, 65536) if not quick else (8192,)):
                e, D = make_env(dtype, layout, rays, n)
                for line in steps(e, D, n):
                    print(f"steps {dtype} {layout} rays={rays} n={n} {line}", flush=True)
                lib.pc_env_destroy(e)

# 5. pc_policy_act
for rays, D in ((12, 18), (16, 23), (32, 39)):
    for prec in PRECS:
        for split in (-1, 0, 1):
            p = C.c_void_p()
            capi.check(lib.pc_policy_create(DEV, D, H, A, prec, split, C.byref(p)), "policy_create")
            _, img = policy(D, prec)
            for n in ((64, 4096, 8192, 8200, 65536) if not quick else (8192,)):
                obs = torch.randn(n, D, device="cuda")
                act, af, lp, val = (torch.empty(n, device="cuda", dtype=torch.int64), torch.empty(n, device="cuda"), torch.empty(n, device="cuda"),
                                    torch.empty(n, device="cuda"))
                rc = lib.pc_policy_act(p, ptr(obs), n, ptr(img), 7, 0, None, ptr(act), ptr(af), ptr(lp), ptr(val), None, None)
                torch.cuda.synchronize()
                print(f"policy_act D={D} prec={prec} split={split} n={n} rc={rc}", flush=True)
            lib.pc_policy_destroy(p)
print("done", flush=True)
