#!/usr/bin/env python3
"""Per-kernel resource figures of a built libppocar.so, from the gfx950 code object's metadata (no GPU needed), and the comparison of two
builds of the library.

    python tools/code_object_diff.py ppo-car_amd/libppocar.so                 # one JSON object per kernel symbol
    python tools/code_object_diff.py OLD/libppocar.so ppo-car_amd/libppocar.so  # what changed between two builds

A kernel's figures: VGPRs, SGPRs, spilled VGPRs / SGPRs, private-segment (scratch) bytes, LDS bytes (static) and code bytes (the symbol's
size in .text).  Comparing, a symbol is looked up under its own name and, where a build gave a kernel template one more trailing
`bool ... = false` parameter, under the name with that parameter dropped (`...Lb0EEv` -> `...Ev`): the same instantiation."""
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def code_object(lib, workdir):
    fat, co = os.path.join(workdir, "fat.bin"), os.path.join(workdir, "co.o")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(workdir, "unused.so")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={co}", "--unbundle"])
    return co


def kernel_figures(lib):
    """{kernel symbol: {field: int, ..., "code_bytes": int}}"""
    with tempfile.TemporaryDirectory() as d:
        co = code_object(lib, d)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in notes.split("\n"):
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)      # amdhsa.kernels: an entry opens with "  - .key:", its keys sit at indent 4
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        key, val = m.group(2), m.group(3).strip().strip("'\"")
        if key in FIELDS:
            cur[key] = int(val)
        elif key == "symbol":
            out[val[:-3] if val.endswith(".kd") else val] = cur
    sizes = {}
    for line in syms.split("\n"):
        p = line.split()
        if len(p) >= 8 and p[3] == "FUNC":
            sizes[p[7]] = int(p[2])
    res = {}
    for name, f in out.items():
        res[name] = {k: f.get(k) for k in FIELDS}
        res[name]["code_bytes"] = sizes.get(name)
    return res


def without_trailing_false(name):
    return re.sub(r"Lb0EEv", "Ev", name, count=1)


def compare(old, new):
    """(identical, changed, missing, added): symbols of `old` found in `new` under their own name or with one trailing false parameter"""
    by_old_name = {}
    for n in new:
        by_old_name.setdefault(n, n)
        by_old_name.setdefault(without_trailing_false(n), n)
    same, changed, missing = [], [], []
    for n, f in old.items():
        m = by_old_name.get(n)
        if m is None:
            missing.append(n)
        elif new[m] == f:
            same.append(n)
        else:
            changed.append((n, f, new[m]))
    matched = {by_old_name[n] for n in old if n in by_old_name}
    return same, changed, missing, sorted(set(new) - matched)


def main(argv):
    if len(argv) == 1:
        for name, f in sorted(kernel_figures(argv[0]).items()):
            print(json.dumps({"kernel": name, **f}))
        return 0
    old, new = kernel_figures(argv[0]), kernel_figures(argv[1])
    same, changed, missing, added = compare(old, new)
    print(json.dumps({"old_kernels": len(old), "new_kernels": len(new), "identical": len(same), "changed": len(changed), "missing": len(missing),
                      "added": len(added)}))
    for n, a, b in changed:
        print("changed", n, json.dumps(a), "->", json.dumps(b))
    for n in missing:
        print("missing", n)
    for n in added:
        print("added", n, json.dumps(new[n]))
    return 1 if changed or missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
