#!/usr/bin/env python3
"""Developer tool: static instruction counts per kernel of a device assembly file (hipcc -S --cuda-device-only), optionally as a
diff against a second file.  Static counts say nothing about trip counts; they are a quick regression screen for a compiler flag
or a source change across ALL kernels of the translation unit.

    python tools/asm_counts.py base.s [other.s] [--filter REGEX]

--sequence (needs other.s): per kernel of base.s, whether other.s holds the SAME instruction sequence, operands included (comments and
the numbering of branch labels aside), with the instruction counts and the code-object resources of both: (VGPRs incl. AGPRs, AGPRs,
SGPRs, VGPR spills, SGPR spills, scratch bytes, LDS bytes, kernel-argument bytes).  --rename 'OLD=NEW' (repeatable) pairs a kernel of
base.s with one of another demangled name in other.s.
"""
import argparse
import collections
import re
import subprocess


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\(.*", "", o).replace("void ", "") for o in out]


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_pk_"):
        return "pk"
    if op.startswith(("v_readlane", "v_writelane")):
        return "lane"
    if op.startswith("v_") and "_f64" in op:
        return "f64"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_nop"):
        return "nop"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_load"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    if op.startswith("scratch_"):
        return "scratch"
    return "other"


def parse(path):
    kernels = collections.OrderedDict()
    cur = None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = kernels.setdefault(m.group(1), collections.Counter())
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        t = line.strip()
        if not t or t.startswith((".", ";", "//")) or t.endswith(":"):
            continue
        op = t.split()[0]
        cur[classify(op)] += 1
        cur["total"] += 1
    return kernels


def sequences(path):
    """{symbol: [instruction lines, comments stripped, branch-label numbers normalised]}"""
    kernels, cur = collections.OrderedDict(), None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = line.split(";")[0].strip()
        if cur is None or not t or t.startswith((".", "//")) or t.endswith(":"):
            continue
        cur.append(re.sub(r"\.L(BB|tmp|func_begin|func_end)?\d+(_\d+)?", lambda m_: ".L" + (m_.group(2) or ""), " ".join(t.split())))
    return kernels


RES_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
            "group_segment_fixed_size", "kernarg_segment_size")


def resources(path):
    """{symbol: RES_KEYS values} from the amdhsa.kernels metadata at the end of the file"""
    out, cur = {}, {}
    for line in open(path):
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) in RES_KEYS:
            cur[m.group(1)] = int(m.group(2))
        elif m.group(1) == "symbol":
            cur["symbol"] = m.group(2).strip("'").removesuffix(".kd")
        if "symbol" in cur and all(k in cur for k in RES_KEYS):
            out[cur["symbol"]] = tuple(cur[k] for k in RES_KEYS)
            cur = {}
    return out


def compare_sequences(a):
    sb, so, rb, ro = sequences(a.base), sequences(a.other), resources(a.base), resources(a.other)
    db, do = dict(zip(sb, demangle(list(sb)))), dict(zip(so, demangle(list(so))))
    by_name = {v: k for k, v in do.items()}
    rename = dict(r.split("=", 1) for r in a.rename)
    same = diff = 0
    for n in sb:
        if n not in rb or not re.search(a.filter, db[n]):       # (device functions have no metadata entry: not kernels)
            continue
        target = rename.get(db[n], db[n])
        o = by_name.get(target)
        if o is None:
            print(f"GONE      instr {len(sb[n]):5d}  {rb[n]}  {db[n]}")
            continue
        seq_same, res_same = sb[n] == so[o], rb[n][:7] == ro[o][:7]
        same, diff = same + (seq_same and res_same), diff + (not (seq_same and res_same))
        verdict = "identical" if seq_same and res_same else ("resources" if seq_same else "DIFFERENT")
        if a.all or not (seq_same and res_same) or target != db[n] or rb[n][7] != ro[o][7]:
            print(f"{verdict:9s} instr {len(sb[n]):5d} -> {len(so[o]):5d}  {rb[n]} -> {ro[o]}  {db[n]}" + (f" -> {target}" if target != db[n] else ""))
            if not seq_same and len(sb[n]) == len(so[o]):       # (same length: say which lines differ, a few of them)
                lines = [(x, y) for x, y in zip(sb[n], so[o]) if x != y]
                for x, y in lines[:4]:
                    print(f"            {x}  ->  {y}")
                print(f"            {len(lines)} line(s) differ")
    for o in so:
        if o in ro and do[o] not in {rename.get(v, v) for v in db.values()} and re.search(a.filter, do[o]):
            print(f"NEW       instr {len(so[o]):5d}  {ro[o]}  {do[o]}")
    print(f"kernels compared {same + diff}: identical {same}, different {diff}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequence", action="store_true", help="compare instruction sequences and resources instead of counts")
    ap.add_argument("--rename", action="append", default=[], help="OLD=NEW: demangled kernel names to pair (with --sequence)")
    ap.add_argument("--all", action="store_true", help="with --sequence: list identical kernels too")
    ap.add_argument("base")
    ap.add_argument("other", nargs="?")
    ap.add_argument("--filter", default=".")
    a = ap.parse_args()
    if a.sequence:
        return compare_sequences(a)
    kb = parse(a.base)
    ko = parse(a.other) if a.other else None
    names = list(kb)
    dn = dict(zip(names, demangle(names)))
    cols = ["total", "valu", "pk", "f64", "mfma", "lane", "salu", "smem", "lds", "vmem", "scratch", "wait", "nop"]
    print(f"{'kernel':64s} " + " ".join(f"{c:>7s}" for c in cols))
    for n in names:
        if not re.search(a.filter, dn[n]):
            continue
        row = kb[n]
        if ko is None:
            print(f"{dn[n][:64]:64s} " + " ".join(f"{row[c]:7d}" for c in cols))
        elif n in ko:
            d = {c: ko[n][c] - row[c] for c in cols}
            if any(d.values()):
                print(f"{dn[n][:64]:64s} " + " ".join(f"{row[c]:7d}" if c == "total" else f"{d[c]:+7d}" for c in cols) + f"  (total {d['total']:+d})")


if __name__ == "__main__":
    main()
