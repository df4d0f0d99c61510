"""The host-side track-table compiler (csrc/track_tables.cpp: what pc_env_create uploads, and every bit-exactness claim of the env
kernels rests on) built with AddressSanitizer + UndefinedBehaviorSanitizer into a small driver and run as a child process: no GPU,
nothing loaded into Python.

The driver compiles a grid of tracks x ray counts x dtypes and prints, per table, its element count and an FNV-1a-64 hash over its
fields, the per-track header fields and the TrackFacts.  Those lines must equal tests/golden/track_tables.json, which was recorded
from the commit BEFORE the compiler left ppocar.hip (profiles/track_tables_refactor.txt has the provenance) -- so the tables are
the same bytes.  Independent of the fixture, the driver checks the tables' structure (chain neighbours, scan flags, index mask),
looks up every angle of every F64 rotation row in the angle hash table by the device's probe rule, and classifies track_id
layouts; the limits (8192 vertices, 2000 px) answer as before."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppo-car_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "track_tables.json")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off"]

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "ppocar_internal.h"

// One line per table: name, element count, FNV-1a-64 over the elements' bytes (the records have no implicit padding; TrackHdr has,
// so it is hashed field by field, start_collides -- the device's -- left out).
static inline uint64_t dump_fnv(const void* p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}
template <class V> static void dump_vec(FILE* f, const char* name, const V& v) {
    std::fprintf(f, "%s %zu %016llx\n", name, v.size(), (unsigned long long)dump_fnv(v.data(), v.size() * sizeof(v[0])));
}
template <class Hdrs, class Facts, class RotIds, class RotDepth, class A, class B, class C, class D, class E, class F, class G, class H>
static void dump_tables(FILE* f, const Hdrs& hdr, const Facts& tf, size_t rden_floats, const RotIds& rot_ids, const RotDepth& rot_depth,
                        const A& segs, const B& vtx, const C& vtxp, const D& seg64, const E& headtab, const F& dirtab, const G& dirtab64,
                        const H& dirhash) {
    dump_vec(f, "segs", segs);
    dump_vec(f, "vtx", vtx);
    dump_vec(f, "vtxp", vtxp);
    dump_vec(f, "seg64", seg64);
    dump_vec(f, "headtab", headtab);
    dump_vec(f, "dirtab", dirtab);
    dump_vec(f, "dirtab64", dirtab64);
    dump_vec(f, "dirhash", dirhash);
    uint64_t hh = 0xcbf29ce484222325ull;
    for (const auto& h : hdr) {
#define DUMP_F(x) hh = dump_fnv(&h.x, sizeof h.x, hh)
        DUMP_F(wall_off); DUMP_F(S); DUMP_F(gate_off); DUMP_F(G); DUMP_F(head_off); DUMP_F(vtx_off); DUMP_F(nV); DUMP_F(dir_off);
        DUMP_F(rden_off); DUMP_F(n_chain); DUMP_F(idx_mask); DUMP_F(start_x); DUMP_F(start_y); DUMP_F(start_rot); DUMP_F(ax0); DUMP_F(ay0);
        DUMP_F(bx0); DUMP_F(bx1); DUMP_F(by0); DUMP_F(by1); DUMP_F(n_scan); DUMP_F(brk2); DUMP_F(vtxp_off); DUMP_F(rot_off); DUMP_F(n_rot);
        DUMP_F(lat_off); DUMP_F(sel_ok);
#undef DUMP_F
    }
    std::fprintf(f, "hdr %zu %016llx\n", hdr.size(), (unsigned long long)hh);
    std::fprintf(f, "rden_floats %zu\n", rden_floats);
    for (size_t k = 0; k < hdr.size(); ++k) {
        const auto& h = hdr[k];
        std::fprintf(f, "track %zu n_chain %d nV %d brk2 %d vtxp_off %d n_scan %d n_rot %d sel_ok %d idx_mask %u rden_off %d\n", k, h.n_chain, h.nV,
                     h.brk2, h.vtxp_off, h.n_scan, h.n_rot, h.sel_ok, h.idx_mask, h.rden_off);
        std::vector<uint64_t> keys(rot_ids[k].size());          // rotation bits by row
        for (const auto& kv : rot_ids[k]) keys[(size_t)kv.second] = kv.first;
        std::fprintf(f, "rot_ids %zu %zu %016llx\n", k, keys.size(), (unsigned long long)dump_fnv(keys.data(), keys.size() * 8));
        std::fprintf(f, "rot_depth %zu %zu %016llx\n", k, rot_depth[k].size(),
                     (unsigned long long)dump_fnv(rot_depth[k].data(), rot_depth[k].size() * sizeof(int)));
    }
    std::fprintf(f, "facts max_G %d max_nV %d sum_nV %d tabs %d rden %d sel %d nv28 %d loops %d\n", tf.max_G, tf.max_nV, tf.sum_nV, (int)tf.tabs,
                 (int)tf.rden, (int)tf.sel, (int)tf.nv28, (int)tf.loops);
}

static uint64_t bits_of(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
static bool vtx_start(const Vtx& v) { return v.ex == 0.f && v.ey == 0.f; }      // chain start / padding / a wall without length

// chain neighbours, scan flags, index mask: what the kernels rely on, whatever the fixture says
static void check_structure(const TrackTables& tt) {
    int starts = 0, flagged = 0;
    for (size_t t = 0; t < tt.hdr.size(); ++t) {
        const TrackHdr& h = tt.hdr[t];
        if (h.idx_mask + 1u < (unsigned)h.nV) { std::printf("check structure FAIL track %zu idx_mask %u nV %d\n", t, h.idx_mask, h.nV); return; }
        int n_flag = 0;
        for (int k = 0; k < h.nV; ++k) {
            const SegD& r = tt.seg64[h.vtx_off + k];
            if (k < h.n_chain && vtx_start(tt.vtx[h.vtx_off + k])) ++starts;
            const int prev = r.prev_next & 0x7fff, next = (int)(((unsigned)r.prev_next >> 16) & 0x7fff);
            for (const int nb : {prev, next})
                if (nb != 0 && !(nb >= 1 && nb < h.n_chain && !vtx_start(tt.vtx[h.vtx_off + nb]))) {
                    std::printf("check structure FAIL track %zu vertex %d neighbour %d\n", t, k, nb);
                    return;
                }
            if (r.prev_next & PC_SEG_SCAN) {
                ++n_flag;
                if (r.h != -1.0) { std::printf("check structure FAIL track %zu vertex %d flagged with h %g\n", t, k, r.h); return; }
            }
        }
        if (n_flag != h.n_scan) { std::printf("check structure FAIL track %zu n_scan %d flagged %d\n", t, h.n_scan, n_flag); return; }
        flagged += n_flag;
    }
    std::printf("check structure ok starts %d flagged %d\n", starts, flagged);
}

// F64: every angle of every rotation row, looked up as the device does (Math<double>::lookup), gives the row's own (cos, sin)
static void check_f64(const TrackTables& tt, int n_nominal, int R) {
    const int step_deg = 360 / n_nominal;
    size_t n_keys = 0;
    for (size_t t = 0; t < tt.hdr.size(); ++t) {
        const TrackHdr& h = tt.hdr[t];
        if (h.rot_off < 0) { std::printf("check f64 none (no rotation table)\n"); return; }
        const PairD* rows = tt.dirtab64.data() + h.rot_off;
        const auto rot_of = [&](int i) { return rows[(size_t)i * (R + 2) + R + 1].x; };
        if (bits_of(rot_of(0)) != bits_of(h.start_rot)) { std::printf("check f64 FAIL track %zu row 0 is not start_rot\n", t); return; }
        if ((int)tt.rot_ids[t].size() != h.n_rot || (int)tt.rot_depth[t].size() != h.n_rot) { std::printf("check f64 FAIL track %zu host maps\n", t); return; }
        const unsigned mask = (unsigned)h.head_off;
        for (int i = 0; i < h.n_rot; ++i) {
            const double rot = rot_of(i);
            const auto it = tt.rot_ids[t].find(bits_of(rot));
            if (it == tt.rot_ids[t].end() || it->second != i) { std::printf("check f64 FAIL track %zu row %d not in rot_ids\n", t, i); return; }
            const PairD lr = rows[(size_t)i * (R + 2) + R];
            if (lr.x >= 0 && bits_of(rot_of((int)lr.x)) != bits_of(rot - 5.0)) { std::printf("check f64 FAIL track %zu row %d left\n", t, i); return; }
            if (lr.y >= 0 && bits_of(rot_of((int)lr.y)) != bits_of(rot + 5.0)) { std::printf("check f64 FAIL track %zu row %d right\n", t, i); return; }
            if ((lr.x >= 0 && lr.x >= h.n_rot) || (lr.y >= 0 && lr.y >= h.n_rot)) { std::printf("check f64 FAIL track %zu row %d index\n", t, i); return; }
            for (int ray = 0; ray < R; ++ray) {
                const uint64_t key = bits_of(rot + (double)(ray * step_deg));
                const unsigned slot = f64dir_hash(key) & mask;
                int at = -1;
                for (int probe = 0; probe < F64DIR_MAX_PROBE; ++probe)
                    if (tt.dirhash[h.dir_off + ((slot + probe) & mask)].key == key) at = probe;
                if (at < 0) { std::printf("check f64 FAIL track %zu row %d ray %d not within the probe bound\n", t, i, ray); return; }
                const F64Dir& e = tt.dirhash[h.dir_off + ((slot + at) & mask)];
                const PairD cs = rows[(size_t)i * (R + 2) + ray];
                if (bits_of(e.c) != bits_of(cs.x) || bits_of(e.s) != bits_of(cs.y)) { std::printf("check f64 FAIL track %zu row %d ray %d (cos, sin)\n", t, i, ray); return; }
                ++n_keys;
            }
        }
    }
    std::printf("check f64 ok keys %zu\n", n_keys);
}

static void layout(const char* name, const std::vector<uint8_t>& id, int n_tracks) {
    const TrackLayout l = pc_internal_classify_track_ids(id.data(), (int64_t)id.size(), n_tracks);
    std::printf("layout %s track_block %d blocks32 %d bal64 %d bal32 %d\n", name, l.track_block, (int)l.blocks32, (int)l.bal64, (int)l.bal32);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {       // name dtype n_nominal track.json...
        std::istringstream ls(line);
        std::string name, path;
        int dtype = 0, n = 0;
        ls >> name >> dtype >> n;
        std::vector<pc_track> tracks;
        while (ls >> path) {
            tracks.emplace_back();
            if (pc_internal_parse_track(path.c_str(), &tracks.back()) != PC_OK) { std::printf("CANNOT PARSE %s\n", path.c_str()); return 3; }
        }
        std::vector<const pc_track*> ptrs;
        for (const pc_track& t : tracks) ptrs.push_back(&t);
        const int step = 360 / n, R = (360 + step - 1) / step;      // pc_ray_count
        TrackTables tt;
        std::string err;
        std::printf("case %s\n", name.c_str());
        const int rc = pc_internal_compile_tracks(ptrs.data(), (int)ptrs.size(), n, R, dtype, tt, err);
        if (rc != PC_OK) { std::printf("error %d %s\n", rc, err.c_str()); continue; }
        dump_tables(stdout, tt.hdr, tt.facts, tt.rden_floats, tt.rot_ids, tt.rot_depth, tt.segs, tt.vtx, tt.vtxp, tt.seg64, tt.headtab, tt.dirtab,
                    tt.dirtab64, tt.dirhash);
        check_structure(tt);
        if (dtype == PC_DTYPE_F64) check_f64(tt, n, R);
    }
    std::printf("case layouts\n");
    for (const int blk : {256, 128, 64, 32}) {      // one track per blk envs
        std::vector<uint8_t> id(4 * blk);
        for (size_t i = 0; i < id.size(); ++i) id[i] = (uint8_t)((i / blk) & 1);
        layout(("per" + std::to_string(blk)).c_str(), id, 2);
    }
    std::vector<uint8_t> id(128);
    for (size_t i = 0; i < id.size(); ++i) id[i] = (uint8_t)(i & 1);
    layout("interleaved128", id, 2);
    id.resize(96);
    layout("interleaved96", id, 2);
    id.assign(128, 0);
    for (size_t i = 0; i < id.size(); i += 4) id[i] = 1;
    layout("uneven128", id, 2);
    id.resize(96);
    for (size_t i = 0; i < id.size(); ++i) id[i] = (uint8_t)(i % 3);
    layout("three96", id, 3);
    return 0;
}
"""

GRID_TRACKS = ("big_track", "track", "oval64", "junction")
GRID_RAYS = (12, 16, 32)
DTYPES = {"f32": 0, "f64": 1}


def _write_track(path, outer, inner, start=(150.0, 200.0)):
    W, H = 1280.0, 720.0
    n = lambda pts: [[x / W, y / H] for x, y in pts]
    gates = [(60, 60), (61, 60), (70, 60), (71, 60)]
    with open(path, "w") as f:
        json.dump({"outer_track_points": n(outer), "inner_track_points": n(inner), "reward_gates": n(gates),
                   "initial_position": [start[0] / W, start[1] / H], "initial_angle": 0.0}, f)
    return path


def make_cases(tmp):
    """-> [(name, dtype, nominal rays, [track files])]: the cases of the fixture, in its order.  Writes the generated tracks under tmp."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from junction_track import _junction_track_json
    tmp = str(tmp)
    files = {name: os.path.join(ROOT, "tracks", name + ".json") for name in ("big_track", "track", "oval64")}
    files["junction"] = _junction_track_json(os.path.join(tmp, "junction.json"))
    # a zigzag polyline of 8200 walls inside 1000 x 600 px (more chain vertices than dtype f32 takes), a box wider than 2000 px, and
    # a box whose top wall is followed by a wall without length
    zigzag = [(100.0 + 0.1 * i, 100.0 + (i % 2) * 50.0 + 0.05 * i) for i in range(8201)]
    files["poly8200"] = _write_track(os.path.join(tmp, "poly8200.json"), zigzag, [(100, 700), (900, 700)])
    files["wide"] = _write_track(os.path.join(tmp, "wide.json"), [(0, 0), (2500, 0), (2500, 300), (0, 300), (0, 0)], [(60, 150), (2400, 150)])
    files["zerolen"] = _write_track(os.path.join(tmp, "zerolen.json"), [(50, 50), (650, 50), (650, 50), (650, 350), (50, 350), (50, 50)],
                                    [(300, 150), (420, 180), (520, 280)])
    cases = [(f"{t}_n{n}_{d}", DTYPES[d], n, [files[t]]) for t in GRID_TRACKS for n in GRID_RAYS for d in DTYPES]
    cases += [(f"two_{d}", DTYPES[d], 16, [files["big_track"], files["track"]]) for d in DTYPES]
    cases += [("seventeen_f64", 1, 12, [files[("big_track", "track", "oval64")[i % 3]] for i in range(17)])]     # n_tracks > 16: no rotation table
    cases += [(f"{t}_{d}", DTYPES[d], 12, [files[t]]) for t in ("poly8200", "wide", "zerolen") for d in DTYPES]
    return cases


def _compiler(tmp):
    """g++, or ROCm's clang++: the first that builds a sanitized program which runs here."""
    src = os.path.join(tmp, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    for cxx in ("g++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        exe = shutil.which(cxx)
        if exe is None:
            continue
        if subprocess.run([exe, src, "-o", os.path.join(tmp, "probe")] + SAN, capture_output=True).returncode == 0 and \
                subprocess.run([os.path.join(tmp, "probe")], capture_output=True).returncode == 0:
            return exe
    return None


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("track_tables")
    CXX = _compiler(str(tmp))
    if CXX is None:
        pytest.skip("needs g++ or clang++ with the sanitizer runtimes")
    (tmp / "driver.cpp").write_text(DRIVER)
    exe = tmp / "driver"
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + SAN + [f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", str(tmp / "driver.cpp"),
           os.path.join(CSRC, "track_json.cpp"), os.path.join(CSRC, "track_tables.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    cases = make_cases(tmp)
    (tmp / "cases.txt").write_text("".join(f"{name} {dtype} {n} {' '.join(paths)}\n" for name, dtype, n, paths in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(tmp / "cases.txt")], capture_output=True, text=True, env=env, timeout=600)
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("case "):
            cur = out.setdefault(line[5:], [])
        else:
            cur.append(line)
    return r, out, [c[0] for c in cases]


def _fields(line):
    """'track 0 n_chain 26 nV 28 ...' -> {'n_chain': 26, 'nV': 28, ...}"""
    w = line.split()
    return {w[i]: int(w[i + 1]) for i in range(2 if w[0] == "track" else 1, len(w) - 1, 2)}


def _track(lines, k=0):
    return _fields(next(l for l in lines if l.startswith(f"track {k} ")))


def _facts(lines):
    return _fields(next(l for l in lines if l.startswith("facts ")))


def test_the_sanitized_run_is_clean(run):
    r, out, names = run
    assert r.returncode == 0, f"driver failed (rc {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "ERROR: LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert list(out) == names + ["layouts"]
    assert not [l for lines in out.values() for l in lines if "FAIL" in l]


def test_every_table_equals_the_recording_of_the_previous_compiler(run):
    _, out, names = run
    golden = json.load(open(FIXTURE))["cases"]
    assert sorted(golden) == sorted(names)
    for name in names:
        got = [l for l in out[name] if not l.startswith("check ")]
        assert got == golden[name], name


def test_chain_structure(run):
    _, out, _ = run
    for n in GRID_RAYS:
        for d in DTYPES:
            big, trk, oval, junc = (out[f"{t}_n{n}_{d}"] for t in GRID_TRACKS)
            h = _track(big)
            assert (h["n_chain"], h["nV"], h["brk2"]) == (26, 28, 13) and h["vtxp_off"] >= 0
            assert _facts(big)["nv28"] == 1 and _facts(big)["loops"] == 1
            h = _track(trk)
            assert (h["n_chain"], h["nV"], h["brk2"]) == (18, 20, 9)
            assert _facts(trk)["nv28"] == 0 and _facts(trk)["loops"] == 1
            assert _facts(oval)["nv28"] == 0 and _facts(oval)["loops"] == 0
            # the T-junction's two walls and the crossing's two, of nine (tests/junction_track.py)
            assert _track(junc)["n_scan"] == 4 and "check structure ok starts 2 flagged 4" in junc
    for name, lines in out.items():
        if name != "layouts" and not lines[0].startswith("error "):
            assert any(l.startswith("check structure ok ") for l in lines), name
            for k in range(sum(l.startswith("track ") for l in lines)):
                h = _track(lines, k)
                assert h["idx_mask"] + 1 >= h["nV"] and h["nV"] % 4 == 0 and h["n_chain"] <= h["nV"], (name, k)


def test_f64_angles_are_found_by_the_devices_probe_rule(run):
    _, out, names = run
    for name in names:
        lines = out[name]
        if name.endswith("_f64") and not lines[0].startswith("error "):
            check = next(l for l in lines if l.startswith("check f64 "))
            if name == "seventeen_f64":
                assert check == "check f64 none (no rotation table)" and all(_track(lines, k)["n_rot"] == 0 for k in range(17))
            else:
                assert check.startswith("check f64 ok keys ") and int(check.split()[-1]) > 0, (name, check)
                assert _track(lines)["n_rot"] > 0


def test_limits(run):
    _, out, _ = run
    assert out["poly8200_f32"] == ["error -5 track 0: 8204 chain vertices; dtype f32 takes at most 8192 (use dtype f64)"]
    assert out["wide_f32"] == ["error -5 track 0: the walls' bounding box exceeds 2000 px; dtype f32 is priced for tracks that fit (use dtype f64)"]
    for name in ("poly8200_f64", "wide_f64"):
        h = _track(out[name])
        assert h["sel_ok"] == 0 and h["rden_off"] == -1 and h["n_scan"] == 0, name
        assert _facts(out[name])["sel"] == 0 and _facts(out[name])["rden"] == 0
    assert _track(out["poly8200_f64"])["nV"] == 8204
    for d in DTYPES:      # the wall without length is a chain start: three starts where the two chains alone have two
        assert any(l.startswith("check structure ok starts 3 ") for l in out[f"zerolen_{d}"]), out[f"zerolen_{d}"]
        assert _track(out[f"zerolen_{d}"])["brk2"] == -1


def test_track_id_layouts(run):
    _, out, _ = run
    got = {l.split()[1]: _fields(l.split(None, 1)[1]) for l in out["layouts"]}
    L = lambda tb, b32, b64, bal32: {"track_block": tb, "blocks32": b32, "bal64": b64, "bal32": bal32}
    assert got == {"per256": L(256, 1, 0, 0), "per128": L(128, 1, 0, 0), "per64": L(64, 1, 0, 0), "per32": L(32, 1, 1, 0),      # (32 envs of each track in every block of 64: split evenly, though not interleaved)
                   "interleaved128": L(0, 0, 1, 1), "interleaved96": L(0, 0, 0, 1), "uneven128": L(0, 0, 0, 0), "three96": L(0, 0, 0, 0)}
