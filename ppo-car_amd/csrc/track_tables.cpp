// track_tables.cpp -- the tracks compiled into the tables the env kernels read (TrackTables, ppocar_internal.h), and the layout of a
// track_id array.  Host arithmetic only: pc_env_create uploads the result.  Every bit-exactness claim of the env kernels rests on
// these tables, so the unit is built with -ffp-contract=off like the kernels, and it runs -- and is tested -- without a GPU.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <unordered_set>

#include "ppocar_internal.h"

namespace {

// glibc's cos and sin, each through its own call: an optimiser that sees both of one argument may merge them into sincos(), whose
// cosine differs from cos() in the last place for some arguments -- and the tables below stand for the reference's separate
// np.cos / np.sin calls (car_env.py:426-427, :584)
__attribute__((noinline)) double libm_cos(double a) { return std::cos(a); }
__attribute__((noinline)) double libm_sin(double a) { return std::sin(a); }

uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
double val(uint64_t b) { double v; std::memcpy(&v, &b, 8); return v; }

struct Compiler {
    const int n_tracks, n_nominal, R;
    const bool f64;
    TrackTables& out;
    std::string& err;
    const int step_deg = 360 / n_nominal;      // 360 // n (car_env.py:269)
    std::vector<PairD> vpos;       // the chain vertices' exact positions (indexed like vtx); the only state the steps share beside `out`

    bool is_start(const TrackHdr& h, int k) const { return out.seg64[h.vtx_off + k].ex == 0.0 && out.seg64[h.vtx_off + k].ey == 0.0; }

    // walls and gates as the reference holds them; the walls again as vertex chains: a segment continues the chain iff it starts exactly
    // where the previous ended.  The sweep's float32 coordinates are relative to the ANCHOR = the centre of the vertices' bounding box.
    // -> wall_k: wall w = the segment closed by chain vertex wall_k[w]
    std::vector<int> chains_and_anchor(const pc_track* t, TrackHdr& h) {
        std::vector<Seg>& segs = out.segs;
        std::vector<Vtx>& vtx = out.vtx;
        std::vector<SegD>& seg64 = out.seg64;
        h.wall_off = (int)segs.size();
        for (size_t i = 0; i < t->walls.size(); i += 4) segs.push_back(Seg{t->walls[i], t->walls[i + 1], t->walls[i + 2], t->walls[i + 3]});
        h.gate_off = (int)segs.size();
        for (size_t i = 0; i < t->gates.size(); i += 4) segs.push_back(Seg{t->gates[i], t->gates[i + 1], t->gates[i + 2], t->gates[i + 3]});
        h.vtx_off = (int)vtx.size();
        {
            double bx0 = 1e300, bx1 = -1e300, by0 = 1e300, by1 = -1e300;
            for (int w = 0; w < h.S; ++w) {
                const Seg& sg = segs[h.wall_off + w];
                bx0 = std::min({bx0, sg.x1, sg.x2}); bx1 = std::max({bx1, sg.x1, sg.x2});
                by0 = std::min({by0, sg.y1, sg.y2}); by1 = std::max({by1, sg.y1, sg.y2});
            }
            h.ax0 = 0.5 * (bx0 + bx1);
            h.ay0 = 0.5 * (by0 + by1);
            h.bx0 = (float)bx0; h.bx1 = (float)bx1; h.by0 = (float)by0; h.by1 = (float)by1;
        }
        // the sweep's view of a wall's closing vertex: its anchor-relative position, the UNIT vector along (x1 - x2, y1 - y2)
        // (car_env.py:171) in float32, and that vector's copy scaled by 2^-40
        const auto edge = [&h](const Seg& sg) {
            const double ex = sg.x1 - sg.x2, ey = sg.y1 - sg.y2, len = std::hypot(ex, ey);
            const float xr = (float)(sg.x2 - h.ax0), yr = (float)(sg.y2 - h.ay0);
            if (len == 0.0) return Vtx{xr, yr, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};     // a wall without length is never hit: a chain start
            const float fx = (float)(ex / len), fy = (float)(ey / len);
            return Vtx{xr, yr, fx, fy, fx * 0x1p-40f, fy * 0x1p-40f, 0.f, 0.f};
        };
        std::vector<int> wall_k(h.S);
        for (int w = 0; w < h.S; ++w) {
            const Seg& sg = segs[h.wall_off + w];
            const bool cont = w > 0 && segs[h.wall_off + w - 1].x2 == sg.x1 && segs[h.wall_off + w - 1].y2 == sg.y1;
            if (!cont) {
                vtx.push_back(Vtx{(float)(sg.x1 - h.ax0), (float)(sg.y1 - h.ay0), 0.f, 0.f, 1.f, 0.f, 0.f, 0.f});   // chain start: zero edge (scaled copy (1, 0): see Sweep::cand)
                seg64.push_back(SegD{sg.x1, sg.y1, 0.0, 0.0, -1.0, 0, 0});
                vpos.push_back(PairD{sg.x1, sg.y1});
            }
            vtx.push_back(edge(sg));
            seg64.push_back(SegD{sg.x1, sg.y1, sg.x1 - sg.x2, sg.y1 - sg.y2, -1.0, 0, 0});
            vpos.push_back(PairD{sg.x2, sg.y2});
            wall_k[w] = (int)vtx.size() - 1 - h.vtx_off;
        }
        h.n_chain = (int)vtx.size() - h.vtx_off;
        while ((vtx.size() - h.vtx_off) % 4) {  // the sweep walks vertex groups of four: pad with chain-start sentinels
            vtx.push_back(Vtx{vtx.back().xr, vtx.back().yr, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f});
            seg64.push_back(SegD{seg64.back().x1, seg64.back().y1, 0.0, 0.0, -1.0, 0, 0});
            vpos.push_back(vpos.back());
        }
        h.nV = (int)vtx.size() - h.vtx_off;
        return wall_k;
    }

    // F32 mode: the selector's "nothing selected" pattern (SEL_INIT) carries vertex index 0 only while the index takes at
    // most 13 of the candidate's mantissa bits; the float32 coordinates (relative to the track's anchor) and the flag
    // thresholds are priced for a track that fits 2000 px.  F64 mode has neither limit.
    int limits(int k, const TrackHdr& h) {
        if (h.nV > 65535 || (!f64 && h.nV > 8192)) {
            err = "track " + std::to_string(k) + ": " + std::to_string(h.nV) + " chain vertices; dtype f32 takes at most 8192 (use dtype f64)";
            return PC_ERR_UNSUPPORTED;
        }
        if (!f64 && (h.bx1 - h.bx0 > 2000.0f || h.by1 - h.by0 > 2000.0f)) {
            err = "track " + std::to_string(k) + ": the walls' bounding box exceeds 2000 px; dtype f32 is priced for tracks that fit (use dtype f64)";
            return PC_ERR_UNSUPPORTED;
        }
        return PC_OK;
    }
    // F64 handles: the float32 SELECTOR (the persistent kernel's literal form, env_step_fast<..., LIT>) runs on a track within
    // those same limits; any other track takes the filter form (env_step_core<double>), which has none.
    bool selector_fits(const TrackHdr& h) const { return !f64 || (h.nV <= 8192 && h.bx1 - h.bx0 <= 2000.0f && h.by1 - h.by0 <= 2000.0f); }
    // low bits of a sweep candidate that carry the vertex index (at least 5: the unrolled 28-vertex sweep's constant)
    static int index_bits(int nV) {
        int b = 5;
        while ((1 << b) < nV) ++b;
        return b;
    }

    // exactly two chains?  (what the kernels compiled for big_track's layout rely on: TrackHdr::brk2)
    void two_chain_packing(TrackHdr& h) {
        const int o = h.vtx_off;
        int n_starts = 0, second = -1;
        for (int k = 0; k < h.n_chain; ++k)
            if (is_start(h, k) && ++n_starts == 2) second = k;
        h.brk2 = n_starts == 2 ? second : -1;
        h.vtxp_off = -1;
        if (h.brk2 > 0 && h.n_chain == 2 * h.brk2) {     // ... of the same length: the packed copy (VtxP)
            h.vtxp_off = (int)out.vtxp.size();
            for (int i = 0; i < h.brk2; ++i) {
                const Vtx &a = out.vtx[o + i], &b = out.vtx[o + h.brk2 + i];
                out.vtxp.push_back(VtxP{{a.xr, b.xr}, {a.yr, b.yr}, {a.ex, b.ex}, {a.ey, b.ey}, {a.exs, b.exs}, {a.eys, b.eys}});
            }
        }
    }

    // chain neighbours and end margins of every segment (SegD::h, SegD::prev_next), and the segments float32 cannot order (PC_SEG_SCAN).
    // What float32 can get wrong is the ORDER of two hits that lie within its resolution of each other.  The selector
    // keeps 23 - b mantissa bits of a candidate (b index bits): two hits closer than sel_res = 1001 px * 2^-(23 - b) along
    // a ray (beyond 1000 px the reported distance is 1000 either way) may be taken in the wrong order.
    //   * Two walls that share a vertex V at an angle of at least ~13 degrees: such hits lie within sel_res / sin(13 deg) of
    //     V, so a refined hit within `margin` = max(0.05 px, 4.6 sel_res) of a segment's end is compared with the chain
    //     neighbours under the strict test (SegD::h; refine_careful).
    //   * Anything else that brings two walls within `near` = max(0.05 px, 1.5 sel_res) of each other -- walls that cross
    //     or touch without being chain neighbours (a T-junction, an X), a spike sharper than 13 degrees, a wall shorter than
    //     2 margin (its neighbours' neighbours are that close) -- cannot be settled by looking at two neighbours: those
    //     segments carry PC_SEG_SCAN and every ray whose selection lands on one of them is resolved by the float64 scan of
    //     the whole chain under the reference's strict test (car_env.py:178), i.e. exactly.
    void neighbours_margins_scan(TrackHdr& h, const std::vector<int>& wall_k, bool sel, int idx_bits) {
        std::vector<Seg>& segs = out.segs;
        std::vector<SegD>& seg64 = out.seg64;
        const int n = h.nV, o = h.vtx_off;
        const double sel_res = 1001.0 * std::ldexp(1.0, -(23 - idx_bits));
        const double margin = std::max(0.05, 4.6 * sel_res), near = std::max(0.05, 1.5 * sel_res);
        // (where the selector runs: nV <= 8192 there, so prev / next fit their 15 bits beside PC_SEG_SCAN; the F64 filter form never reads seg64)
        for (int k = 0; k < n && sel; ++k) {
            if (is_start(h, k)) continue;     // chain starts / padding: no segment (h = -1: |t - 0.5| < h never holds)
            int c0 = k;     // first vertex of this chain, and its last
            while (!is_start(h, c0)) --c0;
            int c1 = k;
            while (c1 + 1 < h.n_chain && !is_start(h, c1 + 1)) ++c1;
            const bool closed = c1 > c0 && vpos[o + c0].x == vpos[o + c1].x && vpos[o + c0].y == vpos[o + c1].y;
            const int prev = k - 1 > c0 ? k - 1 : (closed && c1 != k ? c1 : 0);       // shares this segment's first endpoint
            const int next = k + 1 <= c1 ? k + 1 : (closed && c0 + 1 != k ? c0 + 1 : 0);   // shares its second endpoint
            static_assert(PC_SEG_SCAN == 0x8000, "prev in bits 0..14, PC_SEG_SCAN in bit 15, next in bits 16..30");
            seg64[o + k].prev_next = prev | (next << 16);      // (prev, next < nV <= 8192)
            const double len = std::hypot(seg64[o + k].ex, seg64[o + k].ey);
            seg64[o + k].h = 0.5 - margin / len;
            if (len < 2.0 * margin) seg64[o + k].prev_next |= PC_SEG_SCAN;
        }
        if (!sel) return;
        const auto seg_of = [&](int w) { return segs[h.wall_off + w]; };
        const auto pt_seg = [](double px, double py, const Seg& s) {     // distance of a point from a segment
            const double ex = s.x2 - s.x1, ey = s.y2 - s.y1, l2 = ex * ex + ey * ey;
            double t = l2 > 0.0 ? ((px - s.x1) * ex + (py - s.y1) * ey) / l2 : 0.0;
            t = std::min(1.0, std::max(0.0, t));
            return std::hypot(px - (s.x1 + t * ex), py - (s.y1 + t * ey));
        };
        const auto orient = [](const Seg& s, double px, double py) { return (s.x2 - s.x1) * (py - s.y1) - (s.y2 - s.y1) * (px - s.x1); };
        for (int a = 0; a < h.S; ++a) {
            const Seg sa = seg_of(a);
            const int ka = wall_k[a];
            if (is_start(h, ka)) continue;     // (a wall without length is a chain start: never hit)
            const int pa = seg64[o + ka].prev_next & 0x7fff, na = (int)(((unsigned)seg64[o + ka].prev_next >> 16) & 0x7fff);
            for (int b = a + 1; b < h.S; ++b) {
                const Seg sb = seg_of(b);
                const int kb = wall_k[b];
                if (is_start(h, kb)) continue;
                bool bad;
                if (pa == kb || na == kb) {
                    // chain neighbours: a spike sharper than ~13 degrees (|sin| < 0.22 with the walls folding back on each other)
                    const double ax = sa.x2 - sa.x1, ay = sa.y2 - sa.y1, bx = sb.x2 - sb.x1, by = sb.y2 - sb.y1;
                    const double la = std::hypot(ax, ay), lb = std::hypot(bx, by);
                    const double sn = std::fabs(ax * by - ay * bx) / (la * lb), cs = (ax * bx + ay * by) / (la * lb);
                    // consecutive walls run head to tail: folding back = their directions nearly opposite
                    bad = sn < 0.22 && cs < 0.0;
                } else {
                    const double o1 = orient(sa, sb.x1, sb.y1), o2 = orient(sa, sb.x2, sb.y2), o3 = orient(sb, sa.x1, sa.y1), o4 = orient(sb, sa.x2, sa.y2);
                    const bool cross = ((o1 > 0) != (o2 > 0)) && ((o3 > 0) != (o4 > 0));
                    const double d = cross ? 0.0 : std::min({pt_seg(sa.x1, sa.y1, sb), pt_seg(sa.x2, sa.y2, sb), pt_seg(sb.x1, sb.y1, sa), pt_seg(sb.x2, sb.y2, sa)});
                    bad = d < near;
                }
                if (bad) {
                    seg64[o + ka].prev_next |= PC_SEG_SCAN;
                    seg64[o + kb].prev_next |= PC_SEG_SCAN;
                }
            }
        }
        for (int k = 0; k < n; ++k)
            if (seg64[o + k].prev_next & PC_SEG_SCAN) { seg64[o + k].h = -1.0; ++h.n_scan; }
    }

    // F64 handles: the literal arithmetic wants the wall's SECOND ENDPOINT as the track file gives it (x1 - ex need not be
    // x2 to the last bit): the records' (ex, ey) fields carry (x2, y2) from here on (lit_fast); a chain start or padding
    // record gets x2 = x1: den == 0, never a hit
    void second_endpoints(TrackHdr& h) {
        const int o = h.vtx_off;
        for (int k = 0; k < h.nV; ++k) {
            SegD& r = out.seg64[o + k];
            const bool start = is_start(h, k);
            r.ex = start ? r.x1 : vpos[o + k].x;
            r.ey = start ? r.y1 : vpos[o + k].y;
        }
    }

    // F64 mode: every rotation an episode can reach (see Math<double>), breadth first over +-5.0 turns, into `rots`; and the rotation
    // table (Math<double>): row i = the R rays' (cos, sin) at rotation i, then (index of rot - 5.0, index of rot + 5.0), then (rot, -)
    void rotation_table(int k, const pc_track* t, TrackHdr& h, std::unordered_set<uint64_t>& rots) {
        std::unordered_set<uint64_t> frontier;
        std::vector<uint64_t> rot_list;                       // index -> rotation (breadth first; index 0 = start_rot: what reset gives)
        std::unordered_map<uint64_t, int>& rid = out.rot_ids[k];
        rid.clear();
        std::vector<int>& depth = out.rot_depth[k];
        int cur_depth = 0;
        const auto add_rot = [&](uint64_t b) {
            if (!rots.insert(b).second) return false;
            rid[b] = (int)rot_list.size();
            rot_list.push_back(b);
            depth.push_back(cur_depth);
            return true;
        };
        add_rot(bits(t->start_rot));
        frontier = rots;
        for (int turn = 0; turn < 1000 && !frontier.empty(); ++turn) {      // CarEnv truncates at 1000 steps (car_env.py:749)
            cur_depth = turn + 1;
            std::unordered_set<uint64_t> next;
            for (const uint64_t b : frontier)
                for (const double w : {val(b) + 5.0, val(b) - 5.0})            // :440-442
                    if (add_rot(bits(w))) next.insert(bits(w));
            frontier.swap(next);
        }
        std::vector<PairD>& dirtab64 = out.dirtab64;
        h.rot_off = (int)dirtab64.size();
        h.n_rot = (int)rot_list.size();
        for (const uint64_t b : rot_list) {
            for (int ray = 0; ray < R; ++ray) {
                const double a = (val(b) + (double)(ray * step_deg)) * (PC_PI / 180.0);   // np.radians(rot + a), :269, :465
                dirtab64.push_back(PairD{libm_cos(a), libm_sin(a)});
            }
            const auto lk = rid.find(bits(val(b) - 5.0)), rk = rid.find(bits(val(b) + 5.0));
            dirtab64.push_back(PairD{lk == rid.end() ? -1.0 : (double)lk->second, rk == rid.end() ? -1.0 : (double)rk->second});
            dirtab64.push_back(PairD{val(b), 0.0});
        }
    }

    // F64 mode: every angle an episode can reach -- a rotation of `rots` plus a ray's offset --, glibc's cos / sin of it, hashed by the
    // angle's bits
    void angle_hash(TrackHdr& h, const std::unordered_set<uint64_t>& rots) {
        std::unordered_set<uint64_t> keys;
        for (const uint64_t b : rots)
            for (int ray = 0; ray < R; ++ray) keys.insert(bits(val(b) + (double)(ray * step_deg)));   // :269, :465
        size_t cap = 1024;
        while (cap < 4 * keys.size()) cap <<= 1;
        std::vector<F64Dir> tab;
        for (;; cap <<= 1) {            // (grown until no probe sequence is longer than the device follows)
            tab.assign(cap, F64Dir{F64DIR_EMPTY, 0.0, 0.0, 0});
            bool ok = true;
            for (const uint64_t k : keys) {
                size_t slot = f64dir_hash(k) & (cap - 1);
                int probe = 0;
                while (tab[slot].key != F64DIR_EMPTY && probe < F64DIR_MAX_PROBE) { slot = (slot + 1) & (cap - 1); ++probe; }
                if (probe == F64DIR_MAX_PROBE) { ok = false; break; }
                const double a = val(k) * (PC_PI / 180.0);   // np.radians
                tab[slot] = F64Dir{k, libm_cos(a), libm_sin(a), 0};
            }
            if (ok) break;
        }
        h.dir_off = (int)out.dirhash.size();
        h.head_off = (int)(cap - 1);
        out.dirhash.insert(out.dirhash.end(), tab.begin(), tab.end());
    }

    // direction lattice [361]: start_rot + j degrees, np.radians then libm cos/sin; entry 360 = (0, 0): no ray.  F32 handles keep it in
    // float32 (the selector's) and in float64 (the refinement's).  F64 handles keep the float32 one alone: every angle rot + a is one
    // of them mod 360, and the float32 direction only selects, so that cos of the unreduced angle differs in float64's last places
    // does not matter
    void direction_lattice(const pc_track* t, bool with_f64) {
        for (int j = 0; j < 360; ++j) {
            const double a = (t->start_rot + (double)j) * (PC_PI / 180.0);
            const double c = libm_cos(a), s = libm_sin(a);
            out.dirtab.push_back(PairF{(float)c, (float)s});
            if (with_f64) out.dirtab64.push_back(PairD{c, s});
        }
        out.dirtab.push_back(PairF{0.f, 0.f});
        if (with_f64) out.dirtab64.push_back(PairD{0.0, 0.0});
    }

    // heading grid [72]: start_rot + 5 j degrees, np.radians then libm cos/sin
    void heading_grid(const pc_track* t) {
        for (int j = 0; j < 72; ++j) {
            const double a = (t->start_rot + 5.0 * j) * (PC_PI / 180.0);
            out.headtab.push_back(PairD{libm_cos(a), libm_sin(a)});
        }
    }

    int track(int k, const pc_track* t) {
        TrackHdr& h = out.hdr[k];
        h.S = t->n_walls();
        h.G = t->n_gates();
        h.n_scan = 0;
        h.rot_off = -1;     // (F64 handles: set below)
        h.n_rot = 0;
        h.lat_off = -1;
        h.sel_ok = 1;
        const std::vector<int> wall_k = chains_and_anchor(t, h);
        if (const int rc = limits(k, h)) return rc;
        const bool sel = selector_fits(h);      // the float32 selector runs on this track
        const int idx_bits = index_bits(h.nV);
        h.sel_ok = sel ? 1 : 0;
        h.idx_mask = (1u << idx_bits) - 1u;
        two_chain_packing(h);
        neighbours_margins_scan(h, wall_k, sel, idx_bits);
        if (f64 && sel) second_endpoints(h);
        if (f64) {
            h.dir_off = -1;
            h.head_off = 0;
            if (n_tracks <= 16) {
                std::unordered_set<uint64_t> rots;
                rotation_table(k, t, h, rots);
                angle_hash(h, rots);
            }
            if (out.dirtab64.empty()) out.dirtab64.push_back(PairD{0.0, 0.0});
            h.lat_off = (int)out.dirtab.size();
        } else {
            h.dir_off = (int)out.dirtab.size();
            h.lat_off = h.dir_off;
        }
        direction_lattice(t, !f64);
        // the float32 1/den table [361][nV] exists only where a kernel can stage it in LDS: chains of at most FT_VTX_MAX vertices, and on F64
        // handles only for tracks the selector may run on (a 65535-vertex float64 track would cost 95 MB it can never read)
        const bool want_rden = h.nV <= FT_VTX_MAX && (!f64 || h.sel_ok);
        if (out.rden_floats + (size_t)361 * h.nV > (size_t)INT_MAX) {
            err = "pc_env_create: the tracks' 1/den tables exceed 2^31 floats";
            return PC_ERR_UNSUPPORTED;
        }
        h.rden_off = want_rden ? (int)out.rden_floats : -1;
        if (want_rden) out.rden_floats += (size_t)361 * h.nV;
        if (!f64) h.head_off = (int)out.headtab.size();
        h.start_collides = 0;
        h.start_x = t->start_x;
        h.start_y = t->start_y;
        h.start_rot = t->start_rot;
        heading_grid(t);
        return PC_OK;
    }

    void facts() {
        TrackFacts& tf = out.facts;
        for (const TrackHdr& h : out.hdr) {
            tf.max_G = std::max(tf.max_G, h.G);
            tf.max_nV = std::max(tf.max_nV, h.nV);
            tf.sum_nV += h.nV;
            tf.tabs = tf.tabs && h.lat_off >= 0 && (!f64 || (h.sel_ok && h.rot_off >= 0));
            tf.rden = tf.rden && h.rden_off >= 0;
            tf.sel = tf.sel && h.sel_ok;
            tf.nv28 = tf.nv28 && h.nV == 28 && h.n_chain == 26 && h.brk2 == 13 && h.vtxp_off >= 0;
            tf.loops = tf.loops && h.vtxp_off >= 0 && (h.brk2 == 13 || h.brk2 == 9) && h.n_chain == 2 * h.brk2 && h.nV == 4 * ((h.brk2 + 1) / 2);
        }
    }
};

}  // namespace

int pc_internal_compile_tracks(const pc_track* const* tracks, int n_tracks, int n_nominal, int R, int dtype, TrackTables& out, std::string& err) {
    out = TrackTables{};
    out.hdr.resize(n_tracks);
    out.rot_ids.assign(n_tracks, {});
    out.rot_depth.assign(n_tracks, {});
    Compiler c{n_tracks, n_nominal, R, dtype == PC_DTYPE_F64, out, err};
    for (int k = 0; k < n_tracks; ++k)
        if (const int rc = c.track(k, tracks[k])) return rc;
    c.facts();
    return PC_OK;
}

TrackLayout pc_internal_classify_track_ids(const uint8_t* track_id, int64_t n_envs, int n_tracks) {
    const size_t N = (size_t)n_envs;
    TrackLayout l;
    for (int blk = 256; blk >= 32 && !l.track_block; blk >>= 1) {
        bool ok = true;
        for (size_t i = 0; i < N && ok; ++i) ok = track_id[i] == track_id[i & ~(size_t)(blk - 1)];
        if (ok) l.track_block = blk;
    }
    l.blocks32 = l.track_block >= 32;
    for (int blk = 64; blk >= 32; blk >>= 1) {
        bool ok = n_tracks == 2 && N % blk == 0;
        for (size_t b = 0; b < N && ok; b += blk) {
            int ones = 0;
            for (int i = 0; i < blk; ++i) ones += track_id[b + i] == 1, ok = ok && track_id[b + i] < 2;
            ok = ok && ones == blk / 2;
        }
        (blk == 64 ? l.bal64 : l.bal32) = ok;
    }
    return l;
}
