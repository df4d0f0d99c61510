// track_records.hpp -- the records of the track tables, as the host compiles them (track_tables.cpp) and the kernels read them
// (kernels/env_math.hpp).  Includes nothing from HIP: any C++ compiler takes it, so the table compiler builds and is tested without a GPU.
#pragma once

#ifdef __HIPCC__
#define PC_HOST_DEVICE __host__ __device__
#else
#define PC_HOST_DEVICE
#endif

#define PC_PI 3.141592653589793238462643383279502884 /* NPY_PI: np.radians = x * (PI / 180), on the host as in the kernels */

// ------------------------------------------------------------------------------------------
// device-side data
// ------------------------------------------------------------------------------------------
struct TrackHdr {        // one per track, read with scalar loads
    int wall_off, S;     // segs[wall_off .. wall_off+S): the walls
    int gate_off, G;     // segs[gate_off .. gate_off+G): the reward gates
    int head_off;        // F32: heading table [72] (cos, sin) of radians(start_rot + 5 j)
    int start_collides;  // Car.update at reset already hits a wall (car_env.py:686,468-469)
    int vtx_off, nV;     // F32: the walls again as vertex chains, vtx[vtx_off .. vtx_off+nV); nV is padded to a multiple of 4
    int dir_off;         // F32: ray direction table [361] of this track in dirtab / dirtab64 (entry 360 = (0, 0): no ray)
                         // F64: first slot of the track's angle -> (cos, sin) hash table in dirhash (Math<double>; head_off = its slot
                         //      mask), -1 = none
    int rden_off;        // F32: 1/den table [361][nV] of this track in rden (row 360 = +inf: never hits)
    int n_chain;         // F32: chain vertices before the padding to a multiple of 4 (vtx[n_chain .. nV) are sentinels)
    unsigned idx_mask;   // F32: (1 << b) - 1, b = max(5, ceil(log2(nV))): the low bits of a sweep candidate carry its vertex index
    double start_x, start_y, start_rot;
    double ax0, ay0;            // F32: the anchor of the sweep's float32 coordinates: the centre of the wall vertices' bounding box
    float bx0, bx1, by0, by1;   // F32: that bounding box (the sweep's flag threshold is priced from it)
    int n_scan;                 // F32: how many segments carry PC_SEG_SCAN (diagnostic)
    int brk2;                   // F32: index of the chain's SECOND chain-start vertex when the walls are exactly two chains (-1 otherwise)
    int vtxp_off;               // F32: those two chains have the same length (n_chain = 2 brk2): their vertices again, packed by
                                //      position in the chain, vtxp[vtxp_off .. vtxp_off + brk2) (-1 otherwise)
    int rot_off, n_rot;         // F64: the track's ROTATION TABLE in dirtab64 (Math<double>): n_rot rows of R + 1 entries; -1 = none
    int lat_off;                // the track's float32 direction lattice [361] in dirtab (F32: = dir_off; F64: the selector's directions, -1 = none)
    int sel_ok;                 // F64: the float32 selector may run on this track (chain tables built, <= 8192 vertices, fits 2000 px)
};

// One wall / gate segment as the reference holds it (Boundary.get_points, car_env.py:74): 32 bytes.
struct Seg { double x1, y1, x2, y2; };

// F32 wall sweep: the walls as chains of vertices, (xr, yr) = the vertex relative to the track's anchor (TrackHdr::ax0, ay0: the
// centre of its bounding box), rounded from float64 -- the sweep only SELECTS, so it can afford float32 coordinates as long as
// the flag threshold prices their rounding (flag_threshold).  Vertex k closes the segment (k-1, k) unless it
// starts a new chain: then its edge (ex, ey) is (0, 0) (a real wall has length).  (ex, ey) = the UNIT vector along p[k-1] - p[k]
// rounded from float64 -- the selector's u = cross(e, a) / cross(e, dir) does not depend on the edge's length, and with a unit
// edge cross(e, a) is the car's distance from the wall line in pixels, which makes its rounding threshold one number per car --,
// (exs, eys) the same scaled by 2^-40 (exact): the sweep's selector values live in that scaled domain (see wall_sweep_f32).
// 32 bytes = one s_load_dwordx8.
// Why chains: the reference's hit test 0 < t < 1 (car_env.py:178) is "the two endpoints lie strictly on
// opposite sides of the ray line".  Evaluated per VERTEX -- one cross product c_k = cross(p_k - pos, dir)
// shared by the two segments that meet there -- a float32 ray cannot slip between two adjacent walls
// through the rounding-wide crack that two independently rounded t's leave at their common corner.
struct Vtx { float xr, yr, ex, ey, exs, eys, pad0, pad1; };
#ifdef __clang__
typedef float f32x2 __attribute__((ext_vector_type(2)));
#else
typedef float f32x2 __attribute__((vector_size(8)));      // (a host compiler without clang's vector types: same size and alignment)
#endif
// Walls that are exactly two chains of the same length L (big_track.json: the outer and the inner loop, 13 vertices each):
// record i holds vertex i of BOTH chains -- component 0 = chain vertex i, component 1 = chain vertex L + i -- so that the
// sweep's packed-fp32 instructions advance both chains at once (wall_sweep_loops).  Same values as the two Vtx records.
struct VtxP { f32x2 xr, yr, ex, ey, exs, eys; };   // 48 bytes
// The float64 refinement's view of the same chain, one 48-byte record per vertex k = the segment that vertex closes:
// (x1, y1) -> (x1 - ex, y1 - ey) with (ex, ey) = p[k-1] - p[k] formed in float64 as the reference forms (x1 - x2), (y1 - y2)
// (car_env.py:171); h = 0.5 - (0.05 px) / |e|: a refined hit whose parameter t satisfies |t - 0.5| < h lies at least 0.05 px
// inside the segment's ends (-1 for chain starts / padding, which have a zero edge: no segment); prev / next = the chain
// neighbours of the segment -- prev shares its first endpoint, next its second (0: none; a closed loop wraps).
struct SegD { double x1, y1, ex, ey, h; int prev_next, pad; };   // prev in bits 0..14, PC_SEG_SCAN, next in bits 16..30
// PC_SEG_SCAN: this wall comes closer to another one than float32 can order hits, without the two being plain chain neighbours
// (walls that cross or touch -- a T-junction, an X --, a spike sharper than ~13 degrees, a wall shorter than the end margin;
// found on the host at pc_env_create): h = -1, and a ray whose selection lands here is resolved by the float64 scan of the chain
constexpr int PC_SEG_SCAN = 0x8000;

// The table-driven kernels stage a track's chain in LDS (rollout.hpp's region offsets): at most this many vertices.  The host
// builds the 1/den table only for such tracks.
constexpr int FT_VTX_MAX = 64;

// F64 mode's directions.  The reference forms np.cos / np.sin of np.radians(angle) (car_env.py:426-427, :463-466, :584) for
// angle = rotation [+ a], rotation = the start rotation after a sequence of +-5.0 (each sum rounded: :440-442), a = the ray's
// whole-degree offset (:269).  Inside an episode (at most 1000 turns) only a few thousand distinct float64 rotations can occur
// -- the roundings merge the paths -- and ~15 k distinct angles: the host enumerates them, evaluates cos / sin with glibc (the
// reference's own libm) and the device LOOKS THEM UP by the angle's bit pattern: the reference's bits by construction, where the
// device's own cos / sin (ocml) differ from glibc in the last place for some arguments.  An angle that is not in the table
// (set_state with a rotation no episode reaches; more than 16 tracks: dir_off < 0) is evaluated on the device as before.
struct F64Dir { unsigned long long key; double c, s; unsigned long long pad; };     // 32 bytes; key = the angle's bits (degrees)
constexpr unsigned long long F64DIR_EMPTY = 0x7ff8dead00000000ull;                  // (a NaN pattern no sum produces)
constexpr int F64DIR_MAX_PROBE = 8;                                                 // the host sizes the table so that this holds
PC_HOST_DEVICE inline unsigned f64dir_hash(unsigned long long k) {
    k ^= k >> 29;
    k *= 0xBF58476D1CE4E5B9ull;
    return (unsigned)(k >> 32);
}

static_assert(sizeof(Seg) == 32 && sizeof(Vtx) == 32, "segment / vertex records are 32 bytes (one s_load_dwordx8)");
static_assert(sizeof(VtxP) == 48, "packed vertex records: 48 bytes");
static_assert(sizeof(SegD) == 48, "refinement table: 48 bytes per chain vertex");
static_assert(sizeof(F64Dir) == 32, "angle hash table: 32 bytes per slot");
