// render.hpp -- part of the single translation unit ppocar.hip (included there after track_maps.hpp; not a stand-alone header).
// K18 render_background_kernel / K19 render_frames_kernel: observation rows turned into RGB frames (pc_render_background,
// pc_render_frames).  The drawing rule is exact integer arithmetic in quarter pixels (q), so that
// tests/render_reference.py (numpy int64) and these kernels agree on every pixel.
//
// The integer bounds.  Frames are W = 1280 / scale by H = 720 / scale; the centre of pixel (i, j) is
// P = (4 scale i + 2 scale, 4 scale j + 2 scale), so 0 < P.x < 5120 and 0 < P.y < 2880.
//   static geometry  a track is accepted only with every wall / gate coordinate inside [-1024, 2304] x [-1024, 1744] px, i.e.
//                    [-4096, 9216] x [-4096, 6976] q: |B - A| <= 13312 and |P - A| <= 9216 per axis.
//   dynamic          a frame draws its car only with the car inside the same box and |cos|, |sin| <= 1 (the guards of render_frames_kernel).
//                    A ray is at most 1000 px long in a direction (c ci - s si, s ci + c si) of at most sqrt(2) per axis: its end is
//                    within 1415 px of the car, inside [-2439, 3719] px = [-9756, 14876] q: |B - A| <= 5660, |P - A| <= 14876; the
//                    car's capsule ends lie within 14 px of the car.
// So every difference is below 2^14 = 16384 in magnitude; a dot or cross product is a sum of two products below 2^28 each: below
// 2^29 < 2^30, it fits int32, as do L = |B - A|^2 and |P - A|^2.  A squared cross product is below 2^58 and h^2 L below
// 900 * 2^29 < 2^39 (the widest half-width is max(24, 3 * 10) = 30 q): both fit int64.  (The lanes of a partial tile that lie outside the
// frame compute with P up to 6144 q, |P - A| <= 15900: still below 2^14; they store nothing.)
#pragma once

#define PC_RENDER_TILE_W 64      // pixels: 16 lanes x 4 pixels
#define PC_RENDER_LANE_ROWS 4    // rows per lane, 16 apart: a wave still writes 4 consecutive rows per store
#define PC_RENDER_TILE_H 64      // rows: 256 threads / 16 lanes x PC_RENDER_LANE_ROWS
#define PC_RENDER_CHUNK 256      // primitives binned per pass: one per thread, so a pass's list always fits

struct RenderTrack { int wall_off, n_walls, gate_off, n_gates; };
struct RenderPalette { uint32_t rgb[PC_RENDER_COLORS]; };      // r | g << 8 | b << 16

// primitive kinds of K19's list, as bits of a pixel's coverage mask: a higher bit is a later layer
#define PC_RENDER_BIT_NEXT 1
#define PC_RENDER_BIT_RAY 2
#define PC_RENDER_BIT_HIT 4
#define PC_RENDER_BIT_CAR 8

// Q(v): a float64 pixel coordinate to quarter pixels (one exact product, round to nearest even)
__host__ __device__ inline int render_q(const double v) { return (int)rint(v * 4.0); }

// Does the segment (A, A + e) of squared length L = |e|^2 and squared half-width h2 cover the point A + w?  u = w . e, cr = w x e.
__device__ inline bool render_covers(const int wx, const int wy, const int ex, const int ey, const int L, const int h2, const int u, const int cr) {
    if (L == 0 || u <= 0) return wx * wx + wy * wy <= h2;
    if (u >= L) {
        const int vx = wx - ex, vy = wy - ey;
        return vx * vx + vy * vy <= h2;
    }
    return (long long)cr * (long long)cr <= (long long)h2 * (long long)L;
}

// ------------------------------------------------------------------------------------------
// K18: the static layers of every track, one thread per pixel, every wall and gate of the pixel's track tested (once per handle and
// scale).  bg [n_tracks][2][H][W] uint8: plane 0 = PC_RENDER_GRASS / _ROAD / _WALL, plane 1 = 1 + the highest gate that covers the
// pixel (0: none) -- gates are kept OUT of plane 0, so K19 can hide the gates a car has passed by comparing plane 1 with next_gate.
// Road: even-odd over all walls.  A wall counts when it straddles the pixel's row, (A.y > P.y) != (B.y > P.y), and crosses it
// strictly to the right of P: with w = P - A, e = B - A that is cross = w.x e.y - w.y e.x < 0 for e.y > 0 and > 0 for e.y < 0.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void render_background_kernel(const int4* __restrict__ walls, const int4* __restrict__ gates,
                                                                const RenderTrack* __restrict__ trk, const int n_tracks, const int scale,
                                                                const int W, const int H, const int h_wall, const int h_gate,
                                                                uint8_t* __restrict__ bg) {
    const int64_t HW = (int64_t)H * W;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= HW * n_tracks) return;
    const int k = (int)(idx / HW);
    const int rem = (int)(idx - (int64_t)k * HW);
    const int j = rem / W, i = rem - j * W;
    const int Px = 4 * scale * i + 2 * scale, Py = 4 * scale * j + 2 * scale;
    const RenderTrack t = trk[k];
    int crossings = 0;
    bool wall = false;
    for (int s = 0; s < t.n_walls; ++s) {
        const int4 a = walls[t.wall_off + s];
        const int ex = a.z - a.x, ey = a.w - a.y, wx = Px - a.x, wy = Py - a.y;
        const int cr = wx * ey - wy * ex;
        if ((a.y > Py) != (a.w > Py)) crossings += (ey > 0 ? cr < 0 : cr > 0) ? 1 : 0;
        wall = wall || render_covers(wx, wy, ex, ey, ex * ex + ey * ey, h_wall * h_wall, wx * ex + wy * ey, cr);
    }
    int gate = 0;
    for (int g = 0; g < t.n_gates; ++g) {
        const int4 a = gates[t.gate_off + g];
        const int ex = a.z - a.x, ey = a.w - a.y, wx = Px - a.x, wy = Py - a.y;
        if (render_covers(wx, wy, ex, ey, ex * ex + ey * ey, h_gate * h_gate, wx * ex + wy * ey, wx * ey - wy * ex)) gate = g + 1;
    }
    bg[(int64_t)k * 2 * HW + rem] = (uint8_t)(wall ? PC_RENDER_WALL : ((crossings & 1) ? PC_RENDER_ROAD : PC_RENDER_GRASS));
    bg[(int64_t)k * 2 * HW + HW + rem] = (uint8_t)gate;
}

// ------------------------------------------------------------------------------------------
// K19: one workgroup per (frame, tile of 64 x 64 pixels); a lane owns 4 horizontally adjacent pixels in each of 4 rows 16 apart and
// writes each row's 12 bytes as three dword stores (16 lanes = 192 contiguous bytes per row; every scale's W is a multiple of 4, so a
// lane's pixels of a row are all inside the frame or all outside).  The static layers' dwords are loaded first, so that their latency
// hides behind the binning.  The frame's dynamic primitives -- R rays, R hit discs, the car's capsule, the highlighted gate
// -- are binned against the tile's box PC_RENDER_CHUNK at a time, one per thread, compacted into an LDS list with a ballot per
// wave; every pixel then tests only that list (cross and dot are affine in P: two integer adds per further pixel of the lane) and
// keeps a mask of the layers that cover it.  360 nominal rays are 722 primitives: three passes.  The static layers come from K18's
// image (a few hundred KB: L2-resident), the palette from the launch's arguments through LDS.
// A row that fails a guard (position or heading not finite, |cos| or |sin| above 1, the car outside [-1024, 2304] x [-1024, 1744] px,
// a track id the handle does not have -- which shows track 0) draws the static layers only, every gate plain.
// ------------------------------------------------------------------------------------------
struct RenderFrames {
    const float* obs;
    int64_t obs_ld;
    const int32_t* next_gate;
    const uint8_t* track_id;
    int64_t m0;                      // the launch's first frame
    int scale, W, H, tiles_x, tiles_y, R, n_tracks;
    int h2_ray, h2_hit, h2_car, h2_gate, h_max;
    const double2* dirs;             // [R] cos / sin of radians(i * step), the host's
    const int4* gates;
    const RenderTrack* trk;
    const uint8_t* bg;
    uint8_t* frames;
    RenderPalette pal;
};

__global__ __launch_bounds__(256) void render_frames_kernel(const RenderFrames a) {
    __shared__ int4 seg[PC_RENDER_CHUNK];      // A.x, A.y, e.x, e.y
    __shared__ int4 aux[PC_RENDER_CHUNK];      // L, h2, layer bit
    __shared__ int count;
    __shared__ uint32_t pal[PC_RENDER_COLORS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int tiles = a.tiles_x * a.tiles_y;
    const int64_t m = a.m0 + blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int i0 = tx * PC_RENDER_TILE_W + (tid & 15) * 4, j0 = ty * PC_RENDER_TILE_H + (tid >> 4);      // the lane's rows: j0 + 16 r
    const int sq = 4 * a.scale, half = 2 * a.scale;
    const int Px = sq * i0 + half, Py = sq * j0 + half;
    // the tile's pixel centres (a partial tile keeps the whole tile's box: a longer list, the same pixels)
    const int bx0 = sq * tx * PC_RENDER_TILE_W + half, bx1 = bx0 + sq * (PC_RENDER_TILE_W - 1);
    const int by0 = sq * ty * PC_RENDER_TILE_H + half, by1 = by0 + sq * (PC_RENDER_TILE_H - 1);
#pragma unroll
    for (int k = 0; k < PC_RENDER_COLORS; ++k)
        if (tid == k) pal[k] = a.pal.rgb[k];

    const float* const o = a.obs + m * a.obs_ld;
    const float o0 = o[0], o1 = o[1], o4 = o[4], o5 = o[5];
    int trk = a.track_id ? (int)a.track_id[m] : 0;
    const double x = (double)o0 * 1280.0, y = (double)o1 * 720.0, c = (double)o4, s = (double)o5;
    const bool dyn = trk < a.n_tracks && isfinite(o0) && isfinite(o1) && isfinite(o4) && isfinite(o5) && fabs(c) <= 1.0 && fabs(s) <= 1.0 &&
                     x >= -1024.0 && x <= 2304.0 && y >= -1024.0 && y <= 1744.0;
    if (trk >= a.n_tracks) trk = 0;
    const RenderTrack t = a.trk[trk];
    const int64_t HW = (int64_t)a.H * a.W;
    uint32_t layer4[PC_RENDER_LANE_ROWS], gate4[PC_RENDER_LANE_ROWS];
#pragma unroll
    for (int r = 0; r < PC_RENDER_LANE_ROWS; ++r) {
        const int j = j0 + 16 * r;
        layer4[r] = gate4[r] = 0u;
        if (i0 < a.W && j < a.H) {
            const uint8_t* const plane = a.bg + (int64_t)trk * 2 * HW + (int64_t)j * a.W + i0;
            layer4[r] = *(const uint32_t*)plane;
            gate4[r] = *(const uint32_t*)(plane + HW);
        }
    }
    const int ng = (dyn && a.next_gate) ? a.next_gate[m] : -1;       // gate g is drawn iff g >= ng
    const bool hl = dyn && a.next_gate && ng >= 0 && ng < t.n_gates;
    const int n_prim = dyn ? 2 * a.R + 2 : 0;

    int mask[PC_RENDER_LANE_ROWS] = {0, 0, 0, 0};      // 4 bits per pixel, the row's 4 pixels in 16 bits
    for (int base = 0; base < n_prim; base += PC_RENDER_CHUNK) {     // (workgroup-uniform: every thread meets every barrier)
        if (tid == 0) count = 0;
        __syncthreads();
        const int p = base + tid;
        bool have = false;
        int Ax = 0, Ay = 0, Bx = 0, By = 0, h2 = 0, bit = 0;
        if (p < 2 * a.R) {
            const int i = p < a.R ? p : p - a.R;
            const float e = o[6 + i];
            double d = isfinite(e) ? 1000.0 * (double)e : 0.0;
            d = d < 0.0 ? 0.0 : (d > 1000.0 ? 1000.0 : d);
            const double2 cs = a.dirs[i];
            const double dx = c * cs.x - s * cs.y, dy = s * cs.x + c * cs.y;
            Bx = render_q(x + d * dx);
            By = render_q(y + d * dy);
            if (p < a.R) {
                Ax = render_q(x); Ay = render_q(y); h2 = a.h2_ray; bit = PC_RENDER_BIT_RAY;
            } else {
                Ax = Bx; Ay = By; h2 = a.h2_hit; bit = PC_RENDER_BIT_HIT;
            }
            have = true;
        } else if (p == 2 * a.R) {
            Ax = render_q(x - 8.0 * c); Ay = render_q(y - 8.0 * s);
            Bx = render_q(x + 14.0 * c); By = render_q(y + 14.0 * s);
            h2 = a.h2_car; bit = PC_RENDER_BIT_CAR;
            have = true;
        } else if (p == 2 * a.R + 1 && hl) {
            const int4 g = a.gates[t.gate_off + ng];
            Ax = g.x; Ay = g.y; Bx = g.z; By = g.w; h2 = a.h2_gate; bit = PC_RENDER_BIT_NEXT;
            have = true;
        }
        // the primitive's box, grown by the widest half-width, against the tile's
        have = have && min(Ax, Bx) - a.h_max <= bx1 && max(Ax, Bx) + a.h_max >= bx0 && min(Ay, By) - a.h_max <= by1 && max(Ay, By) + a.h_max >= by0;
        const unsigned long long b = __ballot(have);
        int slot = 0;
        if (lane == 0 && b) slot = atomicAdd(&count, __popcll(b));
        slot = __shfl(slot, 0) + __popcll(b & ((1ull << lane) - 1ull));
        if (have) {
            const int ex = Bx - Ax, ey = By - Ay;
            seg[slot] = make_int4(Ax, Ay, ex, ey);
            aux[slot] = make_int4(ex * ex + ey * ey, h2, bit, 0);
        }
        __syncthreads();
        const int n = count;
        for (int q = 0; q < n; ++q) {
            const int4 g = seg[q], w = aux[q];
            const int du = sq * g.z, dc = sq * g.w;
#pragma unroll
            for (int r = 0; r < PC_RENDER_LANE_ROWS; ++r) {
                int wx = Px - g.x;
                const int wy = Py + 16 * r * sq - g.y;
                int u = wx * g.z + wy * g.w, cr = wx * g.w - wy * g.z;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (render_covers(wx, wy, g.z, g.w, w.x, w.y, u, cr)) mask[r] |= w.z << (4 * k);
                    wx += sq; u += du; cr += dc;
                }
            }
        }
        __syncthreads();
    }
    if (n_prim == 0) __syncthreads();       // the palette's writes
#pragma unroll
    for (int r = 0; r < PC_RENDER_LANE_ROWS; ++r) {
        const int j = j0 + 16 * r;
        if (!(i0 < a.W && j < a.H)) continue;
        uint32_t rgb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int col = (int)((layer4[r] >> (8 * k)) & 3u);
            const int gv = (int)((gate4[r] >> (8 * k)) & 255u);
            if (gv != 0 && gv > ng) col = PC_RENDER_GATE;       // plane 1 holds g + 1: drawn iff g >= ng
            const int mk = mask[r] >> (4 * k);
            if (mk & PC_RENDER_BIT_CAR) col = PC_RENDER_CAR;
            else if (mk & PC_RENDER_BIT_HIT) col = PC_RENDER_HIT;
            else if (mk & PC_RENDER_BIT_RAY) col = PC_RENDER_RAY;
            else if (mk & PC_RENDER_BIT_NEXT) col = PC_RENDER_NEXT_GATE;
            rgb[k] = pal[col];
        }
        uint32_t* const out = (uint32_t*)(a.frames + ((m * a.H + j) * (int64_t)a.W + i0) * 3);
        out[0] = rgb[0] | (rgb[1] << 24);
        out[1] = (rgb[1] >> 8) | (rgb[2] << 16);
        out[2] = (rgb[2] >> 16) | (rgb[3] << 8);
    }
}
