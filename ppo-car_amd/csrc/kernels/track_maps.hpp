// track_maps.hpp -- part of the single translation unit ppocar.hip (included there after evaluation.hpp; not a stand-alone header).
// K16 track_maps_kernel<STEPS, FIRST>: the rollout's observation rows reduced to per-cell counters (pc_track_maps).
#pragma once

// the largest plane held in LDS: cell_px = 8 (160 x 90 cells); two uint32 planes of it are 115 200 bytes of the CU's 160 KiB
#define PC_MAP_LDS_CELLS 14400
// rows a workgroup walks between two flushes of its LDS planes, and the largest q an LDS partial takes: 1024 lanes x 1024 rows x 2047
// stays below 2^32 (so does the visit count); a larger q (no car reaches it: |v| <= max_speed on both axes gives q <= 1449) goes
// straight to the global plane
#define PC_MAP_LDS_ROWS 1024
#define PC_MAP_LDS_QMAX 2048

// ------------------------------------------------------------------------------------------
// K16: where the cars were, how fast, where they crashed.  One lane per env, forward in t over the workgroup's rows [blockIdx.y * rows,
// + rows), U rows in flight per lane (K14's layout: with FIRST the walk over t is sequential per env, the loads are not).  Of every
// 4 D-byte observation row the lane reads entries 0-3; the flag rows are coalesced across envs.  obs is read once.
//   contention: right after a reset every env sits in ONE cell, in training most sit in a few.  So nothing is added to global memory
//   per sample: VISITS and SPEED go to two uint32 planes in LDS (planes of at most PC_MAP_LDS_CELLS cells, the workgroup's first env's
//   track), flushed with one 64-bit integer atomicAdd per non-zero cell every PC_MAP_LDS_ROWS rows; a wave whose counted lanes all sit
//   in one cell adds once (count, sum of q by a butterfly) instead of 64 times to one LDS address.  Samples the LDS planes do not take
//   -- smaller cells, an env of another track than the workgroup's first, a q >= PC_MAP_LDS_QMAX -- and the rare crashes add to the
//   global planes directly.  Every add is an integer add: the maps do not depend on which path a sample took, on the launch geometry
//   or on the order of arrival.
// FIRST: state row 4 of pc_first_episodes decides which envs count (RUNNING on entry), and an env stops counting after the step that
// closes its episode; the grid then has ONE workgroup row (blockIdx.y == 0 walks all T rows).
// STEPS: as in K14 (false: step t's flags in row t + 1, step T - 1's in last_*).
// ------------------------------------------------------------------------------------------
template <bool STEPS, bool FIRST>
__global__ __launch_bounds__(1024) void track_maps_kernel(const float* __restrict__ obs, const int64_t D, const float* __restrict__ term,
                                                          const float* __restrict__ trunc, const float* __restrict__ last_term,
                                                          const float* __restrict__ last_trunc, const int64_t T, const int64_t N,
                                                          const int64_t rows, const uint8_t* __restrict__ track_id, const int n_tracks,
                                                          const int GW, const int GH, const double* __restrict__ first_state,
                                                          unsigned long long* __restrict__ maps) {
    __shared__ uint32_t part[2 * PC_MAP_LDS_CELLS];     // [VISITS | SPEED][cells] of track wg_trk
    const int cells = GW * GH;
    const bool lds = cells <= PC_MAP_LDS_CELLS;
    const int64_t e0 = (int64_t)blockIdx.x * blockDim.x, e = e0 + threadIdx.x;
    const int wg_trk = track_id ? (int)track_id[e0] : 0;        // (e0 < N: the grid has ceil(N / blockDim.x) columns)
    const int trk = e < N ? (track_id ? (int)track_id[e] : 0) : n_tracks;
    bool running = trk < n_tracks;                              // an env past N or on a track without planes never counts
    if (FIRST && running) running = first_state[4 * N + e] == (double)PC_FIRST_RUNNING;
    const int64_t plane = (int64_t)cells;
    unsigned long long* const mine = maps + (int64_t)(running ? trk : 0) * PC_MAP_PLANES * plane;
    const float fw = (float)GW, fh = (float)GH;
    const auto flag = [=](const float* rows_, const float* last, const int64_t t) {
        if constexpr (STEPS) return rows_[t * N + e];
        else return t + 1 < T ? rows_[(t + 1) * N + e] : last[e];
    };
    // one sample of every lane of the wave (all 64 lanes arrive here together: the row loops below are wave-uniform)
    const auto sample = [&](const float o0, const float o1, const float o2, const float o3, const float tm, const float tr) {
        const bool use = running && isfinite(o0) && isfinite(o1);
        if (FIRST && running) running = tm == 0.0f && tr == 0.0f;       // the closing step itself counted
        const float fx = floorf(o0 * fw), fy = floorf(o1 * fh);
        const int cx = fx > 0.0f ? (fx < fw - 1.0f ? (int)fx : GW - 1) : 0;
        const int cy = fy > 0.0f ? (fy < fh - 1.0f ? (int)fy : GH - 1) : 0;
        const int cell = cy * GW + cx;
        const double s = sqrt((double)o2 * (double)o2 + (double)o3 * (double)o3) * (double)PC_MAP_SPEED_UNIT;
        const unsigned long long q = s < 9.0e18 ? (unsigned long long)(long long)rint(s) : 0ull;    // (not finite: 0)
        const bool small = q < PC_MAP_LDS_QMAX;
        const bool to_lds = lds && trk == wg_trk;
        const uint64_t mask = __ballot(use);
        if (mask == 0) return;
        const int key = use ? trk * cells + cell : -1;
        const int lead = __ffsll((unsigned long long)mask) - 1;
        const int key0 = __shfl(key, lead);
        if (__ballot(use && key == key0 && small) == mask) {            // one cell for the whole wave: one add of (count, sum of q)
            uint32_t sum = use ? (uint32_t)q : 0u;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
            if ((int)(threadIdx.x & 63) == lead) {
                const uint32_t cnt = (uint32_t)__popcll((unsigned long long)mask);
                if (to_lds) {
                    atomicAdd(&part[cell], cnt);
                    atomicAdd(&part[PC_MAP_LDS_CELLS + cell], sum);
                } else {
                    atomicAdd(&mine[PC_MAP_VISITS * plane + cell], (unsigned long long)cnt);
                    atomicAdd(&mine[PC_MAP_SPEED * plane + cell], (unsigned long long)sum);
                }
            }
        } else if (use) {
            if (to_lds) {
                atomicAdd(&part[cell], 1u);
                if (small) atomicAdd(&part[PC_MAP_LDS_CELLS + cell], (uint32_t)q);
                else atomicAdd(&mine[PC_MAP_SPEED * plane + cell], q);
            } else {
                atomicAdd(&mine[PC_MAP_VISITS * plane + cell], 1ull);
                atomicAdd(&mine[PC_MAP_SPEED * plane + cell], q);
            }
        }
        if (use && tm != 0.0f) atomicAdd(&mine[PC_MAP_CRASHES * plane + cell], 1ull);
    };
    const int64_t t_begin = (int64_t)blockIdx.y * rows, t_end = t_begin + rows < T ? t_begin + rows : T;
    constexpr int U = 8;  // rows in flight per lane
    for (int64_t tb = t_begin; tb < t_end; tb += PC_MAP_LDS_ROWS) {     // (workgroup-uniform: every thread meets every barrier)
        const int64_t te = tb + PC_MAP_LDS_ROWS < t_end ? tb + PC_MAP_LDS_ROWS : t_end;
        if (lds) {
            for (int i = threadIdx.x; i < cells; i += blockDim.x) part[i] = part[PC_MAP_LDS_CELLS + i] = 0u;
            __syncthreads();
        }
        int64_t t = tb;
        for (; t + U <= te && __any(running); t += U) {
            float o[U][4], tm[U], tr[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const float* const row = obs + ((t + j) * N + e) * D;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[j][k] = running ? row[k] : 0.0f;
                tm[j] = running ? flag(term, last_term, t + j) : 0.0f;
                tr[j] = FIRST && running ? flag(trunc, last_trunc, t + j) : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < U; ++j) sample(o[j][0], o[j][1], o[j][2], o[j][3], tm[j], tr[j]);
        }
        for (; t < te && __any(running); ++t) {
            const float* const row = obs + (t * N + e) * D;
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = running ? row[k] : 0.0f;
            const float tm = running ? flag(term, last_term, t) : 0.0f;
            const float tr = FIRST && running ? flag(trunc, last_trunc, t) : 0.0f;
            sample(o[0], o[1], o[2], o[3], tm, tr);
        }
        if (lds) {
            __syncthreads();
            unsigned long long* const wg = maps + (int64_t)wg_trk * PC_MAP_PLANES * plane;
            for (int i = threadIdx.x; i < cells; i += blockDim.x) {
                const uint32_t v = part[i], q = part[PC_MAP_LDS_CELLS + i];
                if (v) atomicAdd(&wg[PC_MAP_VISITS * plane + i], (unsigned long long)v);
                if (q) atomicAdd(&wg[PC_MAP_SPEED * plane + i], (unsigned long long)q);
            }
            __syncthreads();
        }
    }
}
