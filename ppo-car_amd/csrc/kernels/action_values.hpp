// action_values.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K28 action_values_kernel (pc_sequences_action_values): what the best sequence BEGINNING WITH each of the nine actions earned, from
// the score table a K22 / K25 / K26 launch left -- q [M][9], how many sequences begin with each action, whether one of them outlives
// its first step, and a soft target over the actions that do.  sequences_best_kernel's shape: one wave per state (4 per workgroup),
// lane l walks k = l, l + 64, ... with nine running maxima in registers, then nine butterflies with ties to the lower k.  No atomics,
// no LDS, float64 compares only: the result is exact and does not depend on the launch geometry.
#pragma once

struct ActionValues {
    const double* __restrict__ ret;           // [M][K]
    const uint8_t* __restrict__ actions;      // the first time row of the table: state m, sequence k at actions[m * state_stride + k]
    int64_t state_stride;
    const int32_t* __restrict__ steps;        // [M][K], both or neither
    const uint8_t* __restrict__ status;
    const uint8_t* __restrict__ active;       // [M] or nullptr
    int64_t M;
    int K, accumulate;
    double temperature;
    double* __restrict__ q;                   // [M][9] each
    int32_t* __restrict__ count;
    uint8_t* __restrict__ alive;
    float* __restrict__ target;               // or nullptr
};

__global__ __launch_bounds__(256) void action_values_kernel(const ActionValues p) {
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= p.M) return;      // (whole waves)
    if (p.active && p.active[m] == 0) return;
    const double* __restrict__ row = p.ret + m * p.K;
    const uint8_t* __restrict__ first = p.actions + m * p.state_stride;
    double best[9];
    int at[9], cnt[9];
    unsigned live = 0;      // bit a: a sequence of action a that is not dead at once
#pragma unroll
    for (int a = 0; a < 9; ++a) {
        best[a] = 0.0;
        at[a] = INT_MAX;
        cnt[a] = 0;
    }
    for (int k = lane; k < p.K; k += 64) {
        const double v = row[k];
        const int act = seq_action(first[k]);
        const bool dead = p.status && p.status[m * p.K + k] == PC_FIRST_TERMINATED && p.steps[m * p.K + k] == 1;
        if (!dead) live |= 1u << act;
#pragma unroll
        for (int a = 0; a < 9; ++a) {      // (a select per action keeps the nine in registers)
            const bool mine = a == act;
            if (mine && (at[a] == INT_MAX || v > best[a])) {
                best[a] = v;
                at[a] = k;
            }
            cnt[a] += mine ? 1 : 0;
        }
    }
    for (int s = 1; s < 64; s <<= 1) {
        live |= (unsigned)__shfl_xor((int)live, s, 64);
#pragma unroll
        for (int a = 0; a < 9; ++a) {
            const double ob = __hiloint2double(__shfl_xor(__double2hiint(best[a]), s, 64), __shfl_xor(__double2loint(best[a]), s, 64));
            const int oa = __shfl_xor(at[a], s, 64);
            if (oa != INT_MAX && (at[a] == INT_MAX || ob > best[a] || (ob == best[a] && oa < at[a]))) {
                best[a] = ob;
                at[a] = oa;
            }
            cnt[a] += __shfl_xor(cnt[a], s, 64);
        }
    }
    if (lane != 0) return;
    double qv[9];
    unsigned set = 0;      // the alive actions of the merged row
    double qmax = -INFINITY;
#pragma unroll
    for (int a = 0; a < 9; ++a) {
        const int64_t o = m * 9 + a;
        double v = cnt[a] > 0 ? best[a] : -INFINITY;
        int c = cnt[a];
        bool al = p.status ? ((live >> a) & 1u) != 0 : cnt[a] > 0;
        if (p.accumulate) {
            const double old = p.q[o];
            if (!(v > old)) v = old;      // only a strictly greater return replaces the kept one
            c += p.count[o];
            al = al || p.alive[o] != 0;
        }
        p.q[o] = v;
        p.count[o] = c;
        p.alive[o] = al ? 1 : 0;
        qv[a] = v;
        if (al) {
            set |= 1u << a;
            if (v > qmax) qmax = v;
        }
    }
    if (!p.target) return;
    double e[9], sum = 0.0;
    if (p.temperature == 0.0) {
        int n = 0;
#pragma unroll
        for (int a = 0; a < 9; ++a) {
            e[a] = ((set >> a) & 1u) && qv[a] == qmax ? 1.0 : 0.0;
            n += e[a] != 0.0 ? 1 : 0;
        }
        sum = (double)n;
    } else {
#pragma unroll
        for (int a = 0; a < 9; ++a) {      // (summed in ascending a)
            e[a] = (set >> a) & 1u ? exp((qv[a] - qmax) / p.temperature) : 0.0;
            sum += e[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) {
        float t = 0.0f;
        if (set != 0 && e[a] != 0.0) t = p.temperature == 0.0 ? (float)(1.0 / sum) : (float)(e[a] / sum);
        p.target[m * 9 + a] = t;
    }
}
