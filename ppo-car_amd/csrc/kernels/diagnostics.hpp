// diagnostics.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K14 explained_variance_kernel / explained_variance_final_kernel: 1 - Var(ret - val) / Var(ret) over a whole rollout.
#pragma once

// ------------------------------------------------------------------------------------------
// K14: the critic's explained variance over val[M], ret[M] (float32 in, float64 throughout), two launches, fixed order, no atomics.
// HBM-bound: 8 B per sample, 16-byte loads, grid-stride over a grid sized to the device.
// A running (count, mean, M2) triple per series (x = ret, d = ret - val).  Per thread the sums are taken about a shift K = the
// series' first sample, sum(x - K) and sum((x - K)^2) -- the samples of one rollout lie within a few standard deviations of any of
// them, so nothing of the size of mean^2 is ever added up (the E[x^2] - E[x]^2 form loses (mean / std)^2 of its precision) -- then
// converted once to (n, mean, M2) and merged up the tree lane -> wave -> workgroup -> grid by Chan's pairwise update
//   n = na + nb;  delta = mb - ma;  mean = ma + delta nb / n;  M2 = M2a + M2b + delta^2 na nb / n.
// ------------------------------------------------------------------------------------------
constexpr int PC_EV_MAX_BLOCKS = 2048;   // the first stage's grid never exceeds this (pc_explained_variance_workspace_doubles)

struct EvAcc { double n, mx, qx, md, qd; };   // count; mean and M2 of ret; mean and M2 of ret - val

__device__ __forceinline__ EvAcc ev_merge(const EvAcc a, const EvAcc b) {
    const double n = a.n + b.n;
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double w = b.n / n, c = a.n * w;
    const double dx = b.mx - a.mx, dd = b.md - a.md;
    return EvAcc{n, a.mx + dx * w, a.qx + b.qx + dx * dx * c, a.md + dd * w, a.qd + b.qd + dd * dd * c};
}

// lane 0 of every wave ends with the wave's merge (lanes i and i + off, off = 32 .. 1: one fixed tree); then thread 0 merges the waves
// in index order.  The result is valid in thread 0 only.
__device__ __forceinline__ EvAcc ev_block_merge(EvAcc a, EvAcc* sh) {
    for (int off = 32; off >= 1; off >>= 1) {
        EvAcc b;
        b.n = __shfl_down(a.n, off, 64);
        b.mx = __shfl_down(a.mx, off, 64);
        b.qx = __shfl_down(a.qx, off, 64);
        b.md = __shfl_down(a.md, off, 64);
        b.qd = __shfl_down(a.qd, off, 64);
        a = ev_merge(a, b);
    }
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < nw; ++i) a = ev_merge(a, sh[i]);
    return a;
}

// stage 1: workgroup b leaves its (n, mean_ret, M2_ret, mean_diff, M2_diff) in partial[5 b ..]
__global__ __launch_bounds__(256) void explained_variance_kernel(const float* __restrict__ val, const float* __restrict__ ret, const int64_t M,
                                                                 const int vec, double* __restrict__ partial) {
    __shared__ EvAcc sh[4];
    const double kx = (double)ret[0], kd = (double)ret[0] - (double)val[0];     // the shifts: every thread the same two loads
    double n = 0.0, sx = 0.0, qx = 0.0, sd = 0.0, qd = 0.0;
    auto add = [&](const float v, const float r) {
        const double x = (double)r - kx, d = ((double)r - (double)v) - kd;
        sx += x;
        qx += x * x;
        sd += d;
        qd += d * d;
    };
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const int64_t M4 = vec ? M >> 2 : 0;      // (vec: both arrays 16-byte aligned)
    const f32x4* __restrict__ v4 = reinterpret_cast<const f32x4*>(val);
    const f32x4* __restrict__ r4 = reinterpret_cast<const f32x4*>(ret);
    int64_t i = tid;
    for (; i + nthr < M4; i += 2 * nthr) {    // two 16-byte loads per array in flight
        const f32x4 va = v4[i], ra = r4[i], vb = v4[i + nthr], rb = r4[i + nthr];
#pragma unroll
        for (int c = 0; c < 4; ++c) add(va[c], ra[c]);
#pragma unroll
        for (int c = 0; c < 4; ++c) add(vb[c], rb[c]);
        n += 8.0;
    }
    for (; i < M4; i += nthr) {
        const f32x4 va = v4[i], ra = r4[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) add(va[c], ra[c]);
        n += 4.0;
    }
    for (int64_t j = 4 * M4 + tid; j < M; j += nthr) {
        add(val[j], ret[j]);
        n += 1.0;
    }
    EvAcc a{n, kx, 0.0, kd, 0.0};
    if (n > 0.0) {
        a.mx = kx + sx / n;
        a.qx = qx - sx * sx / n;
        a.md = kd + sd / n;
        a.qd = qd - sd * sd / n;
    }
    a = ev_block_merge(a, sh);
    if (threadIdx.x == 0) {
        double* __restrict__ p = partial + 5 * (size_t)blockIdx.x;
        p[0] = a.n;
        p[1] = a.mx;
        p[2] = a.qx;
        p[3] = a.md;
        p[4] = a.qd;
    }
}

// stage 2 (one workgroup): merges the n_part partials -- thread t its partials t, t + 256, ... in order, then the same tree -- and
// writes out[5] = (mean_ret, M2_ret, mean_diff, M2_diff, 1 - M2_diff / M2_ret; NaN when M2_ret == 0: population variances share M)
__global__ __launch_bounds__(256) void explained_variance_final_kernel(const double* __restrict__ partial, const int n_part, double* __restrict__ out) {
    __shared__ EvAcc sh[4];
    EvAcc a{0.0, 0.0, 0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < n_part; p += 256) {
        const double* __restrict__ q = partial + 5 * (size_t)p;
        a = ev_merge(a, EvAcc{q[0], q[1], q[2], q[3], q[4]});
    }
    a = ev_block_merge(a, sh);
    if (threadIdx.x == 0) {
        out[0] = a.mx;
        out[1] = a.qx;
        out[2] = a.md;
        out[3] = a.qd;
        out[4] = a.qx == 0.0 ? __builtin_nan("") : 1.0 - a.qd / a.qx;
    }
}
