// update_large.hpp -- part of the single translation unit ppocar.hip (included there after update.hpp; not a stand-alone header).
// KLs and K10L: the PPO minibatch step for minibatches above K10's 1024 samples (pc_ppo_adv_stats, pc_ppo_minibatch_large).
//   KLs  ppo_adv_stats_large_kernel + ppo_adv_stats_merge_kernel : (mean, max(unbiased std, 1e-5)) of the gathered advantages of n_mb
//        minibatches, float64 shifted sums, several workgroups per minibatch and a fixed-order merge
//   K10L ppo_fwdbwd_large_kernel : K10's per-sample arithmetic, but a FIXED grid: workgroup g keeps the parameters and the gradient
//        accumulators of its hidden units in registers and walks the sample groups g, g + G, g + 2 G, ... (8 samples each); the index
//        and row loads of the next group are in flight under the arithmetic of the current one
// K10L leaves one gradient partial and one (pl, vl, ent, -) partial per workgroup in K10's layout: K11 and K12 follow unchanged.
// No atomics, one summation order (per workgroup: its groups in walking order; across workgroups: K11's index order).
#pragma once

constexpr int AS_THREADS = 256;          // KLs: threads per workgroup
constexpr int AS_PER_WG = 2048;          // ... samples per workgroup at least (one workgroup up to 2048, 64 from 129 k samples on)
constexpr int AS_MAX_WG = 64;            // ... workgroups per minibatch at most: the merge is one wave
__host__ __device__ inline int adv_stats_parts(const int B) {
    const int p = (B + AS_PER_WG - 1) / AS_PER_WG;
    return p < 1 ? 1 : (p > AS_MAX_WG ? AS_MAX_WG : p);
}

// 64-lane sum of a double in a fixed (butterfly) order: every lane ends with the same bits
__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// KLs, stage 1: workgroup (p, mb) sums (x - K) and (x - K)^2 over its slice of minibatch mb in float64, K = the minibatch's first
// gathered advantage (a shift inside the data: the sums stay of the order of the deviations, nothing cancels as in E[x^2] - E[x]^2).
// Slices are contiguous and a multiple of the workgroup wide; a thread's terms are added in index order, the threads of a wave by
// the butterfly above, the waves in order.
__global__ __launch_bounds__(AS_THREADS) void ppo_adv_stats_large_kernel(const int64_t* __restrict__ idx, const int64_t idx_ld, const int B,
                                                                         const float* __restrict__ adv, double* __restrict__ part) {
    __shared__ double shd[2][AS_THREADS / 64];
    const int u = threadIdx.x, P = gridDim.x, p = blockIdx.x, mb = blockIdx.y;
    const int64_t* __restrict__ ix = idx + (int64_t)mb * idx_ld;
    const double K = (double)adv[ix[0]];
    const int slice = ((B + P - 1) / P + AS_THREADS - 1) / AS_THREADS * AS_THREADS;
    const int lo = p * slice, hi = lo + slice < B ? lo + slice : B;
    double s1 = 0.0, s2 = 0.0;
    for (int i0 = lo + u; i0 < hi; i0 += 8 * AS_THREADS) {      // eight index loads, then eight dependent gathers, in flight together
        int64_t src[8];
        float a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) src[j] = i0 + j * AS_THREADS < hi ? ix[i0 + j * AS_THREADS] : ix[0];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = adv[src[j]];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double d = i0 + j * AS_THREADS < hi ? (double)a[j] - K : 0.0;
            s1 += d;
            s2 += d * d;
        }
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    if ((u & 63) == 0) {
        shd[0][u >> 6] = s1;
        shd[1][u >> 6] = s2;
    }
    __syncthreads();
    if (u < 2) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < AS_THREADS / 64; ++w) t += shd[u][w];
        part[((int64_t)mb * P + p) * 2 + u] = t;
    }
}

// KLs, stage 2: one wave per minibatch adds the P <= 64 partial pairs (butterfly: a fixed order) and rounds to float32 ONCE:
// mean = K + S1 / B, var = (S2 - S1^2 / B) / (B - 1) in float64 (train.py:238-240: Tensor.std() is the unbiased one).
__global__ __launch_bounds__(64) void ppo_adv_stats_merge_kernel(const int64_t* __restrict__ idx, const int64_t idx_ld, const int B, const int P,
                                                                 const float* __restrict__ adv, const double* __restrict__ part,
                                                                 float* __restrict__ stats) {
    const int u = threadIdx.x, mb = blockIdx.x;
    const double K = (double)adv[idx[(int64_t)mb * idx_ld]];
    const double s1 = wave_sum_f64(u < P ? part[((int64_t)mb * P + u) * 2] : 0.0);
    const double s2 = wave_sum_f64(u < P ? part[((int64_t)mb * P + u) * 2 + 1] : 0.0);
    if (u == 0) {
        const double n = (double)B;
        const double var = (s2 - s1 * s1 / n) / (n - 1.0);
        stats[mb * 2] = (float)(K + s1 / n);
        stats[mb * 2 + 1] = fmaxf((float)sqrt(var > 0.0 ? var : 0.0), 1e-5f);       // torch.max(std, 1e-5)
    }
}

// K10L.  The phases are K10's (ppo_fwdbwd_body, update.hpp: the comments there explain each), restated here around a loop so that
// K10's instantiations stay as they are: parameters once, then per group { samples into LDS | next group's loads issued | layer 1 |
// layer 2 | loss | backward into the register accumulators }, then the partial once.  Inside the loop every barrier is the LDS-only
// one: __syncthreads() would wait for the prefetch.  The loads run two groups ahead for the indices and one for the rows, so neither
// of the two dependent cold misses (idx -> obs row) is waited for by the group that issues it.
// adv_stats: this minibatch's (mean, max(std, 1e-5)) from KLs.
template <int DMAX, int AC = 0, int DC = 0>
__global__ __launch_bounds__(256) void ppo_fwdbwd_large_kernel(const int64_t* __restrict__ idx, const int B, const int D_rt, const int A_rt,
                                                               const float* __restrict__ obs, const float* __restrict__ act,
                                                               const float* __restrict__ old_lp, const float* __restrict__ adv,
                                                               const float* __restrict__ ret, const float* __restrict__ adv_stats,
                                                               const float* __restrict__ param, const float clip, const float vf,
                                                               const float ec, float* __restrict__ partial, float* __restrict__ metric_partial) {
    constexpr int H = 256, S = FB_S, LDT = DMAX + 1, LDH = H + 1;
    const int A = AC > 0 ? AC : A_rt, D = DC > 0 ? DC : D_rt;
    static_assert(DC <= DMAX, "observation width");
    __shared__ float sX[S][DMAX];
    __shared__ float sOut[S][16];
    __shared__ float sDout[S][16];
    __shared__ float sMet[S][3];                                          // pl, vl, ent of the group's samples
    __shared__ float sSmp[S][4];                                          // act, old_lp, adv, ret of the group's samples
    __shared__ __attribute__((aligned(16))) float sT[H * LDT > 2 * S * LDH + 16 * LDH + 4 * S * 16 ? H * LDT : 2 * S * LDH + 16 * LDH + 4 * S * 16];
    static_assert(H * LDT >= H * DMAX + 8, "the tile holds one [H][D] block in natural order plus an alignment shift");
    float* sHid = sT;                    // [2][S][LDH]  hidden activations (actor, critic)         } alias the transposition
    float* sW2 = sT + 2 * S * LDH;       // [16][LDH]    output-layer weights, row A = the critic's  } tile: used between
    float* sP2 = sW2 + 16 * LDH;         // [<= 4][S][16] the k-parts of layer 2                     } the load and store phases
    const int u = threadIdx.x, wg = blockIdx.x, G = gridDim.x;
    const int n_grp = (B + S - 1) / S;
    const int o_aW1 = 0, o_ab1 = H * D, o_aW2 = o_ab1 + H, o_ab2 = o_aW2 + A * H, o_cW1 = o_ab2 + A, o_cb1 = o_cW1 + H * D,
              o_cW2 = o_cb1 + H, o_cb2 = o_cW2 + H, n_param = o_cb2 + 1;

    // ---- the sample pipeline: slot j of thread u is element u + 256 j of the group's [S][DMAX] tile; threads 0..S-1 also own one
    // sample's four scalars.  All row addresses in 64 bits (idx * D passes 2^31 at 65536 envs x 1024 steps).
    constexpr int NX = (S * DMAX + 255) / 256;
    int x_s[NX], x_f[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        const int i = u + 256 * j;
        x_s[j] = i / DMAX;
        x_f[j] = i - x_s[j] * DMAX;
    }
    // Every load of the pipeline is UNCONDITIONAL on a clamped address (a dead slot re-reads a live one's line) and the masks are
    // applied when the values go to LDS: a `cond ? load : 0` is a zero write plus a branch around the load, and the zero write made
    // the compiler wait for every load in flight -- the prefetch was waited for where it was issued.
    int64_t nx_src[NX], ns_src;          // the indices of the group after next
    float nx_val[NX], ns_val[4];         // the rows and scalars of the next group
    auto load_indices = [&](const int g) {
        const int s0 = g * S;
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const int b = s0 + (x_s[j] < S ? x_s[j] : S - 1);
            nx_src[j] = idx[b < B ? b : B - 1];
        }
        const int b = s0 + (u & (S - 1));
        ns_src = idx[b < B ? b : B - 1];
    };
    auto load_rows = [&]() {
#pragma unroll
        for (int j = 0; j < NX; ++j) nx_val[j] = obs[nx_src[j] * (int64_t)D + (x_f[j] < D ? x_f[j] : D - 1)];
        ns_val[0] = act[ns_src];
        ns_val[1] = old_lp[ns_src];
        ns_val[2] = adv[ns_src];
        ns_val[3] = ret[ns_src];
    };
    load_indices(wg);                    // (wg < n_grp: the grid is min(groups, cap))

    // ---- the parameters, once: all loads issued before the first wait (as K10)
    float w2a[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) w2a[o] = o < A ? param[o_aW2 + o * H + u] : 0.0f;
    const float w2c = param[o_cW2 + u], b1a = param[o_ab1 + u], b1c = param[o_cb1 + u];
    const int ob = u & 15;                                                // my output index in the layer-2 epilogue
    const float b2 = ob <= A ? param[ob < A ? o_ab2 + ob : o_cb2] : 0.0f;
    const float mean = adv_stats[0], sd = adv_stats[1];
    constexpr int NV4 = (H * DMAX + 3 + 1023) / 1024 + 1;
    f32x4 w1raw4[2][NV4];
    int w1_shift[2], w1_n4[2];
#pragma unroll
    for (int net = 0; net < 2; ++net) {
        const int off = net == 0 ? o_aW1 : o_cW1, b4 = off & ~3;
        w1_shift[net] = off - b4;
        w1_n4[net] = (off + H * D - b4 + 3) >> 2;
        const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(param + b4);
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            const int i4 = u + 256 * j;
            const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
            w1raw4[net][j] = i4 < w1_n4[net] ? src[i4] : z;
        }
    }
    load_rows();
    load_indices(wg + G < n_grp ? wg + G : wg);
    // ---- W1 rows into registers through the LDS tile (one net at a time)
    float w1a[DMAX], w1c[DMAX];
#pragma unroll
    for (int net = 0; net < 2; ++net) {
        lds_barrier();
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            const int i4 = u + 256 * j;
            if (i4 < w1_n4[net]) reinterpret_cast<f32x4*>(sT)[i4] = w1raw4[net][j];
        }
        lds_barrier();
        const float* row = sT + w1_shift[net] + u * D;
#pragma unroll
        for (int f = 0; f < DMAX; ++f) {
            const float w = f < D ? row[f] : 0.0f;
            if (net == 0) w1a[f] = w;
            else w1c[f] = w;
        }
    }
    lds_barrier();   // every thread has read its W1 row out of the tile, which sHid / sW2 alias
#pragma unroll
    for (int o = 0; o < 16; ++o) sW2[o * LDH + u] = o < A ? w2a[o] : (o == A ? w2c : 0.0f);

    // ---- the accumulators of the whole walk
    const float invB = 1.0f / (float)B;
    float g1a[DMAX], g1c[DMAX], g2a[16], g2c = 0.0f, gb1a = 0.0f, gb1c = 0.0f;
    float gb2 = 0.0f;                    // threads 0..A: the output-layer bias gradient
    float met = 0.0f;                    // threads 0..2: pl, vl, ent
#pragma unroll
    for (int f = 0; f < DMAX; ++f) {
        g1a[f] = 0.0f;
        g1c[f] = 0.0f;
    }
#pragma unroll
    for (int o = 0; o < 16; ++o) g2a[o] = 0.0f;
    constexpr bool ROLLED = DMAX > 24;   // (as K10: the 40-wide form re-reads the activations from LDS in the backward pass)
    const int n_out = A + 1, n_pair = S * n_out, n_kp = 256 / n_pair < 4 ? 256 / n_pair : 4;

#pragma unroll 1
    for (int g = wg; g < n_grp; g += G) {
        const int s0 = g * S;
        lds_barrier();   // the previous group's readers of sX / sSmp / sDout / sMet are done
#pragma unroll
        for (int j = 0; j < NX; ++j)
            if (x_s[j] < S) sX[x_s[j]][x_f[j]] = (s0 + x_s[j] < B && x_f[j] < D) ? nx_val[j] : 0.0f;
        if (u < S) {
#pragma unroll
            for (int c = 0; c < 4; ++c) sSmp[u][c] = s0 + u < B ? ns_val[c] : 0.0f;
        }
        // in flight under this group's arithmetic: the next group's rows (their indices arrived a group ago), then the indices of
        // the group after it.  Past the end of the walk the last group's are requested again and never used.
        load_rows();
        load_indices(g + 2 * G < n_grp ? g + 2 * G : g);
        lds_barrier();
        // ---- forward, layer 1 (Linear + ReLU), both nets
        float ha[ROLLED ? 1 : S], hc[ROLLED ? 1 : S];
#pragma unroll
        for (int sidx = 0; sidx < (ROLLED ? 0 : S); ++sidx) {
            float za = b1a, zc = b1c;
#pragma unroll
            for (int f = 0; f < DMAX; ++f) {
                za = __builtin_fmaf(w1a[f], sX[sidx][f], za);
                zc = __builtin_fmaf(w1c[f], sX[sidx][f], zc);
            }
            ha[sidx] = fmaxf(za, 0.0f);
            hc[sidx] = fmaxf(zc, 0.0f);
            sHid[sidx * LDH + u] = ha[sidx];
            sHid[(S + sidx) * LDH + u] = hc[sidx];
        }
        if constexpr (ROLLED) {
#pragma unroll 1
            for (int sidx = 0; sidx < S; ++sidx) {
                float za = b1a, zc = b1c;
#pragma unroll
                for (int f = 0; f < DMAX; ++f) {
                    za = __builtin_fmaf(w1a[f], sX[sidx][f], za);
                    zc = __builtin_fmaf(w1c[f], sX[sidx][f], zc);
                }
                sHid[sidx * LDH + u] = fmaxf(za, 0.0f);
                sHid[(S + sidx) * LDH + u] = fmaxf(zc, 0.0f);
            }
        }
        lds_barrier();
        // ---- forward, layer 2: the S (A + 1) dot products in n_kp k-parts, parts summed in order
        {
            const int kp = u / n_pair, pr = u - kp * n_pair, sidx = pr / n_out, o = pr - sidx * n_out;
            if (kp < n_kp) {
                const int k0 = H * kp / n_kp, k1 = H * (kp + 1) / n_kp;
                const float* hrow = sHid + ((o < A ? 0 : S) + sidx) * LDH;
                const float* wrow = sW2 + o * LDH;
                float acc = 0.0f;
#pragma unroll 8
                for (int k = k0; k < k1; ++k) acc = __builtin_fmaf(wrow[k], hrow[k], acc);
                sP2[(kp * S + sidx) * 16 + o] = acc;
            }
        }
        lds_barrier();
        if (u < S * 16) {
            const int sidx = u >> 4, o = u & 15;
            if (o <= A) {
                float t = b2;
                for (int kp = 0; kp < n_kp; ++kp) t += sP2[(kp * S + sidx) * 16 + o];
                sOut[sidx][o] = t;
            }
        }
        lds_barrier();
        // ---- loss and its gradient w.r.t. the outputs, 16 lanes per sample (K10's sequence)
        if (u < S * 16) {
#define PC_ROW_ROR(v, n) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + (n), 0xf, 0xf, false))
            const int sidx = u >> 4, k = u & 15, b = s0 + sidx;
            const bool live = b < B;
            const float o = sOut[sidx][k];
            const float l = k < A ? o : -INFINITY;
            float mx = l;
            mx = fmaxf(mx, PC_ROW_ROR(mx, 8));
            mx = fmaxf(mx, PC_ROW_ROR(mx, 4));
            mx = fmaxf(mx, PC_ROW_ROR(mx, 2));
            mx = fmaxf(mx, PC_ROW_ROR(mx, 1));
            const float ex = k < A ? expf(l - mx) : 0.0f;
            float sum = ex;
            sum += PC_ROW_ROR(sum, 8);
            sum += PC_ROW_ROR(sum, 4);
            sum += PC_ROW_ROR(sum, 2);
            sum += PC_ROW_ROR(sum, 1);
            const float lse = mx + logf(sum), inv = 1.0f / sum;
            const float lpk = k < A ? l - lse : 0.0f;
            const float pk = ex * inv;
            float ent = -(pk * lpk);
            ent += PC_ROW_ROR(ent, 8);
            ent += PC_ROW_ROR(ent, 4);
            ent += PC_ROW_ROR(ent, 2);
            ent += PC_ROW_ROR(ent, 1);
            const int a = (int)sSmp[sidx][0];
            const float new_lp = __shfl(lpk, (u & 48) + (a & 15), 64);
            const float r = expf(new_lp - sSmp[sidx][1]);                         // train.py:235
            const float An = (sSmp[sidx][2] - mean) / sd;                         // :238-240
            const float rc = fminf(fmaxf(r, 1.0f - clip), 1.0f + clip);
            const float pl1 = -An * r, pl2 = -An * rc;                            // :243-244
            const float pl = fmaxf(pl1, pl2);                                     // :245
            const float dv = __shfl(o, (u & 48) + A, 64) - sSmp[sidx][3];
            const float vl = 0.5f * dv * dv;                                      // :249
            const float g_lp = (pl1 >= pl2 ? -An : 0.0f) * r * invB;
            float dk = 0.0f;
            if (k < A) dk = g_lp * ((k == a ? 1.0f : 0.0f) - pk) + ec * invB * pk * (lpk + ent);
            else if (k == A) dk = vf * dv * invB;
            sDout[sidx][k] = live ? dk : 0.0f;
            if (k == 0) {
                sMet[sidx][0] = live ? pl : 0.0f;
                sMet[sidx][1] = live ? vl : 0.0f;
                sMet[sidx][2] = live ? ent : 0.0f;
            }
#undef PC_ROW_ROR
        }
        lds_barrier();
        // ---- backward: every thread for its hidden unit, into the walk's accumulators
        auto backward_sample = [&](const int sidx, const float h_a, const float h_c) {
            float dha = 0.0f;
#pragma unroll
            for (int o = 0; o < 16; ++o) {
                if (o < A) {
                    const float d = sDout[sidx][o];
                    dha = __builtin_fmaf(w2a[o], d, dha);
                    g2a[o] = __builtin_fmaf(d, h_a, g2a[o]);
                }
            }
            const float dval = sDout[sidx][A];
            g2c = __builtin_fmaf(dval, h_c, g2c);
            dha = h_a > 0.0f ? dha : 0.0f;                           // ReLU backward (threshold at 0)
            const float dhc = h_c > 0.0f ? w2c * dval : 0.0f;
            gb1a += dha;
            gb1c += dhc;
#pragma unroll
            for (int f = 0; f < DMAX; ++f) {
                g1a[f] = __builtin_fmaf(dha, sX[sidx][f], g1a[f]);
                g1c[f] = __builtin_fmaf(dhc, sX[sidx][f], g1c[f]);
            }
        };
        if constexpr (ROLLED) {
#pragma unroll 1
            for (int sidx = 0; sidx < S; ++sidx) backward_sample(sidx, sHid[sidx * LDH + u], sHid[(S + sidx) * LDH + u]);
        } else {
#pragma unroll
            for (int sidx = 0; sidx < S; ++sidx) backward_sample(sidx, ha[sidx], hc[sidx]);
        }
        if (u <= A) {    // output-layer biases: the group's samples in order, then onto the walk's sum
            float t = 0.0f;
#pragma unroll
            for (int sidx = 0; sidx < S; ++sidx) t += sDout[sidx][u];
            gb2 += t;
        }
        if (u < 3) {
            float t = 0.0f;
#pragma unroll
            for (int sidx = 0; sidx < S; ++sidx) t += sMet[sidx][u];
            met += t;
        }
    }

    // ---- this workgroup's partials, in K10's layout (ppo_partial_index): [aW1 (H D)][cW1 (H D)][ab1, aW2, ab2][cb1, cW2, cb2], rows
    // of n_pad floats
    const int HD = H * D, n_pad = (n_param + 3) & ~3;
    float* __restrict__ P = partial + (size_t)wg * n_pad;
    float* __restrict__ Pm = P + HD;
    Pm[o_ab1 + u] = gb1a;
    P[o_cb1 + u] = gb1c;
#pragma unroll
    for (int o = 0; o < 16; ++o)
        if (o < A) Pm[o_aW2 + o * H + u] = g2a[o];
    P[o_cW2 + u] = g2c;
    if (u < A) Pm[o_ab2 + u] = gb2;
    else if (u == A) P[o_cb2] = gb2;
    if (u < 3) metric_partial[wg * 4 + u] = met;
#pragma unroll
    for (int net = 0; net < 2; ++net) {
        lds_barrier();   // (the last group's readers of sHid, which the tile aliases, are done | the other net's stores have read it)
#pragma unroll
        for (int f = 0; f < DMAX; ++f)
            if (f < D) sT[u * D + f] = net == 0 ? g1a[f] : g1c[f];
        lds_barrier();
        f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(P + net * HD);
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            const int i4 = u + 256 * j;
            if (i4 < (HD >> 2)) dst[i4] = reinterpret_cast<const f32x4*>(sT)[i4];
        }
    }
}
