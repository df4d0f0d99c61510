// cem.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// The two steps that turn K22's shooting into the cross-entropy method: K23 cem_sample_kernel (pc_cem_sample) draws every state's K
// sequences from that state's own per-step action weights, K24 cem_refit_kernel (pc_cem_refit) moves those weights towards the E
// best-scoring sequences.  Between them sits K22 on the table K23 filled (one table per state, actions_state_stride = H * K).
// All arithmetic is integer: the weights are uint32 counts in 0 .. 65536 (16.16 fixed point of a probability, unnormalised), the draw
// multiplies a raw Philox word by the row's sum, the refit counts elites.  Nothing depends on the launch geometry.
#pragma once

constexpr int CEM_A = 9;                  // CarEnv's actions
constexpr uint32_t CEM_W_MAX = 65536u;    // the largest weight; anything above is read as this

// One row [9] of weights as BOTH kernels read it: clamped to CEM_W_MAX, and an all-zero row as nine ones.  Returns the row's sum.
__device__ __forceinline__ uint32_t cem_load_row(const uint32_t* __restrict__ row, uint32_t (&w)[CEM_A]) {
    uint32_t S = 0;
#pragma unroll
    for (int a = 0; a < CEM_A; ++a) {
        w[a] = row[a] > CEM_W_MAX ? CEM_W_MAX : row[a];
        S += w[a];      // at most 9 * 65536
    }
    if (S == 0) {
#pragma unroll
        for (int a = 0; a < CEM_A; ++a) w[a] = 1;
        S = CEM_A;
    }
    return S;
}

struct CemSample {
    const uint32_t* __restrict__ weights;     // [M][H][9]
    const uint8_t* __restrict__ keep;         // [M][H], or nullptr
    const uint8_t* __restrict__ active;       // [M], or nullptr
    uint8_t* __restrict__ table;              // [M][H][K]
    int64_t M;
    int H, K, const_columns;
    uint64_t seed, offset;
};

// K23.  Lane idx = (m * H + t) * K + k writes table[idx]: a constant column, the kept sequence, or the inverse CDF of its row's weights
// at r = (x * S) >> 32 < S, x the raw word (offset & 3) of the stream's block for (seed, offset >> 2, idx) (gae_sample.hpp).
__global__ __launch_bounds__(256) void cem_sample_kernel(const CemSample q) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= q.M * q.H * q.K) return;
    const int64_t row = idx / q.K;      // m * H + t
    const int k = (int)(idx - row * q.K);
    if (q.active && q.active[row / q.H] == 0) return;
    int act;
    if (q.const_columns && k < CEM_A) {
        act = k;
    } else if (q.keep && q.K > CEM_A && k == CEM_A) {
        act = q.keep[row];
    } else {
        uint32_t w[CEM_A];
        const uint32_t S = cem_load_row(q.weights + row * CEM_A, w);
        const PhiloxBlock b = philox_block(q.seed, q.offset >> 2, (uint64_t)idx);
        const unsigned word = (unsigned)(q.offset & 3);      // (uniform)
        const uint32_t x = word == 0 ? b.w[0] : word == 1 ? b.w[1] : word == 2 ? b.w[2] : b.w[3];
        const uint32_t r = (uint32_t)(((uint64_t)x * S) >> 32);
        uint32_t cum = 0;
        act = 0;      // the least a with r < w[0] + .. + w[a] = the number of sums r has reached; r < S, so the last needs no compare
#pragma unroll
        for (int a = 0; a < CEM_A - 1; ++a) {
            cum += w[a];
            act += r >= cum ? 1 : 0;
        }
    }
    q.table[idx] = (uint8_t)act;
}

struct CemRefit {
    uint32_t* __restrict__ weights;           // [M][H][9], in place
    const double* __restrict__ ret;           // [M][K]
    const uint8_t* __restrict__ table;        // [M][H][K]
    const uint8_t* __restrict__ active;       // [M], or nullptr
    uint8_t* __restrict__ best_seq;           // [M][H], or nullptr
    int H, K, E, shift;
    uint32_t w_min;
};

// K24's LDS, one block: the K keys, each wave's best key; the radix histogram, the elite counts [H][9], each wave's best k and tie
// count, the selected bin and rank; the elite flags.  The host sizes the launch with bytes().
struct CemLds {
    int K, H;
    __host__ __device__ size_t key() const { return 0; }                                            // uint64 [K]
    __host__ __device__ size_t wave_key() const { return 8 * (size_t)K; }                           // uint64 [4]
    __host__ __device__ size_t hist() const { return wave_key() + 32; }                             // uint32 [256]
    __host__ __device__ size_t count() const { return hist() + 1024; }                              // uint32 [H * 9]
    __host__ __device__ size_t wave_k() const { return count() + 4 * (size_t)H * CEM_A; }           // uint32 [4]
    __host__ __device__ size_t wave_ties() const { return wave_k() + 16; }                          // uint32 [4]
    __host__ __device__ size_t sel() const { return wave_ties() + 16; }                             // uint32 [2]
    __host__ __device__ size_t elite() const { return sel() + 8; }                                  // uint8 [K]
    __host__ __device__ size_t bytes() const { return elite() + (size_t)K; }                        // <= 47 KB at K = 4096, H = 256
};

// float64 -> a uint64 that orders as the value does (a larger value, a larger key); -0.0 takes 0.0's key.  NaN is not a return.
__device__ __forceinline__ uint64_t cem_key(double v) {
    if (v == 0.0) v = 0.0;
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

extern __shared__ uint64_t cem_lds[];

// K24.  One workgroup per state (64 threads up to K = 256, else 256).  The E-th key of the order "value descending, then k ascending"
// by eight 8-bit radix passes over the keys in LDS, from the top byte down: each pass histograms the byte of the keys that still
// match the prefix, wave 0 scans the 256 bins from the top and picks the bin the wanted rank falls in.  What is left of the rank after
// the last pass is how many of the keys EQUAL to the threshold are elites: the first ones in k order, by a prefix count.  Then the elite
// counts per (step, action) -- a ballot per action and one LDS add per (wave, step chunk, action) --, the weights, the rank-0 column.
__global__ __launch_bounds__(256) void cem_refit_kernel(const CemRefit q) {
    const int64_t m = blockIdx.x;
    if (q.active && q.active[m] == 0) return;      // (the whole workgroup)
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = T >> 6;
    const int K = q.K, H = q.H;
    const CemLds at{K, H};
    unsigned char* lds = reinterpret_cast<unsigned char*>(cem_lds);
    uint64_t* key = reinterpret_cast<uint64_t*>(lds + at.key());
    uint64_t* wave_key = reinterpret_cast<uint64_t*>(lds + at.wave_key());
    uint32_t* hist = reinterpret_cast<uint32_t*>(lds + at.hist());
    uint32_t* count = reinterpret_cast<uint32_t*>(lds + at.count());
    uint32_t* wave_k = reinterpret_cast<uint32_t*>(lds + at.wave_k());
    uint32_t* wave_ties = reinterpret_cast<uint32_t*>(lds + at.wave_ties());
    uint32_t* sel = reinterpret_cast<uint32_t*>(lds + at.sel());
    uint8_t* elite = lds + at.elite();
    const double* __restrict__ ret = q.ret + m * K;
    const uint8_t* __restrict__ tab = q.table + m * H * K;

    // the keys; rank 0 = the largest key, the lowest k among its holders (a thread meets its k in ascending order)
    uint64_t bkey = 0;
    uint32_t bk = 0xFFFFFFFFu;
    for (int k = tid; k < K; k += T) {
        const uint64_t x = cem_key(ret[k]);
        key[k] = x;
        if (bk == 0xFFFFFFFFu || x > bkey) {
            bkey = x;
            bk = (uint32_t)k;
        }
    }
    for (int i = tid; i < H * CEM_A; i += T) count[i] = 0;
    for (int s = 1; s < 64; s <<= 1) {
        const uint64_t ok = __shfl_xor((unsigned long long)bkey, s, 64);
        const uint32_t oi = __shfl_xor(bk, s, 64);
        if (oi != 0xFFFFFFFFu && (bk == 0xFFFFFFFFu || ok > bkey || (ok == bkey && oi < bk))) {
            bkey = ok;
            bk = oi;
        }
    }
    if (lane == 0) {
        wave_key[wave] = bkey;
        wave_k[wave] = bk;
    }

    // the E-th key
    uint64_t prefix = 0, mask = 0;
    uint32_t remaining = (uint32_t)q.E;      // 1 .. the number of keys that match the prefix
#pragma unroll 1
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += T) hist[i] = 0;
        __syncthreads();
        for (int k = tid; k < K; k += T) {
            const uint64_t x = key[k];
            if ((x & mask) == prefix) atomicAdd(&hist[(uint32_t)(x >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (wave == 0) {      // lane l: bins 255 - 4 l down to 252 - 4 l
            const int hi = 255 - 4 * lane;
            const uint32_t h0 = hist[hi], h1 = hist[hi - 1], h2 = hist[hi - 2], h3 = hist[hi - 3];
            const uint32_t sum = h0 + h1 + h2 + h3;
            uint32_t incl = sum;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d, 64);
                if (lane >= d) incl += o;
            }
            const uint32_t excl = incl - sum;
            if (excl < remaining && remaining <= incl) {      // exactly one lane
                uint32_t r = remaining - excl;
                int b = hi;
                if (r > h0) {
                    r -= h0; b = hi - 1;
                    if (r > h1) {
                        r -= h1; b = hi - 2;
                        if (r > h2) { r -= h2; b = hi - 3; }
                    }
                }
                sel[0] = (uint32_t)b;
                sel[1] = r;
            }
        }
        __syncthreads();
        prefix |= (uint64_t)sel[0] << shift;
        mask |= (uint64_t)0xFF << shift;
        remaining = sel[1];
    }
    // (every thread holds the threshold key in `prefix` and the number of its holders that are elites in `remaining`)

    // the elites: above the threshold, or at it and among the first `remaining` in k order.  Thread i owns k = i * chunk ..
    const int chunk = (K + T - 1) / T;
    const int k0 = tid * chunk, k1 = k0 + chunk < K ? k0 + chunk : K;
    uint32_t ties = 0;
    for (int k = k0; k < k1; ++k) ties += key[k] == prefix ? 1u : 0u;
    uint32_t incl = ties;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wave_ties[wave] = incl;
    __syncthreads();
    uint32_t before = incl - ties;
    for (int w = 0; w < wave; ++w) before += wave_ties[w];
    for (int k = k0; k < k1; ++k) {
        const uint64_t x = key[k];
        uint8_t e = x > prefix ? 1 : 0;
        if (x == prefix) e = before++ < remaining ? 1 : 0;
        elite[k] = e;
    }
    bkey = 0;
    bk = 0xFFFFFFFFu;
    for (int w = 0; w < nw; ++w) {      // rank 0 over the waves (their k ranges interleave: compare k too)
        const uint64_t ok = wave_key[w];
        const uint32_t oi = wave_k[w];
        if (oi != 0xFFFFFFFFu && (bk == 0xFFFFFFFFu || ok > bkey || (ok == bkey && oi < bk))) {
            bkey = ok;
            bk = oi;
        }
    }
    __syncthreads();

    // c[t][a]: a wave takes 64 consecutive k of one step at a time
    const int per_step = (K + 63) >> 6;
#pragma unroll 1
    for (int j = wave; j < H * per_step; j += nw) {
        const int t = j / per_step;
        const int k = ((j - t * per_step) << 6) + lane;
        const bool el = k < K && elite[k] != 0;
        const int a = el ? seq_action(tab[(int64_t)t * K + k]) : 0;
        uint32_t mine = 0;
#pragma unroll
        for (int b = 0; b < CEM_A; ++b) {
            const uint64_t votes = __ballot(el && a == b);
            if (lane == b) mine = (uint32_t)__popcll(votes);
        }
        if (lane < CEM_A && mine != 0) atomicAdd(&count[t * CEM_A + lane], mine);
    }
    __syncthreads();

    // the weights, a step per thread; the rank-0 column
    for (int t = tid; t < H; t += T) {
        uint32_t* row = q.weights + (m * H + t) * CEM_A;
        uint32_t w[CEM_A];
        cem_load_row(row, w);
#pragma unroll
        for (int a = 0; a < CEM_A; ++a) {
            const uint32_t f = (count[t * CEM_A + a] << 16) / (uint32_t)q.E;      // count <= E <= 4096
            uint32_t v = w[a] - (w[a] >> q.shift) + (f >> q.shift);
            v = v < q.w_min ? q.w_min : v;
            row[a] = v > CEM_W_MAX ? CEM_W_MAX : v;
        }
        if (q.best_seq) q.best_seq[m * H + t] = tab[(int64_t)t * K + bk];
    }
}
