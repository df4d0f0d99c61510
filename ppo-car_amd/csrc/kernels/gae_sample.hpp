// gae_sample.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K3 gae_kernel<ADV, BOOT, EPI, STEPS> (the reverse scan: GAE and episode statistics) and K4 sample_kernel (Categorical
// sample / log_prob / entropy, Philox).
#pragma once

// ------------------------------------------------------------------------------------------
// K3: the reverse scan over the rollout buffer, gae_kernel<ADV, BOOT, EPI, STEPS>.  One lane per env, serial in t (the
// recurrence), rows coalesced across envs.  Instances (the rest are rejected by the static_asserts):
//   K3   <1,0,0,0>  GAE(lambda), buffer.py:36-64 (pc_gae)
//   K3e  <1,0,1,0>  K3 plus the episode statistics (pc_gae_episodes)
//   K3b  <1,1,0,0>  K3 with the truncation bootstrap (pc_gae_bootstrap)
//        <1,1,1,0>  K3b plus the episode statistics (pc_gae_bootstrap with carry / out)
//   K3e  <0,0,1,0>  the episode statistics alone, Buffer layout (pc_episode_stats, PC_EPISODE_BUFFER)
//        <0,0,1,1>  the same, step layout (pc_episode_stats, PC_EPISODE_STEPS)
// ADV: GAE.  Operation order = torch's, one float32 rounding per op (no FMA):
//   delta    = (rew[t] + (gamma * next_val) * term_mask) - val[t]                       :60
//   last_gae = delta + (((gamma*lambda) * term_mask) * trunc_mask) * last_gae           :61
// Every ADV instance runs these float32 operations in this order, so adv / ret are K3's bits whatever else the launch does.
// EPI: EpisodeAcc (below) on the rows already in registers -- no added HBM traffic per transition.
// BOOT: at a truncated step t -- the trunc flag in row t + 1, or last_trunc for t = T - 1 -- next_val is V(final observation) from
// final_val[t / PC_TIME_LIMIT] instead of val[t + 1] / last_val (which gymnasium's same-step auto-reset made V(reset observation));
// every float32 operation and its order stay K3's, and so does the trace cut (trunc_mask).  final_val's values are used only at
// truncated steps.  Each block of U rows loads the (at most two) slots its steps lie in together with its rows: a load per
// truncation inside the recurrence made every wave wait for its outstanding stores (1.31 x K3); these are two coalesced
// L2-resident words per env and block, issued with the rows.
// STEPS (EPI alone): false, the Buffer layout: step t's flags in row t + 1, step T - 1's in last_* (row 0's are never used);
// true: flags[t] belong to rew[t] (pc_env_step / pc_env_step_many rows), last_* are not read.
// ------------------------------------------------------------------------------------------

// Episode statistics (gymnasium's RecordEpisodeStatistics, plus gates and laps) from the rows the scan streams.
// REVERSE like K3: a boundary after step t (its terminated or truncated flag) closes the segment to its right; the right-most
// closed segment is the new carry, every other one a finished episode; the left-most segment adds the carry-in (the episode in
// progress when the window began) and finishes at the first boundary.
//   Decoding: the reward is (float)(rw * s) with rw a sum of the reference's constants (car_env.py:700-748: 0.01 forward,
//   +1 gate, +10 lap, -3 crash), so k = rint(r / s) is one of {0, 1, 11, -3, -2, 8} with a margin >= 0.49:
//   a gate iff k in {1, 11, -2, 8}, a lap iff k in {11, 8}.
//   Exactness: every float32 reward is an integer multiple of u = ulp(f32(0.01 s)) (no reward is smaller in magnitude
//   and not zero).  An episode is at most 1000 steps (car_env.py:749), so every partial sum of one episode -- and of a
//   window of T <= 1024 steps plus its carry -- stays below ~2000 * 11.01 / 0.01 * 2^24 u < 2^45 u < 2^53 u: the float64
//   sums are EXACT, in any order.  The reverse scan here and a forward numpy sum give the same bits, and the fused instances
//   (K3e, K3b with carry / out) give the standalone one's.
// Outputs (float64, structure of arrays, ACCUMULATED into what the caller initialised):
//   out[0..6][N]: finished episodes, sum of their scaled returns, of their lengths, gates, laps; min / max scaled return
//   carry[0..3][N] (in / out): return, length, gates, laps of the episode in progress; length -1 = start not observed
//   (the episode that closes from there is dropped, and the carry restarts at 0).
struct EpisodeAcc {
    double seg_ret = 0.0;               // the open segment: from the scan position to the nearest boundary on its right
    int seg_len = 0, seg_g = 0, seg_l = 0;
    bool closed = false;                // a boundary has been met: the right-most segment is already the carry-out
    double c_ret = 0.0;                 // carry-out (valid once closed)
    int c_len = 0, c_g = 0, c_l = 0;
    int n = 0, s_len = 0, s_g = 0, s_l = 0;   // finished episodes
    double s_ret = 0.0, mn = INFINITY, mx = -INFINITY;

    // step t of the reverse scan; `done`: step t ended an episode (the boundary after it)
    __device__ __forceinline__ void step(const float r, const bool done, const double inv_s) {
        const bool fin = done & closed, first = done & !closed;
        n += fin;
        s_ret += fin ? seg_ret : 0.0;
        s_len += fin ? seg_len : 0;
        s_g += fin ? seg_g : 0;
        s_l += fin ? seg_l : 0;
        mn = fin ? fmin(mn, seg_ret) : mn;
        mx = fin ? fmax(mx, seg_ret) : mx;
        c_ret = first ? seg_ret : c_ret;
        c_len = first ? seg_len : c_len;
        c_g = first ? seg_g : c_g;
        c_l = first ? seg_l : c_l;
        closed |= done;
        const int k = (int)rint((double)r * inv_s);
        seg_ret = (done ? 0.0 : seg_ret) + (double)r;    // the float64 chain: independent of K3's float32 recurrence
        seg_len = (done ? 0 : seg_len) + 1;
        seg_g = (done ? 0 : seg_g) + ((k == 1) | (k == 11) | (k == -2) | (k == 8));
        seg_l = (done ? 0 : seg_l) + ((k == 11) | (k == 8));
    }

    // the left-most segment meets the carry-in; carry and out are read once and written once
    __device__ __forceinline__ void finish(double* __restrict__ carry, double* __restrict__ out, const int64_t e, const int64_t N) {
        const double cin_len = carry[N + e];
        const bool seen = cin_len >= 0.0;
        if (seen) {
            seg_ret = carry[e] + seg_ret;
            seg_len += (int)cin_len;
            seg_g += (int)carry[2 * N + e];
            seg_l += (int)carry[3 * N + e];
        }
        if (closed) {
            if (seen) {
                n += 1;
                s_ret += seg_ret;
                s_len += seg_len;
                s_g += seg_g;
                s_l += seg_l;
                mn = fmin(mn, seg_ret);
                mx = fmax(mx, seg_ret);
            }
        } else {            // no boundary in the window: the carry goes on (a sentinel stays one)
            c_ret = seen ? seg_ret : 0.0;
            c_len = seen ? seg_len : -1;
            c_g = seen ? seg_g : 0;
            c_l = seen ? seg_l : 0;
        }
        carry[e] = c_ret;
        carry[N + e] = (double)c_len;
        carry[2 * N + e] = (double)c_g;
        carry[3 * N + e] = (double)c_l;
        out[e] += (double)n;
        out[N + e] += s_ret;
        out[2 * N + e] += (double)s_len;
        out[3 * N + e] += (double)s_g;
        out[4 * N + e] += (double)s_l;
        out[5 * N + e] = fmin(out[5 * N + e], mn);
        out[6 * N + e] = fmax(out[6 * N + e], mx);
    }
};

template <bool ADV, bool BOOT, bool EPI, bool STEPS>
__global__ __launch_bounds__(256) void gae_kernel(const float* __restrict__ rew, const float* __restrict__ val,
                                                  const float* __restrict__ term, const float* __restrict__ trunc,
                                                  const float* __restrict__ last_val, const float* __restrict__ last_term,
                                                  const float* __restrict__ last_trunc, const float g, const float gl,
                                                  const int64_t T, const int64_t N, float* __restrict__ adv,
                                                  float* __restrict__ ret, const float* __restrict__ final_val, const double inv_s,
                                                  double* __restrict__ carry, double* __restrict__ out) {
    static_assert(ADV || EPI, "the scan computes GAE, episode statistics or both");
    static_assert(!BOOT || ADV, "the truncation bootstrap changes only GAE");
    static_assert(!STEPS || !ADV, "GAE reads the Buffer layout");
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    // What step t reads from the step after it: K3's next_val and masks, and `done` (step t ended an episode; EPI, Buffer
    // layout).  The step takes and returns it by value, with done as a float 0 / 1, so the state stays out of memory until the
    // step is inlined.  That keeps K3's instructions and every instance's registers within the hand-written kernels' counts; a
    // bool member or the two flags carried as floats cost time (profiles/gae_template_refactor.txt has the counts and timings).
    struct State {
        float next_val, tmask, trmask, last_gae, done;
    } st{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (!STEPS) {
        const float lt = last_term[e], ltr = last_trunc[e];
        if constexpr (BOOT) st.next_val = ltr != 0.0f ? final_val[(T - 1) / PC_TIME_LIMIT * N + e] : last_val[e];
        else if constexpr (ADV) st.next_val = last_val[e];     // :53
        st.tmask = 1.0f - lt;                                   // :54
        st.trmask = 1.0f - ltr;                                 // :55
        st.done = ((lt != 0.0f) | (ltr != 0.0f)) ? 1.0f : 0.0f;
    }
    EpisodeAcc acc;
    // step t: its row's rew, val, term, trunc; boot() is final_val of step t - 1's slot, read only when step t - 1 truncated
    const auto step = [=, &acc](State s, const int64_t t, const float r, const float v, const float tm, const float tr,
                                const auto& boot) {
        if constexpr (EPI)
            acc.step(r, STEPS ? (tm != 0.0f) | (tr != 0.0f) : s.done != 0.0f, inv_s);
        else
            (void)acc;      // (captured for the EPI instances)
        if constexpr (ADV) {
            const int64_t off = t * N + e;
            float tmp = g * s.next_val;
            tmp = tmp * s.tmask;
            float delta = r + tmp;
            delta = delta - v;
            float c = gl * s.tmask;
            c = c * s.trmask;
            c = c * s.last_gae;
            s.last_gae = delta + c;
            adv[off] = s.last_gae;          // :62
            ret[off] = s.last_gae + v;      // :63
        }
        if constexpr (BOOT) s.next_val = (tr != 0.0f && t >= 1) ? boot() : v;
        else s.next_val = v;
        s.tmask = 1.0f - tm;
        s.trmask = 1.0f - tr;
        s.done = ((tm != 0.0f) | (tr != 0.0f)) ? 1.0f : 0.0f;
        return s;
    };
    constexpr int U = 8;  // rows in flight per lane: the loads do not depend on the recurrence
    static_assert(U - 1 <= PC_TIME_LIMIT, "the remainder rows' bootstrap reads slot 0");
    int64_t t = T - 1;
    for (; t >= U - 1; t -= U) {
        float r[U], v[U], tm[U], tr[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int64_t off = (t - j) * N + e;
            r[j] = rew[off];
            v[j] = ADV ? val[off] : 0.0f;
            tm[j] = term[off];
            tr[j] = trunc[off];
        }
        // BOOT: steps t - 1 .. t - U lie in slot sa from step sb on, in slot sa - 1 (or sa) below it
        float fa = 0.0f, fb = 0.0f;
        int64_t sb = 0;
        if constexpr (BOOT) {
            const int64_t sa = (t - 1) / PC_TIME_LIMIT;
            sb = sa * PC_TIME_LIMIT;
            fa = final_val[sa * N + e];
            fb = final_val[(t - U > 0 ? t - U : 0) / PC_TIME_LIMIT * N + e];
        }
#pragma unroll
        for (int j = 0; j < U; ++j) st = step(st, t - j, r[j], v[j], tm[j], tr[j], [&] { return t - j - 1 >= sb ? fa : fb; });
    }
    for (; t >= 0; --t) {   // t < U - 1 <= PC_TIME_LIMIT: step t - 1 lies in slot 0 (static_assert above)
        const int64_t off = t * N + e;
        st = step(st, t, rew[off], ADV ? val[off] : 0.0f, term[off], trunc[off], [&] { return final_val[e]; });
    }
    if constexpr (EPI) acc.finish(carry, out, e, N);
}

// ------------------------------------------------------------------------------------------
// K4: categorical sample / log_prob / entropy (model.py:35-40), Philox-4x32-10 counter RNG
// ------------------------------------------------------------------------------------------
// exp(x) for the rollout-time softmax, x = logit - max <= 0: v_exp_f32(x * log2(e)), two instructions.  expf() spends eight
// more per call on carrying x * log2(e) in extended precision; here the product's rounding is a relative error of
// |x| * 2^-24 in the result (1e-7 at x = -2, 1e-6 at x = -20 where the probability is 2e-9), against the 1e-5 the log-probs
// are held to and the 2e-6 they are tested at.  Nine calls per env and step: the draw was 3 % of the rollout kernel.
__device__ __forceinline__ float softmax_exp(const float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
// log and reciprocal of the softmax denominator (1 <= sum <= A): the hardware's one-instruction forms.  v_log_f32 (log2, one ulp) times
// ln 2 is within 2 ulps of log -- 2e-7 absolute on a log-sum-exp below 2.2 -- and v_rcp_f32 within one ulp of 1 / sum; the IEEE division
// and the full-range logf they replace cost 16 more vector instructions per draw for bits the sampler's contract (log-prob within 2e-6 of
// Categorical, model.py:34-41) does not ask for.  EVERY draw of the library goes through these two (pc_sample, the fused policy step in
// all its forms, the persistent kernels): their buffers stay bit-identical to each other.
__device__ __forceinline__ float softmax_log(const float sum) { return __builtin_amdgcn_logf(sum) * 0.693147180559945309417f; }
__device__ __forceinline__ float softmax_rcp(const float sum) { return __builtin_amdgcn_rcpf(sum); }

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
}

// The stream: draw number `offset` of element `idx` is word (offset & 3) of the Philox block with counter
// (idx, offset >> 2) and key `seed` -- all four words of a block are used, so a kernel that walks consecutive
// offsets (the persistent rollout) runs the ten rounds once per four draws.
struct PhiloxBlock { uint32_t w[4]; };
struct NoPhilox {};     // what stands in the block's place in a kernel's greedy instance: no registers
__device__ __forceinline__ PhiloxBlock philox_block(uint64_t seed, uint64_t block, uint64_t idx) {
    uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)block, (uint32_t)(block >> 32)};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return PhiloxBlock{{c[0], c[1], c[2], c[3]}};
}
__device__ __forceinline__ float philox_word_uniform(const PhiloxBlock& b, const unsigned word) {  // word: wave-uniform
    const uint32_t x = word == 0 ? b.w[0] : word == 1 ? b.w[1] : word == 2 ? b.w[2] : b.w[3];
    // (0, 1) open, from the word's top 24 bits k: u = ((float)k + 0.5f) * 2^-24 in float32 (include/ppocar.h states it so).  k + 0.5 is
    // not a float32 from k = 2^23 on (it rounds to even), and for k = 2^24 - 1 it rounds UP to 2^24: unbounded, that one word in 2^24
    // gave u == 1.0f, which passes every bin of the inverse CDF and returned the last action whatever its probability.  The bound is
    // the largest float32 below 1; it changes that word's uniform and no other, so every other draw of every seeded run keeps its bits.
    // Written as ONE fused multiply-add -- fma(k, 2^-24, 2^-25) rounds the exact (k + 0.5) 2^-24 once, and scaling by a power of two
    // commutes with rounding: the same bits as add-then-multiply for every k (tests/test_policy_draw_host.py walks all 2^24) -- so
    // that convert, fma, min are the three instructions convert, add, multiply were: with the minimum appended to the old pair the
    // persistent rollout launch measured 2.5 % slower, in this form it equals the parent (profiles/uniform_bound_ab.txt).
    return fminf(__builtin_fmaf((float)(x >> 8), 1.0f / 16777216.0f, 1.0f / 33554432.0f), 0x1.fffffep-1f);
}
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint64_t offset, uint64_t idx) {
    return philox_word_uniform(philox_block(seed, offset >> 2, idx), (unsigned)(offset & 3));
}

template <int AMAX>
__global__ __launch_bounds__(256) void sample_kernel(const float* __restrict__ logits, const int64_t N, const int A,
                                                     const uint64_t seed, const uint64_t offset,
                                                     int64_t* __restrict__ actions, float* __restrict__ logprob,
                                                     float* __restrict__ entropy) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    float l[AMAX];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < AMAX; ++i) {
        l[i] = i < A ? logits[e * A + i] : -INFINITY;
        mx = fmaxf(mx, l[i]);
    }
    float ex[AMAX];
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < AMAX; ++i) {
        if (i >= A) break;
        ex[i] = softmax_exp(l[i] - mx);
        sum += ex[i];
    }
    const float lse = mx + softmax_log(sum);  // Categorical(logits=...) normalises: logits - logsumexp
    const float inv = softmax_rcp(sum);
    const float u = philox_uniform(seed, offset, (uint64_t)e);
    float cum = 0.0f, ent = 0.0f, lp = 0.0f;
    int act = -1;
#pragma unroll
    for (int i = 0; i < AMAX; ++i) {
        if (i >= A) break;
        const float nl = l[i] - lse;
        const float pr = ex[i] * inv;                        // same draw as policy_tail (the fused policy step)
        cum += pr;
        ent -= pr * fmaxf(nl, -3.4028234663852886e38f);  // torch clamps log-probs at finfo.min
        if (act < 0 && (u < cum || i == A - 1)) {        // inverse CDF; last bin absorbs rounding
            act = i;
            lp = nl;
        }
    }
    actions[e] = act;
    logprob[e] = lp;
    if (entropy) entropy[e] = ent;
}
