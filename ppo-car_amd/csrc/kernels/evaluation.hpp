// evaluation.hpp -- part of the single translation unit ppocar.hip (included there after gae_sample.hpp; not a stand-alone header).
// The two kernels of the batched evaluation (ppo_car_amd.Evaluator): K14 first_episodes_kernel<STEPS>, the forward scan that keeps each
// env's FIRST episode and times its laps (pc_first_episodes), and K15 greedy_kernel, the argmax sibling of K4 (pc_greedy).
#pragma once

// ------------------------------------------------------------------------------------------
// K14: the first episode of every env, forward in t.  One lane per env, rows coalesced across envs, U rows in flight per lane (the
// loads do not depend on the recurrence: K3's decomposition, run the other way).  A pure streaming kernel: 12 bytes per env and step
// in, 64 bytes per env out, a few float64 operations per step.
//   state [PC_FIRST_ROWS][N] float64, in / out (the caller initialises rows 0-5 to 0 and rows 6-7 to +inf):
//     0 return (the float64 sum of the float32 scaled rewards: EXACT by EpisodeAcc's argument, an episode has <= 1000 steps, so the
//       bits are a numpy forward sum's and do not depend on how the steps are cut into windows)   1 length   2 gates   3 laps
//     4 status (PC_FIRST_RUNNING / _TERMINATED / _TRUNCATED; both flags on the closing step = terminated)
//     5 the episode step count at the last lap close (0 = no lap yet): the sum of the lap times
//     6 best lap in steps (the steps between consecutive lap closes, the first lap from the episode's start; +inf = none)
//     7 first lap in steps (+inf = none)
//   Every count is a small integer held exactly in a float64, so the state written by one call is read back bit for bit by the next:
//   one call over T rows == any split of the rows into consecutive calls.
// An env whose status is not RUNNING on entry is left untouched (its lane returns before any load); after the step that closes the
// episode the rest of the window is ignored.  Rewards are decoded by EpisodeAcc::step itself (the open segment of an accumulator that
// never meets a boundary is the forward sum).
// STEPS: false, the Buffer layout: step t's flags in row t + 1, step T - 1's in last_* (row 0's are never read); true: flags[t]
// belong to rew[t], last_* are not read.
// ------------------------------------------------------------------------------------------
template <bool STEPS>
__global__ __launch_bounds__(256) void first_episodes_kernel(const float* __restrict__ rew, const float* __restrict__ term,
                                                             const float* __restrict__ trunc, const float* __restrict__ last_term,
                                                             const float* __restrict__ last_trunc, const int64_t T, const int64_t N,
                                                             const double inv_s, double* __restrict__ state) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    if (state[4 * N + e] != (double)PC_FIRST_RUNNING) return;
    EpisodeAcc acc;
    acc.seg_ret = state[e];
    acc.seg_len = (int)state[N + e];
    acc.seg_g = (int)state[2 * N + e];
    acc.seg_l = (int)state[3 * N + e];
    int status = PC_FIRST_RUNNING;
    int lap_close = (int)state[5 * N + e];
    double best = state[6 * N + e], first = state[7 * N + e];
    // the flags of step t (t + 1 < T is uniform: no divergence)
    const auto flag = [=](const float* rows, const float* last, const int64_t t) {
        if constexpr (STEPS) return rows[t * N + e];
        else return t + 1 < T ? rows[(t + 1) * N + e] : last[e];
    };
    const auto step = [&](const float r, const float tm, const float tr) {
        if (status != PC_FIRST_RUNNING) return;
        const int laps = acc.seg_l;
        acc.step(r, false, inv_s);
        if (acc.seg_l != laps) {            // this step closed a lap
            const double lap = (double)(acc.seg_len - lap_close);
            best = fmin(best, lap);
            first = laps == 0 ? lap : first;
            lap_close = acc.seg_len;
        }
        status = tm != 0.0f ? PC_FIRST_TERMINATED : (tr != 0.0f ? PC_FIRST_TRUNCATED : PC_FIRST_RUNNING);
    };
    constexpr int U = 8;  // rows in flight per lane
    int64_t t = 0;
    for (; t + U <= T && status == PC_FIRST_RUNNING; t += U) {
        float r[U], tm[U], tr[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            r[j] = rew[(t + j) * N + e];
            tm[j] = flag(term, last_term, t + j);
            tr[j] = flag(trunc, last_trunc, t + j);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) step(r[j], tm[j], tr[j]);
    }
    for (; t < T && status == PC_FIRST_RUNNING; ++t) step(rew[t * N + e], flag(term, last_term, t), flag(trunc, last_trunc, t));
    state[e] = acc.seg_ret;
    state[N + e] = (double)acc.seg_len;
    state[2 * N + e] = (double)acc.seg_g;
    state[3 * N + e] = (double)acc.seg_l;
    state[4 * N + e] = (double)status;
    state[5 * N + e] = (double)lap_close;
    state[6 * N + e] = best;
    state[7 * N + e] = first;
}

// ------------------------------------------------------------------------------------------
// K15: the deterministic sibling of K4: action = the FIRST index of the row's maximum (torch.argmax's tie rule), log_prob =
// log_softmax(logits)[action] formed as K4 forms it (softmax_exp / softmax_log: the same bits as K4's log-prob of that action).
// One lane per row; action_f32 (the float copy) and logprob may be NULL.  Logits are finite.
// ------------------------------------------------------------------------------------------
template <int AMAX>
__global__ __launch_bounds__(256) void greedy_kernel(const float* __restrict__ logits, const int64_t N, const int A,
                                                     int64_t* __restrict__ actions, float* __restrict__ action_f32,
                                                     float* __restrict__ logprob) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    float l[AMAX];
    float mx = -INFINITY;
    int act = 0;
#pragma unroll
    for (int i = 0; i < AMAX; ++i) {
        l[i] = i < A ? logits[e * A + i] : -INFINITY;
        if (l[i] > mx) {                    // strict: the first maximum wins
            mx = l[i];
            act = i;
        }
    }
    actions[e] = act;
    if (action_f32) action_f32[e] = (float)act;
    if (logprob) {
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < AMAX; ++i) {
            if (i >= A) break;
            sum += softmax_exp(l[i] - mx);
        }
        logprob[e] = mx - (mx + softmax_log(sum));      // l[act] - logsumexp, l[act] == mx
    }
}
