// sequences.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K22 sequences_kernel: what K action sequences of H steps earn from each of M states (pc_env_rollout_sequences for states the caller
// names, pc_env_rollout_sequences_state for the handle's current state), and sequences_best_kernel, the row's best sequence.  One lane
// per (state, sequence), the state in registers from the first step to the last: no observation, nothing stored but the lane's totals.
// A step is CarEnv.step without auto-reset as step_pose (K20) has it, minus the observation: gate_fires at the OLD pose and heading,
// then crash_step (K21) -- car_move and check_collision's rays at the NEW pose --, then step_books (car_step.hpp).  Nothing is stepped for
// good: the inputs and the handle's env state are only read.
#pragma once

// The states (PoseRows, car_step.hpp), the action tables and the outputs of one call.
struct Sequences : PoseRows {
    const uint8_t* __restrict__ actions;      // [H][K] time-major, shared (state_stride 0) or one table per state (state_stride H * K)
    int64_t state_stride;
    int K, H;
    double reward_scale;
    double* __restrict__ ret;                 // [M][K]
    int32_t* __restrict__ steps;
    uint8_t* __restrict__ status;
    int32_t* __restrict__ gates;              // or nullptr
    int32_t* __restrict__ laps;               // or nullptr
    int32_t* __restrict__ best_k;             // [M], each or nullptr
    int64_t* __restrict__ best_action;
    double* __restrict__ best_ret;
};

__device__ __forceinline__ int seq_action(const uint8_t a) { return a > 8 ? 8 : (int)a; }      // anything outside 0 .. 8 acts as 8

// Lane i: state m = i / K under sequence k = i % K.  A lane whose episode ended -- terminated or truncated -- is frozen: it takes no
// further step and adds nothing; the wave runs on until its last live lane reaches H.  One body pass per distinct track id present in the
// wave (for_each_track, car_step.hpp): a lane past the end, an inactive row and an unknown track are folded into `known`.
template <typename T>
__global__ __launch_bounds__(256) void sequences_kernel(const EnvParams<T> p, const Sequences q) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < q.M * q.K;
    const int64_t m = valid ? i / q.K : 0;
    const int k = (int)(i - m * q.K);
    const bool state = q.px == nullptr;      // (uniform)
    CarRegs st = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
    int next = 0, trk = 0;
    bool act = false;
    if (valid) load_pose<T>(p, q, state, m, st, next, trk, act);
    const bool known = act & (trk < q.n_tracks);
    if (act & !known) {      // a track the handle does not have: nothing rolled out
        q.ret[i] = 0.0;
        q.steps[i] = 0;
        q.status[i] = PC_FIRST_RUNNING;
        if (q.gates) q.gates[i] = 0;
        if (q.laps) q.laps[i] = 0;
    }
    for_each_track(known, trk, [&](const int cur) {
        const TrackHdr hc = cload(p.hdr + cur);
        if (!state) resolve_turns<T>(p, hc, cur, q.turn_row, st);
        const uint8_t* __restrict__ tab = q.actions + m * q.state_stride + k;
        double ret = 0.0;
        int status = PC_FIRST_RUNNING, t = 0, gates = 0, laps = 0;
#pragma unroll 1
        while (t < q.H && status == PC_FIRST_RUNNING) {
            const int a = seq_action(tab[(int64_t)t * q.K]);
            const bool gate_hit = gate_fires<T>(p, hc, st, next, 0, 1);      // the OLD pose and heading
            CarAction did;
            const int r = crash_step<T>(p, hc, st, a, did);
            const StepBooks b = step_books(did.fwd, gate_hit, r == PC_CRASH_TERMINATED, st.time, next, hc.G, q.reward_scale);
            next = b.next;
            gates += b.gate ? 1 : 0;
            laps += b.lap ? 1 : 0;
            if (b.term) status = PC_FIRST_TERMINATED;
            else if (b.trunc) status = PC_FIRST_TRUNCATED;
            ret += (double)b.reward;      // the float32 reward, widened again
            ++t;
        }
        q.ret[i] = ret;
        q.steps[i] = t;
        q.status[i] = (uint8_t)status;
        if (q.gates) q.gates[i] = gates;
        if (q.laps) q.laps[i] = laps;
    });
}

// The best sequence of each state: one wave per row m (4 rows per workgroup), lane l scans k = l, l + 64, ... and keeps its first
// maximum; the wave then keeps the LOWEST k among the lanes that hold the row's maximum, compared as float64.  Launched after
// sequences_kernel on the same stream, it reads what that kernel stored.  An inactive row is not written; a row on a track the handle
// does not have holds K zeros and reports (0, 8, 0).
__global__ __launch_bounds__(256) void sequences_best_kernel(const Sequences q, const uint8_t* __restrict__ handle_track_id) {
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= q.M) return;      // (whole waves)
    const bool state = q.px == nullptr;
    if (!state && q.active && q.active[m] == 0) return;
    const uint8_t* tid = state ? handle_track_id : q.track_id;
    const int trk = tid ? tid[m] : 0;
    const double* __restrict__ row = q.ret + m * q.K;
    double best = 0.0;
    int at = INT_MAX;
    for (int k = lane; k < q.K; k += 64) {
        const double v = row[k];
        if (at == INT_MAX || v > best) {
            best = v;
            at = k;
        }
    }
    for (int s = 1; s < 64; s <<= 1) {
        const double ob = __hiloint2double(__shfl_xor(__double2hiint(best), s, 64), __shfl_xor(__double2loint(best), s, 64));
        const int oa = __shfl_xor(at, s, 64);
        if (oa != INT_MAX && (at == INT_MAX || ob > best || (ob == best && oa < at))) {
            best = ob;
            at = oa;
        }
    }
    if (lane == 0) {
        const bool unknown = trk >= q.n_tracks;
        if (q.best_k) q.best_k[m] = at;
        if (q.best_action) q.best_action[m] = unknown ? 8 : seq_action(q.actions[m * q.state_stride + at]);
        if (q.best_ret) q.best_ret[m] = best;
    }
}
