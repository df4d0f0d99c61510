// sequences_value.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K25 sequences_value_kernel and K26 sequences_combine_kernel: K22 (sequences.hpp) with a discount, the observation of the state a sequence
// ends in, and the critic's value of that state folded into the score (pc_env_rollout_sequences_value for states the caller names,
// pc_env_rollout_sequences_value_state for the handle's current state).  Between the two launches the call runs the policy step
// (pc_policy_act_greedy's launch, unmodified) once over end_obs viewed as M * K rows.
//   K25  one lane per (state, sequence) as K22: the same step -- gate_fires, crash_step, step_books, once each --, the discounted sum in
//        separately rounded float64 operations, and after the loop ONE observe_pose<T> of the lane's registers, by the lane alone
//        (2^0 lanes per pose): the bits K17 / K20 give that pose.
//   K26  one wave per state as sequences_best_kernel: ret = ret_env + end_discount * (double)end_value where the mode bootstraps the
//        lane's status, then the row's best sequence on that ret.
#pragma once

// What the call adds to K22's arguments.
struct SequencesValue : Sequences {
    double gamma;
    int bootstrap;                            // PC_SEQ_BOOTSTRAP_*
    float* __restrict__ end_obs;              // [M][K][D] or nullptr
    const float* __restrict__ end_value;      // [M][K] or nullptr: no policy
    double* __restrict__ end_discount;        // [M][K] or nullptr
    double* __restrict__ ret_env;             // [M][K] or nullptr
};

// Lane i: state m = i / K under sequence k = i % K, K22's lane and K22's loop.  ret[i] receives ret_env: K26 adds the bootstrap in place.
template <typename T>
__global__ __launch_bounds__(256) void sequences_value_kernel(const EnvParams<T> p, const SequencesValue q) {
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
    float* __restrict__ orow = q.end_obs ? q.end_obs + (size_t)i * p.D : nullptr;
    if (act & !known) {      // a track the handle does not have: nothing rolled out, nothing to bootstrap from
        q.ret[i] = 0.0;
        q.steps[i] = 0;
        q.status[i] = PC_FIRST_RUNNING;
        if (q.gates) q.gates[i] = 0;
        if (q.laps) q.laps[i] = 0;
        if (orow)
            for (int j = 0; j < p.D; ++j) orow[j] = 0.0f;
        if (q.end_discount) q.end_discount[i] = 1.0;
        if (q.ret_env) q.ret_env[i] = 0.0;
    }
    for_each_track(known, trk, [&](const int cur) {
        const TrackHdr hc = cload(p.hdr + cur);
        if (!state) resolve_turns<T>(p, hc, cur, q.turn_row, st);
        const uint8_t* __restrict__ tab = q.actions + m * q.state_stride + k;
        double ret = 0.0, disc = 1.0;
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
            ret = __dadd_rn(ret, __dmul_rn(disc, (double)b.reward));      // two roundings, never an fma
            disc = __dmul_rn(disc, q.gamma);
            ++t;
        }
        q.ret[i] = ret;
        q.steps[i] = t;
        q.status[i] = (uint8_t)status;
        if (q.gates) q.gates[i] = gates;
        if (q.laps) q.laps[i] = laps;
        if (q.end_discount) q.end_discount[i] = disc;
        if (q.ret_env) q.ret_env[i] = ret;
        // the observation CarEnv.step returned in the lane's last step: the pose in the registers, terminated lanes included
        if (orow) observe_pose<T>(p, cur, 0, 0, st.px, st.py, st.vx, st.vy, st.k, st.rot, orow, nullptr);
    });
}

// One wave per row m (4 rows per workgroup), after K25 and the policy step on the same stream.  Lane l takes k = l, l + 64, ...: where a
// value is given and the mode covers the lane's status, ret[m][k] becomes ret_env + end_discount * (double)end_value, stored; then
// sequences_best_kernel's scan and butterfly on the lane's own (just stored) values.  end_discount is gamma multiplied `steps` times
// into 1.0, K25's chain repeated (the array itself is optional).  A lane that took no step -- a track the handle does not have -- is
// never bootstrapped.  An inactive row is not written.
__global__ __launch_bounds__(256) void sequences_combine_kernel(const SequencesValue q, const uint8_t* __restrict__ handle_track_id) {
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= q.M) return;      // (whole waves)
    const bool state = q.px == nullptr;
    if (!state && q.active && q.active[m] == 0) return;
    const uint8_t* tid = state ? handle_track_id : q.track_id;
    const int trk = tid ? tid[m] : 0;
    double* __restrict__ row = q.ret + m * q.K;
    const bool boot = q.end_value != nullptr && q.bootstrap != PC_SEQ_BOOTSTRAP_NONE;
    double best = 0.0;
    int at = INT_MAX;
    for (int k = lane; k < q.K; k += 64) {
        double v = row[k];
        if (boot) {
            const int64_t i = m * q.K + k;
            const int status = q.status[i], steps = q.steps[i];
            const bool covered = status == PC_FIRST_RUNNING || (status == PC_FIRST_TRUNCATED && q.bootstrap == PC_SEQ_BOOTSTRAP_RUNNING_TRUNCATED);
            if (covered && steps > 0) {
                double disc = 1.0;
                for (int t = 0; t < steps; ++t) disc = __dmul_rn(disc, q.gamma);
                v = __dadd_rn(v, __dmul_rn(disc, (double)q.end_value[i]));
                row[k] = v;
            }
        }
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
