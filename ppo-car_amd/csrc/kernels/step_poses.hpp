// step_poses.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K20 step_poses_kernel: one CarEnv.step (car_env.py:693-760) of M caller-supplied states on the handle's tracks
// (pc_env_step_poses).  No auto-reset; the handle's own env state is neither read nor written.  The move, the gate test and the
// bookkeeping are car_step.hpp's car_move, gate_fires and step_books; the observation and the wall test at the new pose are
// observe_pose<T> (observe.hpp), whose exhaustive float64 scan takes poses from anywhere.
#pragma once

// The rows of one pc_env_step_poses call: PoseRows in its read-and-written form (car_step.hpp; every state array is required), the
// actions and the outputs.
struct StepPoses : PoseRowsT<true> {
    const int64_t* actions;        // anything outside 0 .. 8 acts as 8 (no thrust, no turn)
    float* reward;
    uint8_t* terminated;
    uint8_t* truncated;
    uint8_t* gate;                 // or nullptr
    double reward_scale;
    int lg;                        // log2(lanes per row)
};

// One CarEnv.step of the row in (st, next) on track `trk` (the same in every active lane), by the 2^lg lanes of its group; every lane
// leaves with the same new state and the same books except `term`, which lane 0 of the group holds (observe_pose reports to that lane).
template <typename T>
__device__ __forceinline__ StepBooks step_pose(const EnvParams<T>& p, const int trk, const int g, const int lg, CarRegs& st, const int next,
                                               const int64_t a, const double reward_scale, float* __restrict__ orow, CarAction& did) {
    const TrackHdr h = cload(p.hdr + __builtin_amdgcn_readfirstlane(trk));
    const int G = 1 << lg;
    // ---- Car.get_passed_gate at the OLD pose with the OLD heading, its rays dealt round-robin to the row's lanes
    int flag = gate_fires<T>(p, h, st, next, g, G) ? 1 : 0;      // any() over the row's lanes (every lane of a group is here: they share the row)
    for (int m = 1; m < G; m <<= 1) flag |= __shfl_xor(flag, m, 64);
    const bool gate_hit = flag != 0;
    const int time = st.time + 1;  // :745
    st = car_move<T>(p, h, st, a, did);
    st.time = time;
    // ---- the observation CarEnv.step returns, and Car.check_collision, at the NEW pose (lane 0 of the group receives `collides`)
    uint8_t collides = 0;
    observe_pose<T>(p, trk, g, lg, st.px, st.py, st.vx, st.vy, st.k, st.rot, orow, &collides);
    return step_books(did.fwd, gate_hit, (collides != 0) | (h.start_collides != 0), time, next, h.G, reward_scale);
}

// Row m of `q` by 2^lg lanes, 256 threads; one body pass per distinct track id present in a wave (for_each_track, car_step.hpp).  A row
// that is not stepped -- active[m] == 0, or a track the handle does not have -- is folded into `known` instead of leaving early; the only
// exit before the waterfall is the bound on m, which whole groups take together.
template <typename T>
__global__ __launch_bounds__(256) void step_poses_kernel(const EnvParams<T> p, const StepPoses q, float* __restrict__ obs) {
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = lane >> q.lg;
    const int g = (int)(lane & ((1 << q.lg) - 1));
    if (m >= q.M) return;
    // every lane of the group loads the row; lane 0 stores it at the very end
    CarRegs st;
    int next, trk;
    bool act;
    load_pose<T>(p, q, false, m, st, next, trk, act);
    const int turns = st.k;
    const int64_t a = q.actions[m];
    float* __restrict__ orow = obs + (size_t)m * p.D;
    const bool known = act & (trk < q.n_tracks);
    if (act & !known) {      // a track the handle does not have: a row of zeros, reward and flags 0, the state as it is
        for (int i = g; i < p.D; i += 1 << q.lg) orow[i] = 0.0f;
        if (g == 0) {
            q.reward[m] = 0.0f;
            q.terminated[m] = 0;
            q.truncated[m] = 0;
            if (q.gate) q.gate[m] = 0;
        }
    }
    for_each_track(known, trk, [&](const int cur) {
        resolve_turns<T>(p, cload(p.hdr + cur), cur, q.turn_row, st);
        CarAction did;
        const StepBooks b = step_pose<T>(p, cur, g, q.lg, st, next, a, q.reward_scale, orow, did);
        if (g == 0) {
            q.px[m] = st.px; q.py[m] = st.py; q.vx[m] = st.vx; q.vy[m] = st.vy;
            q.turns[m] = turns + did.turn;      // (on F64 handles st.k is a table row: the count moves with the action)
            q.next_gate[m] = b.next;
            q.time_step[m] = st.time;
            q.reward[m] = b.reward;
            q.terminated[m] = b.term ? 1 : 0;
            q.truncated[m] = b.trunc ? 1 : 0;
            if (q.gate) q.gate[m] = b.gate ? 1 : 0;
        }
    });
}
