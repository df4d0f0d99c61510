// sequences.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K22 sequences_kernel: what K action sequences of H steps earn from each of M states (pc_env_rollout_sequences for states the caller
// names, pc_env_rollout_sequences_state for the handle's current state), and sequences_best_kernel, the row's best sequence.  One lane
// per (state, sequence), the state in registers from the first step to the last: no observation, nothing stored but the lane's totals.
// A step is CarEnv.step without auto-reset as step_pose (K20) defines it, minus the observation: the gate test at the OLD pose and
// heading, then crash_step (K21) -- the action translation, Car.update and check_collision's rays at the NEW pose --, then K20's
// bookkeeping.  Nothing is stepped for good: the inputs and the handle's env state are only read.
#pragma once

// The states, the action tables and the outputs of one call.  px == nullptr: the STATE form, the handle's own envs (M = its env count).
struct Sequences {
    const double* __restrict__ px;
    const double* __restrict__ py;
    const double* __restrict__ vx;
    const double* __restrict__ vy;
    const int32_t* __restrict__ turns;        // heading = the track's start angle + 5 degrees * turns (ObservePoses' rule)
    const int32_t* __restrict__ next_gate;    // or nullptr: 0
    const int32_t* __restrict__ time_step;    // or nullptr: 0
    const uint8_t* __restrict__ track_id;     // or nullptr: track 0
    const uint8_t* __restrict__ active;       // or nullptr: every row
    const int* __restrict__ turn_row;         // F64 handles: ObservePoses::turn_row
    const uint8_t* __restrict__ actions;      // [H][K] time-major, shared (state_stride 0) or one table per state (state_stride H * K)
    int64_t state_stride;
    int64_t M;
    int K, H;
    int n_tracks;
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

// Car.get_passed_gate (car_env.py:394-408) by ONE lane: the collision rays j * (n // 4), j < nc, at the pose and heading in `st` against
// gate[next] only, step_pose's casts per dtype.  A next_gate outside 0 .. G - 1: no gate to test.
template <typename T>
__device__ __forceinline__ bool gate_fires(const EnvParams<T>& p, const TrackHdr& h, const SearchRegs& st, const int next) {
    if ((next < 0) | (next >= h.G)) return false;
    const Seg gate = p.segs[h.gate_off + next];
    bool fired = false;
#pragma unroll 1
    for (int j = 0; j < p.nc; ++j) {
        const int ray = j * p.q;
        if constexpr (sizeof(T) == 4) {      // cast_d on the float64 lattice, as env_step_core casts it
            const double2 cs = p.dirtab64[h.dir_off + Math<float>::dir_index(p, st.k, ray)];
            fired |= cast_d(gate, st.px, st.py, cs.x, cs.y) < 10.0;      // :387,:390
        } else {                             // the reference's own cast on the old rotation's ray
            double dx, dy;
            Math<double>::ray_dir(p, h, ray, st.k, st.rot, dx, dy);
            fired |= Math<double>::cast(gate, st.px, st.py, dx, dy) < 10.0;
        }
    }
    return fired;
}

// Lane i: state m = i / K under sequence k = i % K.  A lane whose episode ended -- terminated or truncated -- is frozen: it takes no
// further step and adds nothing; the wave runs on until its last live lane reaches H.  Tracks: observe_kernel's waterfall, one body
// pass per distinct track id present in the wave.  No lane leaves before the ballot: a lane past the end, an inactive row and an
// unknown track are folded into `known`.
template <typename T>
__global__ __launch_bounds__(256) void sequences_kernel(const EnvParams<T> p, const Sequences q) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < q.M * q.K;
    const int64_t m = valid ? i / q.K : 0;
    const int k = (int)(i - m * q.K);
    const bool state = q.px == nullptr;      // (uniform)
    SearchRegs st = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
    int next = 0, trk = 0;
    bool act = valid;
    if (valid) {
        if (state) {
            const EnvRegs e = env_load<T>(p, m);
            st.px = e.px; st.py = e.py; st.vx = e.vx; st.vy = e.vy; st.rot = e.rot;
            st.k = e.k;
            st.time = e.time;
            next = e.next;
            trk = p.track_id ? p.track_id[m] : 0;
        } else {
            st.px = q.px[m]; st.py = q.py[m]; st.vx = q.vx[m]; st.vy = q.vy[m];
            st.k = q.turns[m];
            st.time = q.time_step ? q.time_step[m] : 0;
            next = q.next_gate ? q.next_gate[m] : 0;
            trk = q.track_id ? q.track_id[m] : 0;
            act = q.active ? q.active[m] != 0 : true;
        }
    }
    const bool known = act & (trk < q.n_tracks);
    if (act & !known) {      // a track the handle does not have: nothing rolled out
        q.ret[i] = 0.0;
        q.steps[i] = 0;
        q.status[i] = PC_FIRST_RUNNING;
        if (q.gates) q.gates[i] = 0;
        if (q.laps) q.laps[i] = 0;
    }
    uint64_t todo = __ballot(known);
    while (todo) {
        const int first = __ffsll((unsigned long long)todo) - 1;
        const int cur = __builtin_amdgcn_readlane(trk, first);
        const bool match = known & (trk == cur);
        if (match) {
            const TrackHdr hc = cload(p.hdr + cur);
            if constexpr (sizeof(T) == 8) {
                if (!state) {      // the turn count's row of the rotation table and that row's rotation (step_poses_kernel's rule)
                    const int turns = st.k;
                    st.rot = hc.start_rot + 5.0 * (double)turns;
                    st.k = (turns >= -PC_OBSERVE_TURNS && turns <= PC_OBSERVE_TURNS && q.turn_row)
                               ? q.turn_row[(size_t)cur * (2 * PC_OBSERVE_TURNS + 1) + (size_t)(turns + PC_OBSERVE_TURNS)] : -1;
                    if (Math<double>::indexed(hc, st.k)) st.rot = Math<double>::rot_entry(p, hc, st.k, p.R + 1).x;
                }
            }
            const uint8_t* __restrict__ tab = q.actions + m * q.state_stride + k;
            double ret = 0.0;
            int status = PC_FIRST_RUNNING, t = 0, gates = 0, laps = 0;
#pragma unroll 1
            while (t < q.H && status == PC_FIRST_RUNNING) {
                const int a = seq_action(tab[(int64_t)t * q.K]);
                const bool gate_hit = gate_fires<T>(p, hc, st, next);      // the OLD pose and heading
                const int r = crash_step<T>(p, hc, st, a);
                // ---- bookkeeping (car_env.py:694-750), float64 reward exactly as the reference accumulates it
                double rw = 0.0;
                if ((a == 0) | (a == 4) | (a == 5)) rw += 0.01;      // :700,:710,:714
                if (gate_hit) {                  // :726
                    rw += 1.0;                   // :727
                    ++gates;
                    if (next == hc.G - 1) {      // :730 remaining == 0
                        rw += 10.0;              // :732
                        next = 0;                // :734-737
                        ++laps;
                    } else {
                        next += 1;               // :741
                    }
                }
                if (r == PC_CRASH_TERMINATED) {  // :746-748
                    rw -= 3.0;
                    status = PC_FIRST_TERMINATED;
                } else if (r == PC_CRASH_TRUNCATED) {      // :749-750
                    status = PC_FIRST_TRUNCATED;
                }
                ret += (double)(float)(rw * q.reward_scale);      // TransformReward, the float32 store (buffer.py:29), widened again
                ++t;
            }
            q.ret[i] = ret;
            q.steps[i] = t;
            q.status[i] = (uint8_t)status;
            if (q.gates) q.gates[i] = gates;
            if (q.laps) q.laps[i] = laps;
        }
        todo &= ~__ballot(match);
    }
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
