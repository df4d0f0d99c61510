// step_poses.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K20 step_poses_kernel: one CarEnv.step (car_env.py:693-760) of M caller-supplied states on the handle's tracks
// (pc_env_step_poses).  No auto-reset; the handle's own env state is neither read nor written.  The action translation, the physics
// and the bookkeeping restate env_step_core's arithmetic (env_step.hpp); the gate test is env_step_core's per dtype; the observation
// and the wall test at the new pose are observe_pose<T> (observe.hpp), whose exhaustive float64 scan takes poses from anywhere.
#pragma once

// The rows of one pc_env_step_poses call (device arrays of M entries).  The state arrays are read AND written by the same launch
// (every lane of a row's group loads the row first, lane 0 of the group stores it last): they carry neither const nor __restrict__.
struct StepPoses {
    double* px;
    double* py;
    double* vx;
    double* vy;
    int32_t* turns;                // heading = the track's start angle + 5 degrees * turns (ObservePoses' rule); out: turns +- 1
    int32_t* next_gate;
    int32_t* time_step;
    const uint8_t* track_id;       // or nullptr: track 0
    const int64_t* actions;        // anything outside 0 .. 8 acts as 8 (no thrust, no turn)
    const uint8_t* active;         // or nullptr: every row
    const int* turn_row;           // F64 handles: ObservePoses::turn_row
    float* reward;
    uint8_t* terminated;
    uint8_t* truncated;
    uint8_t* gate;                 // or nullptr
    double reward_scale;
    int64_t M;
    int n_tracks;
    int lg;                        // log2(lanes per row)
};

// One row's state as the 2^lg lanes of its group hold it (identically), and what the step reports beside it.
struct PoseRegs {
    double px, py, vx, vy, rot;    // rot: F64 handles, the heading in degrees
    int k;                         // F32: the turn count; F64: the row of the rotation table, -1 = none
    int next, time;
    float reward;
    bool term, trunc, gate;
};

// One CarEnv.step of the row in `st` on track `trk` (the same in every active lane), by the 2^lg lanes of its group; every lane
// leaves with the same new state except `term`, which lane 0 of the group holds (observe_pose reports to that lane).
template <typename T>
__device__ __forceinline__ void step_pose(const EnvParams<T>& p, const int trk, const int g, const int lg, PoseRegs& st, const int64_t a,
                                          const double reward_scale, float* __restrict__ orow) {
    const TrackHdr h = cload(p.hdr + __builtin_amdgcn_readfirstlane(trk));
    const int G = 1 << lg;
    const double rot_old = st.rot;

    // ---- action translation (car_env.py:698-722): thrust first with the PRE-turn heading, then the turn
    const bool fwd = (a == 0) | (a == 4) | (a == 5), bwd = (a == 1) | (a == 6) | (a == 7);
    const bool left = (a == 2) | (a == 4) | (a == 6), right = (a == 3) | (a == 5) | (a == 7);
    double ch0, sh0;  // heading before the turn
    Math<T>::heading(p, h, st.k, rot_old, ch0, sh0);
    double accx = 0.0, accy = 0.0;
    if (fwd) {  // Car.move_car("forward") :423-430
        accx = ch0 * 0.8;
        accy = sh0 * 0.8;
    } else if (bwd) {  // "backward" :431-438: -force_dir * 0.8
        accx = -ch0 * 0.8;
        accy = -sh0 * 0.8;
    }
    double rot_new = rot_old;
    int k_new = st.k;
    if (left) {  // :440
        rot_new -= 5.0;
        k_new -= 1;
    }
    if (right) {  // :442
        rot_new += 5.0;
        k_new += 1;
    }
    if constexpr (sizeof(T) == 8) {      // F64: k is a row of the rotation table: its transition entry (the row of rot -+ 5.0, -1 = none)
        k_new = st.k;
        if (left | right) k_new = Math<double>::turn(p, h, st.k, left);
    }

    // ---- Car.update physics (car_env.py:452-461), float64 in both modes
    double nvx = st.vx + accx, nvy = st.vy + accy;  // :452
    if (!(fwd | bwd)) {                             // :454 ||acc|| == 0  <=>  no thrust
        nvx *= 1 - 0.2;                             // :455
        nvy *= 1 - 0.2;
    }
    nvx = nvx < -10.0 ? -10.0 : (nvx > 10.0 ? 10.0 : nvx);  // :457 np.clip per component
    nvy = nvy < -10.0 ? -10.0 : (nvy > 10.0 ? 10.0 : nvy);
    const double opx = st.px, opy = st.py;
    const double npx = opx + nvx, npy = opy + nvy;  // :459

    // ---- Car.get_passed_gate (:394-408): the collision rays j * (n // 4), j < nc, at the OLD pose with the OLD heading against
    // gate[next] only, dealt round-robin to the row's lanes.  A next_gate outside 0 .. G - 1: no gate to test (a zero segment never hits).
    const bool gate_ok = (st.next >= 0) & (st.next < h.G);
    Seg gate = {0.0, 0.0, 0.0, 0.0};
    if (gate_ok) gate = p.segs[h.gate_off + st.next];
    bool gate_hit = false;
    int k5o = 0;
    if constexpr (sizeof(T) == 4) k5o = 5 * Math<float>::mod72(st.k);
#pragma unroll 1
    for (int jj = 0; jj * G < p.nc; ++jj) {  // (uniform trip count)
        const int j = g + jj * G;
        const int ray = (j < p.nc ? j : 0) * p.q;
        bool hit;
        if constexpr (sizeof(T) == 4) {      // cast_d on the float64 lattice, as env_step_core casts it
            const unsigned m = (unsigned)(k5o + ray * p.step_deg);
            const double2 cs = p.dirtab64[h.dir_off + (int)min(m, m - 360u)];
            hit = cast_d(gate, opx, opy, cs.x, cs.y) < 10.0;  // :387,:390
        } else {                             // the reference's own cast on the old rotation's ray
            double odx, ody;
            Math<double>::ray_dir(p, h, ray, st.k, rot_old, odx, ody);
            hit = Math<double>::cast(gate, opx, opy, odx, ody) < 10.0;
        }
        gate_hit |= hit & (j < p.nc) & gate_ok;
    }
    int flag = gate_hit ? 1 : 0;      // any() over the row's lanes (every lane of a group is here: they share the row)
    for (int m = 1; m < G; m <<= 1) flag |= __shfl_xor(flag, m, 64);
    gate_hit = flag != 0;

    // ---- the observation CarEnv.step returns, and Car.check_collision, at the NEW pose (lane 0 of the group receives `collides`)
    uint8_t collides = 0;
    observe_pose<T>(p, trk, g, lg, npx, npy, nvx, nvy, k_new, rot_new, orow, &collides);
    const bool wall_hit = collides != 0;

    // ---- bookkeeping (car_env.py:694-750), float64 reward exactly as the reference accumulates it
    double rw = 0.0;
    if (fwd) rw += 0.01;  // :700,:710,:714
    int next = st.next;
    if (gate_hit) {               // :726
        rw += 1.0;                // :727
        if (next == h.G - 1) {    // :730 remaining == 0
            rw += 10.0;           // :732
            next = 0;             // :734-737
        } else {
            next += 1;            // :741
        }
    }
    const int time = st.time + 1;  // :745
    const bool destroyed = wall_hit | (h.start_collides != 0);
    bool term = false, trunc = false;
    if (destroyed) {  // :746-748
        term = true;
        rw -= 3.0;
    } else if (time >= PC_TIME_LIMIT) {  // :749-750
        trunc = true;
    }
    st.reward = (float)(rw * reward_scale);  // TransformReward then float32 store (buffer.py:29)
    st.term = term;
    st.trunc = trunc;
    st.gate = gate_hit;
    st.px = npx; st.py = npy; st.vx = nvx; st.vy = nvy; st.rot = rot_new;
    st.k = k_new;
    st.next = next;
    st.time = time;
}

// Row m of `q` by 2^lg lanes, 256 threads; one body pass per distinct track id present in a wave (observe_kernel's waterfall).  A row
// that is not stepped -- active[m] == 0, or a track the handle does not have -- is folded into `known` instead of leaving early: the
// ballot that drives the waterfall is taken over lanes that all reach it (the only exit before it is the bound on m, which whole
// groups take together).
template <typename T>
__global__ __launch_bounds__(256) void step_poses_kernel(const EnvParams<T> p, const StepPoses q, float* __restrict__ obs) {
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = lane >> q.lg;
    const int g = (int)(lane & ((1 << q.lg) - 1));
    if (m >= q.M) return;
    // every lane of the group loads the row; lane 0 stores it at the very end
    PoseRegs st;
    st.px = q.px[m]; st.py = q.py[m]; st.vx = q.vx[m]; st.vy = q.vy[m];
    st.rot = 0.0;
    const int turns = q.turns[m];
    st.k = turns;
    st.next = q.next_gate[m];
    st.time = q.time_step[m];
    st.reward = 0.0f;
    st.term = st.trunc = st.gate = false;
    const int64_t a = q.actions[m];
    const int trk = q.track_id ? q.track_id[m] : 0;
    const bool act = q.active ? q.active[m] != 0 : true;
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
    uint64_t todo = __ballot(known);
    while (todo) {
        const int first = __ffsll((unsigned long long)todo) - 1;
        const int cur = __builtin_amdgcn_readlane(trk, first);
        const bool match = known & (trk == cur);
        if (match) {
            if constexpr (sizeof(T) == 8) {
                // F64 handles: the turn count's row of the rotation table and that row's rotation (pc_env_observe_poses' rule: start_rot
                // after that many turns ONE way); a count beyond the table is start_rot + 5.0 * turns, through the hash / the device's cos, sin
                const TrackHdr hc = cload(p.hdr + cur);
                st.rot = hc.start_rot + 5.0 * (double)turns;
                st.k = (turns >= -PC_OBSERVE_TURNS && turns <= PC_OBSERVE_TURNS && q.turn_row)
                           ? q.turn_row[(size_t)cur * (2 * PC_OBSERVE_TURNS + 1) + (size_t)(turns + PC_OBSERVE_TURNS)] : -1;
                if (Math<double>::indexed(hc, st.k)) st.rot = Math<double>::rot_entry(p, hc, st.k, p.R + 1).x;
            }
            step_pose<T>(p, cur, g, q.lg, st, a, q.reward_scale, orow);
            if (g == 0) {
                // the new turn count: +-1 (F32: step_pose moved k itself; F64: k is a table row, the count moves with the action)
                const bool left = (a == 2) | (a == 4) | (a == 6), right = (a == 3) | (a == 5) | (a == 7);
                q.px[m] = st.px; q.py[m] = st.py; q.vx[m] = st.vx; q.vy[m] = st.vy;
                q.turns[m] = turns + (right ? 1 : 0) - (left ? 1 : 0);
                q.next_gate[m] = st.next;
                q.time_step[m] = st.time;
                q.reward[m] = st.reward;
                q.terminated[m] = st.term ? 1 : 0;
                q.truncated[m] = st.trunc ? 1 : 0;
                if (q.gate) q.gate[m] = st.gate ? 1 : 0;
            }
        }
        todo &= ~__ballot(match);
    }
}
