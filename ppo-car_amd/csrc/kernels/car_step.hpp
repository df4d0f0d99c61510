// car_step.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// The ONE definition of the stateless car step's pieces, shared by K17 observe_kernel (observe.hpp), K20 step_poses_kernel
// (step_poses.hpp), K21 safe_actions_kernel (safe_actions.hpp) and K22 sequences_kernel (sequences.hpp): the rows a call names and how a
// lane loads one (PoseRows, load_pose), the heading rule of a turn count (resolve_turns), the track waterfall (for_each_track), the move
// (car_move), the gate test (gate_fires) and the bookkeeping (step_books).  The production step (env_step_core, env_step.hpp) and the
// persistent rollouts (rollout.hpp) keep their own, tuned forms; the bit-for-bit tests hold these to them.
#pragma once

// How many 5-degree turns either way of the start angle a turn count maps onto an F64 handle's rotation table (an episode makes at most
// 1000 turns, car_env.py:749: the table holds no rotation further out).
constexpr int PC_OBSERVE_TURNS = 1000;

// The state rows of one call (device arrays of M entries) and what the handle adds to them.  RW = false: rows that are only read.
// RW = true: rows that the same launch reads AND writes (K20: every lane of a row's group loads the row first, lane 0 of the group stores
// it last), which carry neither const nor __restrict__.  px == nullptr: the STATE form, the handle's own envs (M = its env count).
template <bool RW, typename S> using RowPtr = std::conditional_t<RW, S*, const S* __restrict__>;
template <bool RW>
struct PoseRowsT {
    RowPtr<RW, double> px, py;
    RowPtr<RW, double> vx, vy;                // or nullptr: 0
    RowPtr<RW, int32_t> turns;                // heading = the track's start angle + 5 degrees * turns
    RowPtr<RW, int32_t> next_gate;            // or nullptr: 0
    RowPtr<RW, int32_t> time_step;            // or nullptr: 0
    const uint8_t* __restrict__ track_id;     // or nullptr: track 0
    const uint8_t* __restrict__ active;       // or nullptr: every row
    const int* __restrict__ turn_row;         // F64 handles: [n_tracks][2 * PC_OBSERVE_TURNS + 1] row of the rotation table, -1 = none
    int64_t M;
    int n_tracks;
};
using PoseRows = PoseRowsT<false>;

// One car as a lane holds it from step to step.
struct CarRegs {
    double px, py, vx, vy, rot;    // rot: F64 handles, the heading in degrees
    int k;                         // F32: the turn count; F64: the row of the rotation table, -1 = none
    int time;
};

// Row m of `q` with its defaults, or (state) env m of the handle as env_step_core holds it.  From the rows, st.k is the turn COUNT:
// resolve_turns makes it the heading once the track is known.
template <typename T, bool RW>
__device__ __forceinline__ void load_pose(const EnvParams<T>& p, const PoseRowsT<RW>& q, const bool state, const int64_t m, CarRegs& st,
                                          int& next, int& trk, bool& act) {
    if (state) {
        const EnvRegs e = env_load<T>(p, m);
        st.px = e.px; st.py = e.py; st.vx = e.vx; st.vy = e.vy; st.rot = e.rot;
        st.k = e.k;
        st.time = e.time;
        next = e.next;
        trk = p.track_id ? p.track_id[m] : 0;
        act = true;
    } else {
        st.px = q.px[m];
        st.py = q.py[m];
        st.vx = q.vx ? q.vx[m] : 0.0;
        st.vy = q.vy ? q.vy[m] : 0.0;
        st.rot = 0.0;
        st.k = q.turns[m];
        st.time = q.time_step ? q.time_step[m] : 0;
        next = q.next_gate ? q.next_gate[m] : 0;
        trk = q.track_id ? q.track_id[m] : 0;
        act = q.active ? q.active[m] != 0 : true;
    }
}

// The heading of a row's turn count on track `cur` (header h).  F32 handles: the count itself.  F64 handles: the count's row of the
// rotation table (the host walked start_rot +- 5.0 that many times ONE way, as Car.move_car does) and that row's rotation; a count beyond
// the table is start_rot + 5.0 * turns with no row (-1), which goes through the hash / the device's cos, sin.
// K17 never moves the car and once lived without the rot_entry line.  The line cannot change its bits: it runs only where the row is
// indexed, and with an indexed row Math<double>::heading and Math<double>::ray_dir -- all K17 does with (k, rot) -- return the table's
// entries and never look at rot.
template <typename T>
__device__ __forceinline__ void resolve_turns(const EnvParams<T>& p, const TrackHdr& h, const int cur, const int* __restrict__ turn_row,
                                              CarRegs& st) {
    if constexpr (sizeof(T) == 8) {
        const int turns = st.k;
        st.rot = h.start_rot + 5.0 * (double)turns;
        st.k = (turns >= -PC_OBSERVE_TURNS && turns <= PC_OBSERVE_TURNS && turn_row)
                   ? turn_row[(size_t)cur * (2 * PC_OBSERVE_TURNS + 1) + (size_t)(turns + PC_OBSERVE_TURNS)] : -1;
        // the row's rotation is its last column, R + 1: addressed as the entry before the next row's first, which needs no R + 1 of its
        // own beside the row length the casts already hold (one SGPR less in observe_kernel)
        if (Math<double>::indexed(h, st.k)) st.rot = Math<double>::rot_entry(p, h, st.k + 1, -1).x;
    }
}

// The track waterfall: body(cur) once per distinct track id among the wave's `known` lanes, run by the lanes of that track, so that the
// body reads the track's records through wave-uniform (scalar) loads.  A wave whose lanes share a track runs the body once.
// EVERY lane of the wave must reach this call: the ballots are taken over the lanes that are here, and a lane that left early would be
// missing from `todo` while its track's pass still ran without it -- or, having left mid-loop, would never clear its bit.  So a kernel
// folds whatever a lane has no work for (past the end, an inactive row, an unknown track) into known = false instead of returning; the
// only exit allowed before the call is one that whole waves, or whole lane groups that share `trk`, take together.
template <typename F>
__device__ __forceinline__ void for_each_track(const bool known, const int trk, F&& body) {
    uint64_t todo = __ballot(known);
    while (todo) {
        const int first = __ffsll((unsigned long long)todo) - 1;
        const int cur = __builtin_amdgcn_readlane(trk, first);
        const bool match = known & (trk == cur);
        if (match) body(cur);
        todo &= ~__ballot(match);
    }
}

// The action translation (car_env.py:698-722) and Car.update (:452-461): `s` moved under action a, its time untouched.  A: the action's
// integer type, compared as it comes; anything outside 0 .. 8 acts as 8 (no thrust, no turn).  `did`: what the action asked for.
// On F64 handles the heading moves as Car.move_car moves it, the literal rot +- 5.0 with the table's transition entry for the row: a
// sequence of steps never re-enters the one-way row of a turn count.
struct CarAction {
    bool fwd;      // it thrust forward (the reward's 0.01)
    int turn;      // what it adds to the turn count: -1 left, +1 right, 0
};

template <typename T, typename A>
__device__ __forceinline__ CarRegs car_move(const EnvParams<T>& p, const TrackHdr& h, const CarRegs& s, const A a, CarAction& did) {
    // ---- action translation: thrust first with the PRE-turn heading, then the turn
    const bool fwd = (a == 0) | (a == 4) | (a == 5), bwd = (a == 1) | (a == 6) | (a == 7);
    const bool left = (a == 2) | (a == 4) | (a == 6), right = (a == 3) | (a == 5) | (a == 7);
    double ch0, sh0;  // heading before the turn
    Math<T>::heading(p, h, s.k, s.rot, ch0, sh0);
    double accx = 0.0, accy = 0.0;
    if (fwd) {  // Car.move_car("forward") :423-430
        accx = ch0 * 0.8;
        accy = sh0 * 0.8;
    } else if (bwd) {  // "backward" :431-438: -force_dir * 0.8
        accx = -ch0 * 0.8;
        accy = -sh0 * 0.8;
    }
    CarRegs n = s;
    if (left) {  // :440
        n.rot -= 5.0;
        n.k -= 1;
    }
    if (right) {  // :442
        n.rot += 5.0;
        n.k += 1;
    }
    if constexpr (sizeof(T) == 8) {      // F64: k is a row of the rotation table: its transition entry (the row of rot -+ 5.0, -1 = none)
        n.k = s.k;
        if (left | right) n.k = Math<double>::turn(p, h, s.k, left);
    }
    // ---- Car.update physics, float64 in both modes
    double nvx = s.vx + accx, nvy = s.vy + accy;  // :452
    if (!(fwd | bwd)) {                           // :454 ||acc|| == 0  <=>  no thrust
        nvx *= 1 - 0.2;                           // :455
        nvy *= 1 - 0.2;
    }
    n.vx = nvx < -10.0 ? -10.0 : (nvx > 10.0 ? 10.0 : nvx);  // :457 np.clip per component
    n.vy = nvy < -10.0 ? -10.0 : (nvy > 10.0 ? 10.0 : nvy);
    n.px = s.px + n.vx;  // :459
    n.py = s.py + n.vy;
    did.fwd = fwd;
    did.turn = (right ? 1 : 0) - (left ? 1 : 0);
    return n;
}

// Car.get_passed_gate (car_env.py:394-408): the collision rays j * (n // 4), j < nc, at the pose and heading in `st` against gate[next]
// only, env_step_core's casts per dtype.  Lane g of G casts rays g, g + G, ... (a uniform trip count) and returns what ITS rays found: a
// group ORs its lanes' answers, a single lane passes (0, 1).  A next_gate outside 0 .. G - 1: no gate to test.
template <typename T>
__device__ __forceinline__ bool gate_fires(const EnvParams<T>& p, const TrackHdr& h, const CarRegs& st, const int next, const int g,
                                           const int G) {
    if ((next < 0) | (next >= h.G)) return false;
    const Seg gate = p.segs[h.gate_off + next];
    bool fired = false;
#pragma unroll 1
    for (int j0 = 0; j0 < p.nc; j0 += G) {
        const int j = g + j0;
        const int ray = (j < p.nc ? j : 0) * p.q;
        bool hit;
        if constexpr (sizeof(T) == 4) {      // cast_d on the float64 lattice
            const double2 cs = p.dirtab64[h.dir_off + Math<float>::dir_index(p, st.k, ray)];
            hit = cast_d(gate, st.px, st.py, cs.x, cs.y) < 10.0;      // :387,:390
        } else {                             // the reference's own cast on the rotation's ray
            double dx, dy;
            Math<double>::ray_dir(p, h, ray, st.k, st.rot, dx, dy);
            hit = Math<double>::cast(gate, st.px, st.py, dx, dy) < 10.0;
        }
        fired |= hit & (j < p.nc);
    }
    return fired;
}

// What one CarEnv.step books (car_env.py:694-750) beside the move.
struct StepBooks {
    float reward;      // TransformReward, then the float32 store (buffer.py:29)
    int next;          // the next gate after the step
    bool term, trunc;
    bool gate, lap;    // gate[next] fired; it closed a lap
};

// forward: the action thrust forward; gate_hit: gate[next] fired at the old pose; crashed: the car is destroyed at the new pose (a wall
// hit, or a track whose start collides); time: the episode's step count AFTER this step; G: the track's gate count.  The reward is summed
// in float64 exactly as the reference accumulates it.
__device__ __forceinline__ StepBooks step_books(const bool forward, const bool gate_hit, const bool crashed, const int time, const int next,
                                                const int G, const double reward_scale) {
    StepBooks b = {0.0f, next, false, false, gate_hit, false};
    double rw = 0.0;
    if (forward) rw += 0.01;      // :700,:710,:714
    if (gate_hit) {               // :726
        rw += 1.0;                // :727
        if (next == G - 1) {      // :730 remaining == 0
            rw += 10.0;           // :732
            b.next = 0;           // :734-737
            b.lap = true;
        } else {
            b.next = next + 1;    // :741
        }
    }
    if (crashed) {  // :746-748
        b.term = true;
        rw -= 3.0;
    } else if (time >= PC_TIME_LIMIT) {  // :749-750
        b.trunc = true;
    }
    b.reward = (float)(rw * reward_scale);
    return b;
}
