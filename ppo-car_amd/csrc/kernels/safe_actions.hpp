// safe_actions.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K21 safe_actions_kernel: which of the 9 actions can still avoid a crash within `depth` steps (pc_env_safe_actions for states the
// caller names, pc_env_safe_actions_state for the handle's current state).  With step = CarEnv.step without auto-reset, as K20 has it:
//   safe(s, a, 1) = not terminated(step(s, a))
//   safe(s, a, d) = not terminated(s' = step(s, a)) and (truncated(s') or exists a' in 0 .. 8: safe(s', a', d - 1))
// An exhaustive search over the action sequences, one lane per (state, first action), the state in registers from the first step to the
// verdict: no observation, no gate, no reward, nothing stored but the row's 9 bytes.  Nothing is stepped for good: the inputs and the
// handle's env state are only read.
#pragma once

// The states of one call (device arrays of M entries).  px == nullptr: the STATE form, the handle's own envs (M = its env count).
struct SafeActions {
    const double* __restrict__ px;
    const double* __restrict__ py;
    const double* __restrict__ vx;
    const double* __restrict__ vy;
    const int32_t* __restrict__ turns;        // heading = the track's start angle + 5 degrees * turns (ObservePoses' rule)
    const int32_t* __restrict__ time_step;    // or nullptr: 0
    const uint8_t* __restrict__ track_id;     // or nullptr: track 0
    const uint8_t* __restrict__ active;       // or nullptr: every row
    const int* __restrict__ turn_row;         // F64 handles: ObservePoses::turn_row
    int64_t M;
    int n_tracks;
};

// What the search carries from step to step: no gate index, no reward (neither enters `terminated` or `truncated`).
struct SearchRegs {
    double px, py, vx, vy, rot;    // rot: F64 handles, the heading in degrees
    int k;                         // F32: the turn count; F64: the row of the rotation table, -1 = none
    int time;
};

constexpr int PC_CRASH_ALIVE = 0, PC_CRASH_TERMINATED = 1, PC_CRASH_TRUNCATED = 2;

// One CarEnv.step of `st` under action a as far as `terminated` / `truncated` need it, by ONE lane: step_pose's action translation and
// Car.update restated (step_poses.hpp; car_env.py:698-722, :452-461), then Car.check_collision's rays j * (n // 4), j < nc, at the NEW
// pose, each by the very scan observe_pose<T> gives a ray -- scan_chain_d on F32 handles, the loop over all walls on F64 handles -- so
// `best < 10.0` is K20's decision bit for bit.  On F64 handles the heading moves as Car.move_car moves it, the literal rot +- 5.0 with the
// table's transition entry for the row: a sequence of steps never re-enters the one-way row of a turn count.
template <typename T>
__device__ __forceinline__ int crash_step(const EnvParams<T>& p, const TrackHdr& h, SearchRegs& st, const int a) {
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
    const double npx = st.px + nvx, npy = st.py + nvy;  // :459
    // ---- Car.check_collision at the NEW pose (:376-392): r in range(0, n, n // 4)
    bool hit = false;
#pragma unroll 1
    for (int j = 0; j < p.nc; ++j) {
        const int ray = j * p.q;
        double best = 1000.0;      // Ray.get_distance :198
        if constexpr (sizeof(T) == 4) {
            const double2 d64 = p.dirtab64[h.dir_off + Math<float>::dir_index(p, k_new, ray)];
            const SegD* sg64 = p.seg64 + h.vtx_off;
            best = scan_chain_d([sg64](const int i) { return cload(sg64 + i); }, h.nV, npx, npy, d64.x, d64.y);
        } else {
            double dx, dy;
            Math<double>::ray_dir(p, h, ray, k_new, rot_new, dx, dy);
            const Seg* walls = p.segs + h.wall_off;
            for (int w = 0; w < h.S; ++w) {
                const double d = Math<double>::cast(cload(walls + w), npx, npy, dx, dy);
                if (d < best) best = d;      // :203-207
            }
        }
        hit |= best < 10.0;      // :390
    }
    st.px = npx; st.py = npy; st.vx = nvx; st.vy = nvy; st.rot = rot_new;
    st.k = k_new;
    st.time += 1;  // :745
    if (hit | (h.start_collides != 0)) return PC_CRASH_TERMINATED;      // :746-748
    return st.time >= PC_TIME_LIMIT ? PC_CRASH_TRUNCATED : PC_CRASH_ALIVE;  // :749-750
}

// exists a in 0 .. 8: safe(s, a, D).  Compile-time recursion: every level's frame (4 doubles, the heading, the time) is a set of
// registers, there is no stack.  The first surviving child ends the level.
template <typename T, int D>
__device__ __forceinline__ bool any_safe(const EnvParams<T>& p, const TrackHdr& h, const SearchRegs& s) {
    if constexpr (D == 0) {
        return true;
    } else {
        bool found = false;
#pragma unroll 1
        for (int a = 0; a < 9 && !found; ++a) {
            SearchRegs c = s;
            const int r = crash_step<T>(p, h, c, a);
            if (r == PC_CRASH_TRUNCATED) found = true;      // the episode ended alive
            else if (r == PC_CRASH_ALIVE) found = any_safe<T, D - 1>(p, h, c);
        }
        return found;
    }
}

// Lane i: state m = i / 9 under first action a = i % 9; its verdict is byte i of `safe`.  Lanes of a wave diverge by construction (each
// follows its own first surviving branch); the wave is as slow as its slowest lane, and that is accepted.  Tracks: observe_kernel's
// waterfall, one body pass per distinct track id present in the wave.  No lane leaves before the ballot: a lane past the end, an
// inactive row and an unknown track are folded into `known`.
template <typename T, int DEPTH>
__global__ __launch_bounds__(256) void safe_actions_kernel(const EnvParams<T> p, const SafeActions q, uint8_t* __restrict__ safe) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < q.M * 9;
    const int64_t m = valid ? i / 9 : 0;
    const int a = (int)(i - m * 9);
    const bool state = q.px == nullptr;      // (uniform)
    SearchRegs st = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
    int trk = 0;
    bool act = valid;
    if (valid) {
        if (state) {
            const EnvRegs e = env_load<T>(p, m);
            st.px = e.px; st.py = e.py; st.vx = e.vx; st.vy = e.vy; st.rot = e.rot;
            st.k = e.k;
            st.time = e.time;
            trk = p.track_id ? p.track_id[m] : 0;
        } else {
            st.px = q.px[m]; st.py = q.py[m]; st.vx = q.vx[m]; st.vy = q.vy[m];
            st.k = q.turns[m];
            st.time = q.time_step ? q.time_step[m] : 0;
            trk = q.track_id ? q.track_id[m] : 0;
            act = q.active ? q.active[m] != 0 : true;
        }
    }
    const bool known = act & (trk < q.n_tracks);
    if (act & !known) safe[i] = 0;      // a track the handle does not have: 9 zeros
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
            const int r = crash_step<T>(p, hc, st, a);
            bool ok = r == PC_CRASH_TRUNCATED;
            if (r == PC_CRASH_ALIVE) ok = any_safe<T, DEPTH - 1>(p, hc, st);
            safe[i] = ok ? 1 : 0;
        }
        todo &= ~__ballot(match);
    }
}
