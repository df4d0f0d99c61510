// safe_actions.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K21 safe_actions_kernel: which of the 9 actions can still avoid a crash within `depth` steps (pc_env_safe_actions for states the
// caller names, pc_env_safe_actions_state for the handle's current state).  With step = CarEnv.step without auto-reset, as K20 has it:
//   safe(s, a, 1) = not terminated(step(s, a))
//   safe(s, a, d) = not terminated(s' = step(s, a)) and (truncated(s') or exists a' in 0 .. 8: safe(s', a', d - 1))
// An exhaustive search over the action sequences, one lane per (state, first action), the state in registers from the first step to the
// verdict: no observation, no gate, no reward, nothing stored but the row's 9 bytes.  Nothing is stepped for good: the inputs and the
// handle's env state are only read.
#pragma once

// The states of one call: PoseRows (car_step.hpp) without next_gate.
typedef PoseRows SafeActions;

constexpr int PC_CRASH_ALIVE = 0, PC_CRASH_TERMINATED = 1, PC_CRASH_TRUNCATED = 2;

// One CarEnv.step of `st` under action a as far as `terminated` / `truncated` need it, by ONE lane: car_move (car_step.hpp), then
// Car.check_collision's rays j * (n // 4), j < nc, at the NEW pose, each by the very scan observe_pose<T> gives a ray -- scan_chain_d on
// F32 handles, the loop over all walls on F64 handles -- so `best < 10.0` is K20's decision bit for bit.  No gate index, no reward:
// neither enters `terminated` or `truncated`.
template <typename T>
__device__ __forceinline__ int crash_step(const EnvParams<T>& p, const TrackHdr& h, CarRegs& st, const int a, CarAction& did) {
    const int time = st.time + 1;  // :745
    st = car_move<T>(p, h, st, a, did);
    st.time = time;
    // ---- Car.check_collision at the NEW pose (:376-392): r in range(0, n, n // 4)
    bool hit = false;
#pragma unroll 1
    for (int j = 0; j < p.nc; ++j) {
        const int ray = j * p.q;
        double best = 1000.0;      // Ray.get_distance :198
        if constexpr (sizeof(T) == 4) {
            const double2 d64 = p.dirtab64[h.dir_off + Math<float>::dir_index(p, st.k, ray)];
            const SegD* sg64 = p.seg64 + h.vtx_off;
            best = scan_chain_d([sg64](const int i) { return cload(sg64 + i); }, h.nV, st.px, st.py, d64.x, d64.y);
        } else {
            double dx, dy;
            Math<double>::ray_dir(p, h, ray, st.k, st.rot, dx, dy);
            const Seg* walls = p.segs + h.wall_off;
            for (int w = 0; w < h.S; ++w) {
                const double d = Math<double>::cast(cload(walls + w), st.px, st.py, dx, dy);
                if (d < best) best = d;      // :203-207
            }
        }
        hit |= best < 10.0;      // :390
    }
    if (hit | (h.start_collides != 0)) return PC_CRASH_TERMINATED;      // :746-748
    return st.time >= PC_TIME_LIMIT ? PC_CRASH_TRUNCATED : PC_CRASH_ALIVE;  // :749-750
}

// exists a in 0 .. 8: safe(s, a, D).  Compile-time recursion: every level's frame (4 doubles, the heading, the time) is a set of
// registers, there is no stack.  The first surviving child ends the level.
template <typename T, int D>
__device__ __forceinline__ bool any_safe(const EnvParams<T>& p, const TrackHdr& h, const CarRegs& s) {
    if constexpr (D == 0) {
        return true;
    } else {
        bool found = false;
#pragma unroll 1
        for (int a = 0; a < 9 && !found; ++a) {
            CarRegs c = s;
            CarAction did;
            const int r = crash_step<T>(p, h, c, a, did);
            if (r == PC_CRASH_TRUNCATED) found = true;      // the episode ended alive
            else if (r == PC_CRASH_ALIVE) found = any_safe<T, D - 1>(p, h, c);
        }
        return found;
    }
}

// Lane i: state m = i / 9 under first action a = i % 9; its verdict is byte i of `safe`.  Lanes of a wave diverge by construction (each
// follows its own first surviving branch); the wave is as slow as its slowest lane, and that is accepted.  One body pass per distinct
// track id present in the wave (for_each_track, car_step.hpp): a lane past the end, an inactive row and an unknown track are folded into
// `known`.
template <typename T, int DEPTH>
__global__ __launch_bounds__(256) void safe_actions_kernel(const EnvParams<T> p, const SafeActions q, uint8_t* __restrict__ safe) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < q.M * 9;
    const int64_t m = valid ? i / 9 : 0;
    const int a = (int)(i - m * 9);
    const bool state = q.px == nullptr;      // (uniform)
    CarRegs st = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
    int next = 0, trk = 0;
    bool act = false;
    if (valid) load_pose<T>(p, q, state, m, st, next, trk, act);
    const bool known = act & (trk < q.n_tracks);
    if (act & !known) safe[i] = 0;      // a track the handle does not have: 9 zeros
    for_each_track(known, trk, [&](const int cur) {
        const TrackHdr hc = cload(p.hdr + cur);
        if (!state) resolve_turns<T>(p, hc, cur, q.turn_row, st);
        CarAction did;
        const int r = crash_step<T>(p, hc, st, a, did);
        bool ok = r == PC_CRASH_TRUNCATED;
        if (r == PC_CRASH_ALIVE) ok = any_safe<T, DEPTH - 1>(p, hc, st);
        safe[i] = ok ? 1 : 0;
    });
}
