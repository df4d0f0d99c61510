// observe.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K17 observe_kernel: CarEnv._get_obs (car_env.py:569-597) + Car.check_collision (car_env.py:376-392) of ARBITRARY poses on the
// handle's tracks (pc_env_observe_poses), or of the handle's current state (pc_env_observe).  Nothing is stepped and no env
// state is written.
#pragma once

// The poses of one pc_env_observe_poses call: PoseRows (car_step.hpp) without next_gate, time_step and active.  The STATE form of the
// kernel reads the handle's own arrays instead and uses only M, n_tracks and lg.
struct ObservePoses : PoseRows {
    int lg;      // log2(lanes per pose)
};

// One pose on track `trk` (the same in every active lane), by the 2^lg lanes of its group: lane g measures rays g, g + G, ...
// Every ray takes the exhaustive float64 form -- the minimum over the track's whole wall list -- that reset_obs_kernel takes:
// poses come from anywhere (on a wall, on a vertex, outside the track), where the float32 selector certifies nothing; and a
// ray reports the same bits whether the sweep certified it or the scan resolved it (env_math.hpp, above cast_exact), so on an
// F32 handle these are pc_env_step's observation bits.  (k, rot): the heading as the step holds it -- F32: the turn count;
// F64: the row of the rotation table (-1: none) and the angle in degrees.
template <typename T>
__device__ __forceinline__ void observe_pose(const EnvParams<T>& p, const int trk, const int g, const int lg, const double px,
                                             const double py, const double vx, const double vy, const int k, const double rot,
                                             float* __restrict__ orow, uint8_t* __restrict__ collides) {
    const TrackHdr h = cload(p.hdr + __builtin_amdgcn_readfirstlane(trk));
    const int G = 1 << lg;
    bool hit = false;
    for (int ray = g; ray < p.R; ray += G) {
        double best = 1000.0;      // Ray.get_distance :198
        if constexpr (sizeof(T) == 4) {      // the float64 chain scan the step's refinement falls back to (wave-uniform records: scalar loads)
            const double2 d64 = p.dirtab64[h.dir_off + Math<float>::dir_index(p, k, ray)];
            const SegD* sg64 = p.seg64 + h.vtx_off;
            best = scan_chain_d([sg64](const int j) { return cload(sg64 + j); }, h.nV, px, py, d64.x, d64.y);
        } else {                             // Ray.get_distance (:186-213) over every wall, the reference's own arithmetic
            double dx, dy;
            Math<double>::ray_dir(p, h, ray, k, rot, dx, dy);
            const Seg* walls = p.segs + h.wall_off;
            for (int w = 0; w < h.S; ++w) {
                const double d = Math<double>::cast(cload(walls + w), px, py, dx, dy);
                if (d < best) best = d;      // :203-207
            }
        }
        orow[6 + ray] = Math<T>::norm_dist(best);      // :593
        // Car.check_collision's rays: r in range(0, n, n // 4) (:389) -- nominal n, not R
        if (ray < p.n_nominal && ray % p.q == 0 && best < 10.0) hit = true;      // :390
    }
    if (g == 0) {
        double ch, sh;
        Math<T>::heading(p, h, k, rot, ch, sh);
        orow[0] = Math<T>::norm(px, 1280.0);      // :578-581
        orow[1] = Math<T>::norm(py, 720.0);
        orow[2] = Math<T>::norm(vx, 10.0);
        orow[3] = Math<T>::norm(vy, 10.0);
        orow[4] = (float)ch;                      // :584-588
        orow[5] = (float)sh;
    }
    // any() over the pose's lanes: xor butterfly inside the 2^lg-lane group (every lane of a group is here: they share the pose)
    int flag = hit ? 1 : 0;
    for (int m = 1; m < G; m <<= 1) flag |= __shfl_xor(flag, m, 64);
    if (g == 0 && collides) *collides = (uint8_t)flag;
}

// STATE = false: pose m of `q`.  STATE = true: env m of the handle, heading as env_step_core takes it (k, and rot on F64 handles).
// One body pass per distinct track id present in a wave (for_each_track, car_step.hpp): the only exit before it is the bound on m,
// which whole groups take together.
template <typename T, bool STATE>
__global__ __launch_bounds__(256) void observe_kernel(const EnvParams<T> p, const ObservePoses q, float* __restrict__ obs,
                                                      uint8_t* __restrict__ collides) {
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = lane >> q.lg;
    const int g = (int)(lane & ((1 << q.lg) - 1));
    if (m >= q.M) return;
    CarRegs st;
    int next, trk;
    bool act;      // (K17 has no `active` rows: every pose is observed)
    load_pose<T>(p, q, STATE, m, st, next, trk, act);
    float* __restrict__ orow = obs + (size_t)m * p.D;
    uint8_t* __restrict__ crow = collides ? collides + m : nullptr;
    const bool known = trk < q.n_tracks;
    if (!known) {      // a track the handle does not have: a row of zeros, no collision
        for (int i = g; i < p.D; i += 1 << q.lg) orow[i] = 0.0f;
        if (g == 0 && crow) *crow = 0;
    }
    for_each_track(known, trk, [&](const int cur) {
        if constexpr (!STATE) resolve_turns<T>(p, cload(p.hdr + cur), cur, q.turn_row, st);
        observe_pose<T>(p, cur, g, q.lg, st.px, st.py, st.vx, st.vy, st.k, st.rot, orow, crow);
    });
}
