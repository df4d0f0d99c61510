// observe.hpp -- part of the single translation unit ppocar.hip (included there, in order; not a stand-alone header).
// K17 observe_kernel: CarEnv._get_obs (car_env.py:569-597) + Car.check_collision (car_env.py:376-392) of ARBITRARY poses on the
// handle's tracks (pc_env_observe_poses), or of the handle's current state (pc_env_observe).  Nothing is stepped and no env
// state is written.
#pragma once

// How many 5-degree turns either way of the start angle pc_env_observe_poses maps onto an F64 handle's rotation table (an
// episode makes at most 1000 turns, car_env.py:749: the table holds no rotation further out).
constexpr int PC_OBSERVE_TURNS = 1000;

// The poses of one pc_env_observe_poses call (device arrays of M entries).  The STATE form of the kernel reads the handle's own
// arrays instead and uses only M, n_tracks and lg.
struct ObservePoses {
    const double* __restrict__ px;
    const double* __restrict__ py;
    const double* __restrict__ vx;           // or nullptr: 0
    const double* __restrict__ vy;           // or nullptr: 0
    const int32_t* __restrict__ turns;       // heading = the track's start angle + 5 degrees * turns
    const uint8_t* __restrict__ track_id;    // or nullptr: track 0
    const int* __restrict__ turn_row;        // F64 handles: [n_tracks][2 * PC_OBSERVE_TURNS + 1] row of the rotation table, -1 = none
    int64_t M;
    int n_tracks;
    int lg;                                  // log2(lanes per pose)
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
// A wave whose poses share a track runs the body once with that track's records in SGPRs; otherwise once per distinct track id
// present (env_step_kernel<.., MIXED>'s waterfall).  The loop's mask is taken once, ahead of it, over lanes that all reach it: the
// only lane-dependent exit before it is the bound on m, which whole groups take together.
template <typename T, bool STATE>
__global__ __launch_bounds__(256) void observe_kernel(const EnvParams<T> p, const ObservePoses q, float* __restrict__ obs,
                                                      uint8_t* __restrict__ collides) {
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = lane >> q.lg;
    const int g = (int)(lane & ((1 << q.lg) - 1));
    if (m >= q.M) return;
    double px, py, vx, vy, rot = 0.0;
    int k, trk;
    if constexpr (STATE) {
        const EnvRegs st = env_load<T>(p, m);
        px = st.px; py = st.py; vx = st.vx; vy = st.vy; rot = st.rot;
        k = st.k;
        trk = p.track_id ? p.track_id[m] : 0;
    } else {
        px = q.px[m];
        py = q.py[m];
        vx = q.vx ? q.vx[m] : 0.0;
        vy = q.vy ? q.vy[m] : 0.0;
        k = q.turns[m];
        trk = q.track_id ? q.track_id[m] : 0;
    }
    float* __restrict__ orow = obs + (size_t)m * p.D;
    uint8_t* __restrict__ crow = collides ? collides + m : nullptr;
    const bool known = trk < q.n_tracks;
    if (!known) {      // a track the handle does not have: a row of zeros, no collision
        for (int i = g; i < p.D; i += 1 << q.lg) orow[i] = 0.0f;
        if (g == 0 && crow) *crow = 0;
    }
    uint64_t todo = __ballot(known);
    while (todo) {
        const int first = __ffsll((unsigned long long)todo) - 1;
        const int cur = __builtin_amdgcn_readlane(trk, first);
        const bool match = known & (trk == cur);
        if (match) {
            if constexpr (!STATE && sizeof(T) == 8) {
                // F64 handles: the turn count's row of the rotation table (the host walked start_rot +- 5.0 that many times, as
                // Car.move_car does); a count beyond the table takes start_rot + 5.0 * turns through the hash / the device's cos, sin
                const int t = k;
                rot = p.hdr[cur].start_rot + 5.0 * (double)t;
                k = (t >= -PC_OBSERVE_TURNS && t <= PC_OBSERVE_TURNS && q.turn_row)
                        ? q.turn_row[(size_t)cur * (2 * PC_OBSERVE_TURNS + 1) + (size_t)(t + PC_OBSERVE_TURNS)] : -1;
            }
            observe_pose<T>(p, cur, g, q.lg, px, py, vx, vy, k, rot, orow, crow);
        }
        todo &= ~__ballot(match);
    }
}
