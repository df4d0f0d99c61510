// ppocar.hip -- HIP kernels (gfx950 / CDNA4) and the C-ABI of libppocar.so.  ONE translation unit: the kernels live in
// kernels/*.hpp (env_math, env_step, gae_sample, evaluation, track_maps, policy, rollout, update), included below in dependency order; this file
// holds the host side (handles, launch configuration, the extern "C" entry points of include/ppocar.h).  The track loader
// (track_json.cpp) and the compiler of the tracks into the env kernels' tables (track_tables.cpp) are host-only units of their own.
//
// Kernels
//   K1  env_step_kernel<T, RPL, MIXED>  the whole CarEnv.step transition (car_env.py:693-760) for one vector-env call,
//                                       with TransformReward and gymnasium's same-step auto-reset folded in
//                                       (train.py:65,68,185)
//   K2  env_reset_kernel<T>             CarEnv.reset for every env (car_env.py:605-691); reset_obs_kernel<T> computes
//                                       each track's constant reset observation once at create
//   K3  gae_kernel<ADV, BOOT, EPI, STEPS>   the reverse scan over the rollout buffer, one template for:
//       K3  <1,0,0,0>                   Buffer.calculate_advantages (buffer.py:36-64, pc_gae)
//       K3e <1,0,1,0> / <0,0,1,STEPS>   episode return, length, gates and laps on K3's rows (pc_gae_episodes) or alone
//                                       (pc_episode_stats, Buffer or step layout)
//       K3b <1,1,EPI,0>                 K3 with V(final observation) at time-limit truncations (pc_gae_bootstrap; EPI: K3e's statistics too)
//   K4  sample_kernel                   Categorical(logits).sample / log_prob / entropy (model.py:35-40)
//   K5  policy_kernel<KS, SPLIT, PREC>  Agent.get_action_and_value(x) of the rollout (model.py:34-41): both MLPs on the
//                                       matrix cores + the draw; policy_pack*_kernel build its LDS weight image
//   K6-8 ppo_gather / ppo_loss / clip_adam   non-GEMM pieces of a PPO minibatch step (train.py:230-261)
//   K9  rollout_kernel<KS, RPL, PREC, MODE> / K9s rollout_small_kernel<..., EPW>   the whole rollout (train.py:173-195) as one
//                                       persistent launch (large / small batches)
//   K10-12 ppo_fwdbwd / grad_reduce / adam (+ clip_adam_mb, the multi-rank step)   one PPO minibatch step without any library GEMM
//   K13 xchg_allreduce_kernel          the per-minibatch gradient all-reduce as a one-shot exchange over peer-mapped buffers (pc_xchg_*)
//   K14 first_episodes_kernel<STEPS>   the forward scan of the batched evaluation: each env's first episode and its lap times (pc_first_episodes)
//   K15 greedy_kernel                  argmax action + its log_prob, the deterministic sibling of K4 (pc_greedy)
//   K16 track_maps_kernel<STEPS, FIRST>   the observation rows of a rollout reduced to per-cell visit, speed and crash counters (pc_track_maps)
//
// Work decomposition of K1: an env is owned by G = 2^lg consecutive lanes of one
// wavefront ("lanes per env", chosen on the host from n_envs so the chip is filled); lane g of the
// group sweeps rays g, g+G, g+2G, ... (RPL = rays per lane, a template constant so the per-ray
// direction / running-minimum live in registers) against all wall segments.  Wall and gate
// segments are wave-uniform data: they are read with SCALAR loads (s_load_dwordx4 through the
// scalar cache) straight into SGPRs and enter the VALU as the one free SGPR operand per
// instruction -- cheaper than an LDS broadcast (no ds_read issue, no staging prologue, no
// barrier); a wave whose envs sit on different tracks runs the body once per distinct track
// (waterfall on the track id), so mixed-track batches stay correct.  Per-env reductions (any
// collision ray < 10 px) are DPP/shuffle butterflies inside the group; there is no LDS, no
// atomics and no inter-workgroup communication.  No MFMA: this is branchy fp32/fp64 geometry.
//
// Numerics
//   T = double  follows the reference's float64 operation order literally (Ray.cast :166-181,
//               np.linalg.norm's fused ddot tail, np.radians = x * (pi/180)); the translation unit
//               is compiled with -ffp-contract=off so nothing is fused behind our back.
//   T = float   the throughput path: float32 RAY GEOMETRY over a float64 kinematic state.  The
//               per-env scalar work (thrust, friction, clip, integrate, reward) is a few dozen
//               float64 operations and stays exactly the reference's; heading is an integer count
//               of 5-degree turns (Car.move_car only adds +-5.0, :440-442) looked up in a 72-entry
//               float64 cos/sin table built on the host; ray directions by float32 angle addition
//               with a per-ray table; ray casts in coordinates RELATIVE to the car, the difference
//               p1 - pos formed in float64 and then rounded (no pos+dir-pos cancellation,
//               :169-175), with u = cross(e,a)/cross(e,d) as the distance.  A float32 position
//               would by itself cost ~1e-4 px at x ~ 1280, i.e. most of the 1e-5 obs tolerance on
//               grazing rays (measured: DESIGN.md).
//               Rewards are bit-exact with the reference's float32(r * reward_scaling).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <climits>
#include <utility>
#include <vector>

#include "ppocar_internal.h"

// ---- the kernels, in dependency order (one translation unit: every kernel is compiled with this file's flags) ----
#include "kernels/env_math.hpp"
#include "kernels/env_step.hpp"
#include "kernels/car_step.hpp"
#include "kernels/observe.hpp"
#include "kernels/step_poses.hpp"
#include "kernels/safe_actions.hpp"
#include "kernels/sequences.hpp"
#include "kernels/sequences_value.hpp"
#include "kernels/gae_sample.hpp"
#include "kernels/cem.hpp"
#include "kernels/action_values.hpp"
#include "kernels/evaluation.hpp"
#include "kernels/track_maps.hpp"
#include "kernels/render.hpp"
#include "kernels/policy.hpp"
#include "kernels/rollout.hpp"
#include "kernels/env_steps.hpp"
#include "kernels/update.hpp"
#include "kernels/update_large.hpp"
#include "kernels/diagnostics.hpp"
#include "kernels/exchange.hpp"

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// Developer-only quick build (tools/ab_run.sh with -DPC_DEV_MIN=<mask>; never the product: the host layer refuses it like the
// ablation build): the dispatch tables keep only the benchmarked kernels -- bit 0: rollout_kernel<6, 9, 2, 3> (target), bit 1:
// rollout_small_kernel<6, 5, 2, 2, 16> (cfg1), bit 2: rollout_kernel<10, 17, 2, 1> (cfg2), bits 3 / 5: the literal form of bits 0 / 2
// for F64 handles, bit 4: rollout_f64_kernel<6, 9, 2> (the filter form), bit 6: the literal form of bit 1, bit 7: the 16-envs-per-wave
// form rollout_kernel<6, 5, 2, 3, false, 2> (big_track's layout), bit 8: its literal form; bits 0 / 3 also keep K1f's
// env_steps_fast_kernel<9, 7, ...> for F32 / F64 handles.  The fp16x2 policy kernels, the float32 env-step kernels and the update
// kernels stay -- so that one kernel experiment compiles in seconds instead of 75.  A plan whose instance the build left out is
// PC_ERR_UNSUPPORTED.
#ifdef PC_DEV_MIN
#define PC_FULL(...) return PC_ERR_UNSUPPORTED
#define PC_DEV(bit, ...) do { if constexpr (((PC_DEV_MIN) >> (bit)) & 1) { __VA_ARGS__; } else return PC_ERR_UNSUPPORTED; } while (0)
#else
#define PC_FULL(...) __VA_ARGS__
#define PC_DEV(bit, ...) __VA_ARGS__
#endif
static thread_local std::string g_hip_err;

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            g_hip_err = std::string(#expr) + ": " + hipGetErrorString(_e);                 \
            return PC_ERR_HIP;                                                             \
        }                                                                                  \
    } while (0)

namespace {

struct DeviceGuard {  // set the handle's device for the call, restore the caller's afterwards
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
        dev_ = dev;
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != dev_) (void)hipSetDevice(prev);
    }
    int dev_;
};

// device is an id the runtime knows.  Not part of DeviceGuard: the per-step entries construct a guard on every call and must not
// pay for hipGetDeviceCount there.
bool valid_device(int device) {
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess && count >= 1 && device >= 0 && device < count;
}

// a reward scale whose inverse decodes the episode statistics' rewards: finite, positive, with a finite inverse
bool valid_reward_scale(double s) { return std::isfinite(s) && s > 0.0 && std::isfinite(1.0 / s); }

// the actor / critic pair every MLP kernel is written for, D -> 256 -> A and D -> 256 -> 1, and its flat parameter count (update.hpp, K10-K12)
bool mlp_shape_ok(int D, int H, int A) { return H == 256 && A >= 1 && A <= 15 && D >= 1 && D <= 40; }
int64_t mlp_n_param(int D, int H, int A) { return 2 * ((int64_t)H * D + H) + (int64_t)A * H + A + H + 1; }
int64_t pad4(int64_t n) { return (n + 3) & ~(int64_t)3; }      // rows of parameters / partials start 16-byte aligned

// The compiled shapes of K10 / K10L.  CarEnv's (Discrete(9); 6 + 12 / 17 / 33 rays) have their action count and observation width compiled in
// -- and, in K10, the deferred clip + Adam prologue; every other shape takes the generic form of its width.  f(DMAX, AC, DC): integral_constants.
template <int V> using IntC = std::integral_constant<int, V>;
template <class F> void with_mlp_shape(int D, int A, F&& f) {
    if (A == 9 && D == 23) f(IntC<24>{}, IntC<9>{}, IntC<23>{});
    else if (A == 9 && D == 18) f(IntC<24>{}, IntC<9>{}, IntC<18>{});
    else if (A == 9 && D == 39) f(IntC<40>{}, IntC<9>{}, IntC<39>{});
    else if (D <= 24) f(IntC<24>{}, IntC<0>{}, IntC<0>{});
    else f(IntC<40>{}, IntC<0>{}, IntC<0>{});
}

// Launch a 512-thread kernel with `lds` bytes of dynamic LDS.  Its limit is raised to 160 KB once per (kernel, device), not on every
// call (pc_env_step is on the per-step path); device ids from 64 on have no bit in the set and raise it on every call.
template <auto K, typename... Args>
int launch_lds(int device, int blocks, size_t lds, hipStream_t st, Args... args) {
    static std::atomic<uint64_t> raised{0};     // bit d: done for device d
    const uint64_t bit = device < 64 ? 1ull << device : 0;
    if (!(raised.load(std::memory_order_acquire) & bit)) {
        HIPCHK(hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        raised.fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL(K, dim3(blocks), dim3(512), lds, st, args...);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

constexpr int kMenu[] = {1, 2, 3, 5, 6, 9, 12, 17, 33};  // rays-per-lane instantiations of K1

int pick_rpl(int need) {
    for (int m : kMenu)
        if (m >= need) return m;
    return -1;
}

// A device allocation that frees itself on destruction or reset (on the device that is current then: pc_env_destroy's guard).  upload =
// allocate + copy from the host, from elements of the same size (the table compiler's plain pair types stand for double2 / float2);
// nothing to upload leaves the buffer null.
template <typename T> struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    hipError_t alloc(size_t n) {
        reset();
        return hipMalloc((void**)&p, n * sizeof(T));
    }
    template <typename H> hipError_t upload(const H* src, size_t n) {
        static_assert(sizeof(H) == sizeof(T), "host and device elements of one layout");
        reset();
        if (!n) return hipSuccess;
        const hipError_t rc = alloc(n);
        return rc != hipSuccess ? rc : hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
    template <typename H> hipError_t upload(const std::vector<H>& v) { return upload(v.data(), v.size()); }
    operator T*() const { return p; }
};
static_assert(sizeof(PairD) == sizeof(double2) && sizeof(PairF) == sizeof(float2), "the table compiler's pairs are the device's by layout");

}  // namespace

// pc_rollout's dispatch options: per env handle (pc_env_set_option).  There is no process-wide state: a new handle starts from
// the member initialisers below.
struct RolloutOpts {
    int form = -1;        // -1 auto, 0 = 256 envs per workgroup, 1 = 32 envs per workgroup
    int rden = 1;         // stage the 1/den table in LDS when it fits (0: never; test / tuning knob)
    int epw_override = 0; // 0 = automatic, 16 / 32 / 128 / 256 = force (test knob)
    int fast = 1;         // the fast modes (LDS tables behind LDS pointers) when the shape allows them (0: never; A/B knob)
    int nv28 = 1;         // kernels compiled for a padded wall chain of 28 vertices (big_track.json) when every track of the batch has one
    int deinterleave = 1; // two tracks interleaved in evenly split blocks: the block's two waves de-interleave it (0: the per-track passes; A/B and test knob)
    int step_form = 0;    // pc_env_step / pc_env_step_many: 0 = automatic (pc_env_step: the table-driven form K1f from PC_STEP_FAST_MIN_ENVS envs
                          // on, where the shape has one; pc_env_step_many: wherever the shape has one), 1 = always the generic per-step kernel
                          // K1, 2 = K1f wherever the shape has one (any batch size)
};
constexpr int64_t PC_STEP_FAST_MIN_ENVS = 8192;   // below: K1's 8+ lanes per env fill the device as well as K1f's workgroups of 128 envs (call to call,
                                                  // tools/step_forms_probe.py: 11.2 against 12.5 us at 4096 envs, 13.6 = 13.6 at 8192, 21 against 15 at 16384, 34 against 21 at 65536)
constexpr int kDefaultPolicyPrecision = 2;   // pc_policy_create(precision = -1): 0 = fp32-input MFMA; split forms on the 16-bit matrix cores (need D <= 40, A <= 9): 1 = bf16 x 3, 2 = fp16 x 2

struct pc_env {
    int device = 0;
    RolloutOpts opt;
    int dtype = PC_DTYPE_F32;
    int64_t N = 0;
    int n_nominal = 12, R = 12, D = 18, n_tracks = 0;
    int lanes_override = 0;
    int lg = 0, rpl = 1, blocks = 0;
    // the host-only parts of the compiled track tables (track_tables.cpp): the headers (start_collides filled in from the device), what
    // dispatch needs to know of the batch's tracks, and -- further down -- the F64 rotation ids
    std::vector<TrackHdr> hdr_host;
    TrackFacts facts;
    // device buffers (each frees itself with the handle)
    DevBuf<double4> pv;
    DevBuf<int4> iv;
    DevBuf<double> rot;
    DevBuf<uint8_t> track_id;
    bool mixed = false;            // a track_id array was given (known before the geometry is chosen)
    bool track_blocks32 = false;   // mixed tracks: every aligned block of 32 envs holds ONE track (what pc_rollout needs)
    int track_block = 0;           // ... the largest of 256 / 128 / 64 / 32 for which that holds (0: none)
    bool track_bal64 = false, track_bal32 = false;   // two tracks, interleaved, every aligned block of 64 / 32 envs split evenly between them (and N a
                                                     // multiple of the block): the block's two waves de-interleave it (rollout_kernel's mode 7)
    DevBuf<TrackHdr> hdr;
    DevBuf<Seg> segs;
    DevBuf<Vtx> vtx;
    DevBuf<VtxP> vtxp;
    DevBuf<double2> headtab;
    DevBuf<float2> dirtab;
    DevBuf<float> rden;
    DevBuf<double2> dirtab64;
    DevBuf<SegD> seg64;
    DevBuf<F64Dir> dirhash;
    std::vector<std::unordered_map<uint64_t, int>> rot_ids;   // F64, host only: per track, rotation bits -> row of the rotation table (pc_env_set_state)
    std::vector<std::vector<int>> rot_depth;                  // F64, host only: per track and row, how many turns from start_rot reach it
    int last_kernel = 0;           // PC_KERNEL_*: what the last successful pc_rollout launched (pc_env_last_rollout_kernel)
    int last_step_kernel = 0;      // PC_STEP_*: what the last pc_env_step / pc_env_step_many launched (pc_env_last_step_kernel)
    bool f64_offgrid = false;      // F64: pc_env_set_state left an env whose episode can leave the rotation table (a rotation that is not a
                                   // row, or a row more turns from start_rot than the env's time step): the selector kernel needs rows
    DevBuf<float> reset_obs;
    // pc_render_*: the tracks' walls and gates in quarter pixels, each track's slice of them, and the rays' directions (host cos / sin);
    // render_err: why the handle's tracks cannot be rendered (empty: they can)
    DevBuf<int4> render_walls, render_gates;
    DevBuf<RenderTrack> render_trk;
    DevBuf<double2> render_dirs;
    std::string render_err;
    DevBuf<int> turn_row;          // F64: per track and turn count -PC_OBSERVE_TURNS .. PC_OBSERVE_TURNS, the row of the rotation table that holds
                                   // start_rot after that many turns one way (-1: none) -- pc_env_observe_poses' headings

    template <typename T> EnvParams<T> params() const {
        EnvParams<T> p;
        p.N = N;
        p.lg = lg;
        p.n_nominal = n_nominal;
        p.q = n_nominal / 4;
        p.nc = (n_nominal + p.q - 1) / p.q;
        p.step_deg = 360 / n_nominal;
        p.R = R;
        p.D = D;
        p.colbits = 0;
        for (int r = 0; r < 64 && r < n_nominal; r += n_nominal / 4) p.colbits |= 1ull << r;
        p.pv = pv;
        p.iv = iv;
        p.rot = rot;
        p.track_id = track_id;
        p.hdr = hdr;
        p.segs = segs;
        p.vtx = vtx;
        p.vtxp = vtxp;
        p.headtab = headtab;
        p.dirtab = dirtab;
        p.rden = rden;
        p.dirtab64 = dirtab64;
        p.seg64 = seg64;
        p.dirhash = dirhash;
        p.reset_obs = reset_obs;
        return p;
    }

    // lanes per env: fill ~4 waves per SIMD (256 CUs x 4 SIMDs x 64 lanes x 4) but never more
    // lanes than rays, and keep rays-per-lane inside the instantiated menu.
    int choose_geometry() {
        int G;
        if (lanes_override > 0) {
            G = lanes_override;
        } else {
            const int64_t target = 262144;
            G = 1;
            while (G < 64 && (int64_t)G * N < target && G < R) G <<= 1;
        }
        // F64 keeps 6 VGPRs per ray slot; a mixed-track batch reads every table through per-env pointers: 33 slots on one lane
        // spilled there (564 B of scratch) -- two lanes per env are the better geometry anyway
        const int max_rpl = (dtype == PC_DTYPE_F64 || mixed) ? 17 : 33;
        while (true) {
            const int need = (R + G - 1) / G;
            const int m = pick_rpl(need);
            if (m > 0 && m <= max_rpl) {
                rpl = m;
                break;
            }
            if (G >= 64) return PC_ERR_UNSUPPORTED;
            G <<= 1;
        }
        lg = 0;
        while ((1 << lg) < G) ++lg;
        const int64_t lanes = N << lg;
        blocks = (int)((lanes + 255) / 256);
        return PC_OK;
    }
};

template <typename T, int RPL>
static void launch_step(const pc_env* e, const int64_t* actions, double reward_scale, float* obs, float* reward, float* term,
                        float* trunc, int32_t* gates_passed, float* final_obs, hipStream_t st) {
    if (e->track_id) {
        if constexpr (RPL <= 17)     // (choose_geometry never gives a mixed-track batch more slots per lane)
            hipLaunchKernelGGL((env_step_kernel<T, RPL, true>), dim3(e->blocks), dim3(256), 0, st, e->params<T>(), actions,
                               reward_scale, obs, reward, term, trunc, gates_passed, final_obs);
    } else
        hipLaunchKernelGGL((env_step_kernel<T, RPL, false>), dim3(e->blocks), dim3(256), 0, st, e->params<T>(), actions,
                           reward_scale, obs, reward, term, trunc, gates_passed, final_obs);
}

// env_steps_fast_kernel's arguments, handed by steps_fast_launch to the instance it picks (`tab`: the TAB instance)
using StepsFastArgs = std::tuple<EnvParams<float>, const int64_t*, int, double, float*, float*, float*, float*, int, int, int32_t*, float*, int>;
template <int RPL, int SWP, bool LIT, bool TWO = false>
static int run_steps_fast(bool tab, int device, int blocks, size_t lds, hipStream_t st, const StepsFastArgs& args) {
    return std::apply([&](auto... a) {
        return tab ? launch_lds<env_steps_fast_kernel<RPL, SWP, true, LIT, TWO>>(device, blocks, lds, st, a...)
                   : launch_lds<env_steps_fast_kernel<RPL, SWP, false, LIT, TWO>>(device, blocks, lds, st, a...);
    }, args);
}

// K1f (env_steps_fast_kernel): T successive steps as one launch, where the shape has the table-driven form -- 12 / 16 / 32 nominal rays,
// every track's gather tables inside the LDS limits, a mixed batch in blocks of one track per workgroup; F64 handles: every track inside
// the selector's limits with its rotation table, every env's rotation on it (the conditions of pc_rollout's literal kernels).
// PC_ERR_UNSUPPORTED: no such form for this handle (the caller launches K1).  `table`: stage the 1/den table too (worth it for T > 1).
static int steps_fast_launch(pc_env* e, const int64_t* actions, int64_t T, double reward_scale, float* obs, float* reward, float* term,
                             float* trunc, bool table, hipStream_t st, int32_t* gates_passed = nullptr, float* final_obs = nullptr) {
    const bool f64 = e->dtype == PC_DTYPE_F64;
    const TrackFacts& f = e->facts;
    const bool rays12 = e->n_nominal == 12 && e->R == 12, rays16 = e->n_nominal == 16 && e->R == 17, rays32 = e->n_nominal == 32 && e->R == 33;
    if (!(rays12 || rays16 || rays32) || !e->opt.fast || T < 1 || T > INT_MAX) return PC_ERR_UNSUPPORTED;
    if ((gates_passed || final_obs) && T != 1) return PC_ERR_INVALID_ARG;      // (the optional outputs are pc_env_step's)
    const bool all_nv28 = e->opt.nv28 != 0 && f.nv28, all_loops = e->opt.nv28 != 0 && f.loops;
    const int epw = e->N <= 32768 ? 128 : 256;      // (one wave per SIMD on twice the workgroups up to 32768 envs, as pc_rollout's big form)
    // two tracks interleaved in evenly split blocks of 64 envs: de-interleaved by wave (the kernel's TWO form: 16 rays, the reference's track layouts)
    const bool two = e->track_id && e->track_block < epw && e->n_tracks == 2 && e->track_bal64 && all_loops && rays16 && e->opt.deinterleave;
    if (!f.tabs || f.max_G > TAB_MAX_GATES || f.max_nV > FT_VTX_MAX || (f64 && e->f64_offgrid) || (e->track_id && e->track_block < epw && !two))
        return PC_ERR_UNSUPPORTED;
    size_t lds = (size_t)(256 * e->D + (two ? 256 + 2 * ft_floats(false, true) : ft_floats(false, true))) * sizeof(float);
    const int rden_all = 361 * (two ? f.sum_nV : f.max_nV);
    const bool tab = table && f.rden && e->opt.rden != 0 && lds + (size_t)rden_all * sizeof(float) <= 160 * 1024;
    if (tab) lds += (size_t)rden_all * sizeof(float);
    const int ts_floats = two ? ((ft_floats(false, true) + (tab ? 361 * e->hdr_host[0].nV : 0) + 3) & ~3) : 0;
    const int blocks = (int)((e->N + epw - 1) / epw);
    const int vec_ok = ((e->N * e->D) % 4 == 0 && ((uintptr_t)obs & 15) == 0) ? 1 : 0;
    EnvParams<float> prm = e->params<float>();
    prm.lg = 1;
    int (*run)(bool, int, int, size_t, hipStream_t, const StepsFastArgs&) = nullptr;
    if (two) PC_FULL(run = f64 ? run_steps_fast<9, 5, true, true> : run_steps_fast<9, 5, false, true>);
    else if (rays16 && all_nv28) { if (f64) PC_DEV(3, run = run_steps_fast<9, 7, true>); else PC_DEV(0, run = run_steps_fast<9, 7, false>); }
    else if (rays16) PC_FULL(run = f64 ? run_steps_fast<9, 0, true> : run_steps_fast<9, 0, false>);
    else if (rays12) PC_FULL(run = f64 ? run_steps_fast<6, 0, true> : run_steps_fast<6, 0, false>);
    else PC_FULL(run = f64 ? run_steps_fast<17, 0, true> : run_steps_fast<17, 0, false>);
    const int rc = run(tab, e->device, blocks, lds, st, {prm, actions, (int)T, reward_scale, obs, reward, term, trunc, epw, vec_ok, gates_passed, final_obs,
                                                         ts_floats});
    if (rc != PC_OK) return rc;
    e->last_step_kernel = tab ? PC_STEP_K1F_TABLE : PC_STEP_K1F;
    return PC_OK;
}

// K1 (env_step_kernel): one step of every env, the generic kernel -- any ray count on the menu, any track, per-env track ids
static int step_generic_launch(pc_env* e, const int64_t* actions, double reward_scale, float* obs, float* reward, float* terminated,
                               float* truncated, int32_t* gates_passed, float* final_obs, hipStream_t st) {
    e->last_step_kernel = PC_STEP_K1;
#define PC_CASE(T, M)                                                                                        \
    case M:                                                                                                  \
        launch_step<T, M>(e, actions, reward_scale, obs, reward, terminated, truncated, gates_passed, final_obs, st); \
        break;
    if (e->dtype == PC_DTYPE_F64) {
        switch (e->rpl) {
#ifndef PC_DEV_MIN
            PC_CASE(double, 1) PC_CASE(double, 2) PC_CASE(double, 3) PC_CASE(double, 5) PC_CASE(double, 6)
            PC_CASE(double, 9) PC_CASE(double, 12) PC_CASE(double, 17)
#endif
            default: return PC_ERR_UNSUPPORTED;
        }
    } else {
        switch (e->rpl) {
            PC_CASE(float, 1) PC_CASE(float, 2) PC_CASE(float, 3) PC_CASE(float, 5) PC_CASE(float, 6)
            PC_CASE(float, 9) PC_CASE(float, 12) PC_CASE(float, 17) PC_CASE(float, 33)
            default: return PC_ERR_UNSUPPORTED;
        }
    }
#undef PC_CASE
    HIPCHK(hipGetLastError());
    return PC_OK;
}

// policy_kernel's arguments, handed by policy_act_impl to the instance it picks (`split`: the SPLIT instance)
using PolicyArgs = std::tuple<const float*, int64_t, int, int, const float*, uint64_t, uint64_t, const uint64_t*, int64_t*, float*, float*, float*, float*>;
template <int KS, int PREC, bool GR = false>
static int run_policy(bool split, int device, int blocks, size_t lds, hipStream_t st, const PolicyArgs& args) {
    return std::apply([&](auto... a) {
        return split ? launch_lds<policy_kernel<KS, true, PREC, GR>>(device, blocks, lds, st, a...)
                     : launch_lds<policy_kernel<KS, false, PREC, GR>>(device, blocks, lds, st, a...);
    }, args);
}
template <int PREC, bool GR = false>
static auto policy_run_for(int KS) { return KS == 5 ? run_policy<5, PREC, GR> : KS == 6 ? run_policy<6, PREC, GR> : run_policy<10, PREC, GR>; }

// one pc_rollout call's arguments, as the rollout kernels take them
struct RolloutIO {
    const float* image;
    int A, T;
    double reward_scale;
    uint64_t seed, offset;
    const uint64_t* offset_dev;
    float *obs_buf, *act_buf, *rew_buf, *val_buf, *term_buf, *trunc_buf, *logprob_buf, *next_obs, *next_term, *next_trunc, *last_value, *reward_sum;
    float* final_obs;   // pc_rollout_final_obs's [slots][N][D] (NULL: pc_rollout)
};

// what pc_rollout launches (plan_rollout): the kernel instance, through the launcher of its family (roll_big / roll_small / roll_f64), its grid
// and LDS bytes, and the launch's own arguments
struct RolloutPlan {
    int (*launch)(const pc_env*, const RolloutPlan&, const RolloutIO&, hipStream_t) = nullptr;
    int blocks = 0;
    size_t lds = 0;
    int rden_lds = 0;   // floats of the 1/den table staged in LDS (0: none)
    int epw = 0;        // envs per workgroup (rollout_kernel, rollout_f64_kernel)
    int lg = 1;         // EnvParams::lg
    int vec_ok = 0;     // 16-byte stores of the observation rows
    int kernel = 0;     // PC_KERNEL_*: what pc_env_last_rollout_kernel reports
};

// (GR: the kernel's greedy instance -- pc_rollout_greedy; the call's seed / offset are zeros it does not read)
template <int KS, int RPL, int PREC, int MODE, bool LIT = false, int LGE = 1, bool GR = false>
static int roll_big(const pc_env* e, const RolloutPlan& p, const RolloutIO& c, hipStream_t st) {
    EnvParams<float> prm = e->params<float>();
    prm.lg = p.lg;
    return launch_lds<rollout_kernel<KS, RPL, PREC, MODE, LIT, LGE, GR>>(e->device, p.blocks, p.lds, st, prm, c.image, c.A, c.T, c.reward_scale, c.seed,
                                                                      c.offset, c.offset_dev, c.obs_buf, c.act_buf, c.rew_buf, c.val_buf, c.term_buf,
                                                                      c.trunc_buf, c.logprob_buf, c.next_obs, c.next_term, c.next_trunc, p.rden_lds,
                                                                      p.epw, p.vec_ok, c.last_value, c.reward_sum, c.final_obs);
}

template <int KS, int RPL, int PREC, int MODE, int EPW, bool LIT = false, bool GR = false>
static int roll_small(const pc_env* e, const RolloutPlan& p, const RolloutIO& c, hipStream_t st) {
    EnvParams<float> prm = e->params<float>();
    prm.lg = p.lg;
    return launch_lds<rollout_small_kernel<KS, RPL, PREC, MODE, EPW, LIT, GR>>(e->device, p.blocks, p.lds, st, prm, c.image, c.A, c.T, c.reward_scale,
                                                                            c.seed, c.offset, c.offset_dev, c.obs_buf, c.act_buf, c.rew_buf, c.val_buf,
                                                                            c.term_buf, c.trunc_buf, c.logprob_buf, c.next_obs, c.next_term,
                                                                            c.next_trunc, p.rden_lds, p.vec_ok, c.last_value, c.reward_sum,
                                                                            c.final_obs);
}

template <int KS, int RPL, int PREC, bool SEL>
static int roll_f64(const pc_env* e, const RolloutPlan& p, const RolloutIO& c, hipStream_t st) {
    EnvParams<double> prm = e->params<double>();
    prm.lg = p.lg;
    return launch_lds<rollout_f64_kernel<KS, RPL, PREC, SEL>>(e->device, p.blocks, p.lds, st, prm, c.image, c.A, c.T, c.reward_scale, c.seed, c.offset,
                                                               c.offset_dev, c.obs_buf, c.act_buf, c.rew_buf, c.val_buf, c.term_buf, c.trunc_buf,
                                                               c.logprob_buf, c.next_obs, c.next_term, c.next_trunc, p.epw, c.last_value, c.reward_sum,
                                                               c.final_obs);
}

// rollout_kernel's generic mode (0) or fast mode (1; 2: with the 1/den table in LDS)
template <int KS, int RPL, int PREC>
static auto roll_big_mode(int mode) { return mode == 2 ? roll_big<KS, RPL, PREC, 2> : mode == 1 ? roll_big<KS, RPL, PREC, 1> : roll_big<KS, RPL, PREC, 0>; }

// rollout_small_kernel's generic mode (0) or fast mode (1: the small form takes the 1/den table as a run-time branch) at 32 envs per workgroup,
// or the fast mode at 16 (`epw16`: the split forms, at most five ray slots per lane)
template <int KS, int RPL, int PREC>
static auto roll_small_mode(int mode, bool epw16) {
    if constexpr (PREC != 0 && RPL <= 5)
        if (epw16) return roll_small<KS, RPL, PREC, 1, 16>;
    return mode ? roll_small<KS, RPL, PREC, 1, 32> : roll_small<KS, RPL, PREC, 0, 32>;
}

// pc_rollout_greedy's menu (F32 handles, fp16 x 2, Discrete(9), the table-driven modes): the greedy instance of the kernel plan_rollout
// picks for the sampled call -- md = the kernel's MODE (1 / 2, at 16 rays also the chain layouts 3 / 4 / 5).  Not in a developer quick build.
using RolloutLaunch = int (*)(const pc_env*, const RolloutPlan&, const RolloutIO&, hipStream_t);
static int greedy_big(int KS, int rpl, int md, RolloutLaunch& out) {
    if (KS == 5 && rpl == 6) PC_FULL(out = md == 2 ? roll_big<5, 6, 2, 2, false, 1, true> : roll_big<5, 6, 2, 1, false, 1, true>);
    else if (KS == 6 && rpl == 9)
        PC_FULL(out = md == 3 ? roll_big<6, 9, 2, 3, false, 1, true> : md == 5 ? roll_big<6, 9, 2, 5, false, 1, true>
                    : md == 4 ? roll_big<6, 9, 2, 4, false, 1, true> : md == 2 ? roll_big<6, 9, 2, 2, false, 1, true>
                              : roll_big<6, 9, 2, 1, false, 1, true>);
    else if (KS == 10 && rpl == 17) PC_FULL(out = (roll_big<10, 17, 2, 1, false, 1, true>));
    else return PC_ERR_UNSUPPORTED;
    return PC_OK;
}
static int greedy_small(int KS, int rpl, bool epw16, bool rden, RolloutLaunch& out) {
    if (KS == 5 && rpl == 3) PC_FULL(out = epw16 ? roll_small<5, 3, 2, 1, 16, false, true> : roll_small<5, 3, 2, 1, 32, false, true>);
    else if (KS == 6 && rpl == 5)
        PC_FULL(out = (epw16 && rden) ? roll_small<6, 5, 2, 2, 16, false, true> : epw16 ? roll_small<6, 5, 2, 1, 16, false, true>
                                      : roll_small<6, 5, 2, 1, 32, false, true>);
    else if (KS == 10 && rpl == 9) PC_FULL(out = (roll_small<10, 9, 2, 1, 32, false, true>));
    else return PC_ERR_UNSUPPORTED;
    return PC_OK;
}

// The state rows of a K17 / K20 / K21 / K22 call: the caller's arrays (px == nullptr: the STATE form, M = the handle's env count; an
// array the call does not have: nullptr, the kernels' default) and what the handle adds
template <bool RW>
static PoseRowsT<RW> pose_rows(const pc_env* e, RowPtr<RW, double> px, RowPtr<RW, double> py, RowPtr<RW, double> vx, RowPtr<RW, double> vy,
                               RowPtr<RW, int32_t> turns, RowPtr<RW, int32_t> next_gate, RowPtr<RW, int32_t> time_step,
                               const uint8_t* track_id, const uint8_t* active, int64_t M) {
    return {px, py, vx, vy, turns, next_gate, time_step, track_id, active, e->turn_row, M, e->n_tracks};
}
static PoseRows state_rows(const pc_env* e) { return pose_rows<false>(e, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, e->N); }

// 256-thread blocks for M rows of per_row lanes each: refused where the count does not fit a grid's x dimension (which also keeps
// M * per_row inside an int64_t)
static int lanes_grid(const int64_t M, const int64_t per_row, unsigned& blocks) {
    if (M > (int64_t)INT_MAX * 256 / per_row) return PC_ERR_UNSUPPORTED;
    blocks = (unsigned)((M * per_row + 255) / 256);
    return PC_OK;
}

// K17, K20: lanes per pose and the grid -- enough to fill the device at small M (the rule of choose_geometry), never more than rays, one at large M; the
// handle's pc_env_set_lanes_per_env override applies (every choice writes the same bytes: a ray's value does not depend on its lane)
static int pose_geometry(const pc_env* e, const int64_t M, int& lg, unsigned& blocks) {
    int G = 1;
    if (e->lanes_override > 0) {
        while (2 * G <= e->lanes_override && 2 * G <= e->R) G <<= 1;
    } else {
        while (2 * G <= e->R && G < 64 && (int64_t)G * M < 262144) G <<= 1;
    }
    lg = 0;
    while ((1 << lg) < G) ++lg;
    return lanes_grid(M, 1 << lg, blocks);
}

template <typename T, bool STATE>
static int observe_launch(const pc_env* e, ObservePoses q, float* obs, uint8_t* collides, hipStream_t st) {
    unsigned blocks;
    const int rc = pose_geometry(e, q.M, q.lg, blocks);
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL((observe_kernel<T, STATE>), dim3(blocks), dim3(256), 0, st, e->params<T>(), q, obs, collides);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

// K20: K17's geometry (a row's bytes do not depend on the lanes it gets either)
template <typename T>
static int step_poses_launch(const pc_env* e, StepPoses q, float* obs, hipStream_t st) {
    unsigned blocks;
    const int rc = pose_geometry(e, q.M, q.lg, blocks);
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL((step_poses_kernel<T>), dim3(blocks), dim3(256), 0, st, e->params<T>(), q, obs);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

// K21: one lane per (state, first action), 256 threads; a kernel per search depth (the recursion below the first action is compile-time)
template <typename T>
static int safe_actions_launch(const pc_env* e, const SafeActions& q, const int depth, uint8_t* safe, hipStream_t st) {
    unsigned blocks;
    const int rc = lanes_grid(q.M, 9, blocks);
    if (rc != PC_OK) return rc;
    const dim3 grid(blocks), block(256);
    switch (depth) {
        case 1: hipLaunchKernelGGL((safe_actions_kernel<T, 1>), grid, block, 0, st, e->params<T>(), q, safe); break;
        case 2: hipLaunchKernelGGL((safe_actions_kernel<T, 2>), grid, block, 0, st, e->params<T>(), q, safe); break;
        case 3: hipLaunchKernelGGL((safe_actions_kernel<T, 3>), grid, block, 0, st, e->params<T>(), q, safe); break;
        default: hipLaunchKernelGGL((safe_actions_kernel<T, 4>), grid, block, 0, st, e->params<T>(), q, safe); break;
    }
    HIPCHK(hipGetLastError());
    return PC_OK;
}

// K22: one lane per (state, sequence), 256 threads; then, where a best_* array is asked for, a wave per state over what the first stored
template <typename T>
static int sequences_launch(const pc_env* e, const Sequences& q, hipStream_t st) {
    unsigned blocks;
    const int rc = lanes_grid(q.M, q.K, blocks);
    if (rc != PC_OK) return rc;
    const EnvParams<T> p = e->params<T>();
    hipLaunchKernelGGL((sequences_kernel<T>), dim3(blocks), dim3(256), 0, st, p, q);
    HIPCHK(hipGetLastError());
    if (q.best_k || q.best_action || q.best_ret) {
        hipLaunchKernelGGL(sequences_best_kernel, dim3((unsigned)((q.M + 3) / 4)), dim3(256), 0, st, q, p.track_id);
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

// f(T{}) with T the handle's arithmetic: f is a generic lambda that names the launch's instance by decltype of its argument
template <typename F>
static int by_dtype(const pc_env* e, F&& f) {
    return e->dtype == PC_DTYPE_F64 ? f(double{}) : f(float{});
}

// K22's arguments past the states, shared by its two entry points: refused before the handle is looked at, else filled into q
static int sequences_args(Sequences& q, const uint8_t* actions, int64_t actions_state_stride, int K, int H, double reward_scale, double* ret,
                          int32_t* steps, uint8_t* status, int32_t* gates, int32_t* laps, int32_t* best_k, int64_t* best_action,
                          double* best_ret) {
    if (!actions || !ret || !steps || !status) return PC_ERR_INVALID_ARG;
    if (K < 1 || K > PC_SEQ_MAX_CANDIDATES) return PC_ERR_INVALID_ARG;
    if (H < 1 || H > PC_TIME_LIMIT) return PC_ERR_INVALID_ARG;
    if (actions_state_stride != 0 && actions_state_stride != (int64_t)H * K) return PC_ERR_INVALID_ARG;
    if (!std::isfinite(reward_scale)) return PC_ERR_INVALID_ARG;
    q.actions = actions; q.state_stride = actions_state_stride; q.K = K; q.H = H; q.reward_scale = reward_scale;
    q.ret = ret; q.steps = steps; q.status = status; q.gates = gates; q.laps = laps;
    q.best_k = best_k; q.best_action = best_action; q.best_ret = best_ret;
    return PC_OK;
}

extern "C" {

const char* pc_strerror(int code) {
    switch (code) {
        case PC_OK: return "ok";
        case PC_ERR_INVALID_ARG: return "invalid argument";
        case PC_ERR_IO: return "track file not found or unreadable";
        case PC_ERR_PARSE: return "track JSON malformed or schema violated";
        case PC_ERR_HIP: return "HIP runtime error";
        case PC_ERR_UNSUPPORTED: return "unsupported configuration";
        case PC_ERR_NO_DEVICE: return "no usable gfx950 device";
        case PC_ERR_TIMEOUT: return "a peer did not arrive at the gradient exchange (pc_xchg)";
        default: return "unknown error";
    }
}

const char* pc_last_hip_error(void) { return g_hip_err.c_str(); }

int pc_ray_count(int n) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (n < 4 || n > 360) return PC_ERR_INVALID_ARG;
    const int step = 360 / n;
    return (360 + step - 1) / step;  // len(range(0, 360, 360 // n)), car_env.py:269
}

int pc_track_load_json(const char* path, pc_track** out) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!path || !out) return PC_ERR_INVALID_ARG;
    std::unique_ptr<pc_track> t(new (std::nothrow) pc_track);
    if (!t) return PC_ERR_INVALID_ARG;
    const int rc = pc_internal_parse_track(path, t.get());
    if (rc != PC_OK) return rc;
    *out = t.release();
    return PC_OK;
}

int pc_track_from_arrays(const double* walls, int n_walls, const double* gates, int n_gates, double start_x, double start_y,
                         double start_angle_deg, pc_track** out) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!walls || !gates || n_walls < 1 || n_gates < 1 || !out) return PC_ERR_INVALID_ARG;
    pc_track* t = new (std::nothrow) pc_track;
    if (!t) return PC_ERR_INVALID_ARG;
    t->walls.assign(walls, walls + 4 * (size_t)n_walls);
    t->gates.assign(gates, gates + 4 * (size_t)n_gates);
    t->start_x = start_x;
    t->start_y = start_y;
    t->start_rot = start_angle_deg;
    *out = t;
    return PC_OK;
}

int pc_track_info(const pc_track* t, int* n_walls, int* n_gates, double* start) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!t) return PC_ERR_INVALID_ARG;
    if (n_walls) *n_walls = t->n_walls();
    if (n_gates) *n_gates = t->n_gates();
    if (start) {
        start[0] = t->start_x;
        start[1] = t->start_y;
        start[2] = t->start_rot;
    }
    return PC_OK;
}

int pc_track_geometry(const pc_track* t, double* walls, double* gates) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!t) return PC_ERR_INVALID_ARG;
    if (walls) memcpy(walls, t->walls.data(), t->walls.size() * sizeof(double));
    if (gates) memcpy(gates, t->gates.data(), t->gates.size() * sizeof(double));
    return PC_OK;
}

void pc_track_destroy(pc_track* t) { delete t; }

void pc_env_destroy(pc_env* e) {
    if (!e) return;
    DeviceGuard g(e->device);
    delete e;      // (the device buffers free themselves: DevBuf)
}

// pc_render_*: quantise the tracks' geometry (Q of include/ppocar.h) and build the rays' direction table with the host's cos / sin
// (math.radians' product, then libm: what tests/render_reference.py evaluates).  A track the integer bounds of kernels/render.hpp do not
// hold for leaves render_err set and the handle otherwise as it is: only the render calls refuse it.
static int render_prepare(pc_env* e, const pc_track* const* tracks) {
    struct Q4 { int x, y, z, w; };
    std::vector<Q4> walls, gates;
    std::vector<RenderTrack> trk((size_t)e->n_tracks);
    const auto quantise = [&](const std::vector<double>& src, std::vector<Q4>& dst, int k, const char* what) {
        for (size_t i = 0; i + 3 < src.size(); i += 4) {
            for (int j = 0; j < 4; ++j) {
                const double v = src[i + j], hi = (j & 1) ? 1744.0 : 2304.0;
                if (!(std::isfinite(v) && v >= -1024.0 && v <= hi) && e->render_err.empty())
                    e->render_err = "track " + std::to_string(k) + ": " + what + " " + std::to_string(i / 4) +
                                    " has a coordinate outside [-1024, 2304] x [-1024, 1744] px: it cannot be rendered";
            }
            if (e->render_err.empty()) dst.push_back({render_q(src[i]), render_q(src[i + 1]), render_q(src[i + 2]), render_q(src[i + 3])});
        }
    };
    for (int k = 0; k < e->n_tracks; ++k) {
        trk[k].wall_off = (int)walls.size();
        trk[k].gate_off = (int)gates.size();
        trk[k].n_walls = tracks[k]->n_walls();
        trk[k].n_gates = tracks[k]->n_gates();
        if (trk[k].n_gates > 255 && e->render_err.empty())
            e->render_err = "track " + std::to_string(k) + ": more than 255 reward gates: it cannot be rendered";
        quantise(tracks[k]->walls, walls, k, "wall");
        quantise(tracks[k]->gates, gates, k, "gate");
    }
    if (!e->render_err.empty()) return PC_OK;
    std::vector<PairD> dirs((size_t)e->R);
    const int step = 360 / e->n_nominal;
    for (int i = 0; i < e->R; ++i) {
        const double a = (double)(i * step) * (3.14159265358979323846 / 180.0);
        dirs[i] = {std::cos(a), std::sin(a)};
    }
    static_assert(sizeof(Q4) == sizeof(int4), "quantised segments are int4 by layout");
    HIPCHK(e->render_walls.upload(walls));
    HIPCHK(e->render_gates.upload(gates));
    HIPCHK(e->render_trk.upload(trk));
    HIPCHK(e->render_dirs.upload(dirs));
    return PC_OK;
}

// Compile the tracks and classify the track_id layout on the host (track_tables.cpp), upload the tables, and let the device fill in what
// it computes by the kernels' own arithmetic: the 1/den table, each track's reset observation and start_collides.
static int env_create_impl(pc_env* e, const pc_track* const* tracks, const uint8_t* track_id) {
    const bool f64 = e->dtype == PC_DTYPE_F64;
    TrackTables tt;
    const int rc = pc_internal_compile_tracks(tracks, e->n_tracks, e->n_nominal, e->R, e->dtype, tt, g_hip_err);
    if (rc != PC_OK) return rc;
    e->hdr_host = std::move(tt.hdr);
    e->rot_ids = std::move(tt.rot_ids);
    e->rot_depth = std::move(tt.rot_depth);
    e->facts = tt.facts;
    std::vector<int> turn_row;
    if (f64) {      // pc_env_observe_poses: the rotation a turn count means = start_rot after that many turns ONE way, each sum rounded
                    // (car_env.py:440-442); the table holds every one of them (its breadth-first depth is the count)
        turn_row.assign((size_t)e->n_tracks * (2 * PC_OBSERVE_TURNS + 1), -1);
        for (int k = 0; k < e->n_tracks; ++k) {
            if (e->hdr_host[k].rot_off < 0) continue;
            int* row = turn_row.data() + (size_t)k * (2 * PC_OBSERVE_TURNS + 1) + PC_OBSERVE_TURNS;
            for (const double step : {5.0, -5.0}) {
                double rot = e->hdr_host[k].start_rot;
                for (int t = 0; t <= PC_OBSERVE_TURNS; ++t, rot += step) {
                    uint64_t b;
                    std::memcpy(&b, &rot, 8);
                    const auto it = e->rot_ids[k].find(b);
                    row[step > 0 ? t : -t] = it != e->rot_ids[k].end() ? it->second : -1;
                }
            }
        }
    }
    // ---- device buffers
    const size_t N = (size_t)e->N;
    HIPCHK(e->pv.alloc(N));
    HIPCHK(e->iv.alloc(N));
    if (f64) HIPCHK(e->rot.alloc(N));
    if (track_id) {
        const TrackLayout l = pc_internal_classify_track_ids(track_id, e->N, e->n_tracks);
        e->track_block = l.track_block;
        e->track_blocks32 = l.blocks32;
        e->track_bal64 = l.bal64;
        e->track_bal32 = l.bal32;
        HIPCHK(e->track_id.upload(track_id, N));
    }
    HIPCHK(e->hdr.upload(e->hdr_host));
    HIPCHK(e->segs.upload(tt.segs));
    HIPCHK(e->vtx.upload(tt.vtx));
    HIPCHK(e->vtxp.upload(tt.vtxp));
    HIPCHK(e->headtab.upload(tt.headtab));
    HIPCHK(e->dirtab.upload(tt.dirtab));
    HIPCHK(e->dirtab64.upload(tt.dirtab64));
    HIPCHK(e->seg64.upload(tt.seg64));
    HIPCHK(e->dirhash.upload(tt.dirhash));
    HIPCHK(e->turn_row.upload(turn_row));
    HIPCHK(e->rden.alloc(tt.rden_floats ? tt.rden_floats : 1));
    hipLaunchKernelGGL(rden_build_kernel, dim3(64), dim3(256), 0, 0, e->params<float>(), e->n_tracks, e->rden.p);
    HIPCHK(hipGetLastError());
    HIPCHK(e->reset_obs.alloc((size_t)e->n_tracks * e->D));
    // ---- per-track reset observation + start_collides, computed on the device by the same arithmetic
    DevBuf<int> d_sc;
    HIPCHK(d_sc.alloc(e->n_tracks));
    const int rb = (e->n_tracks + 63) / 64;
    if (f64)
        hipLaunchKernelGGL(reset_obs_kernel<double>, dim3(rb), dim3(64), 0, 0, e->params<double>(), e->n_tracks, e->reset_obs.p, d_sc.p);
    else
        hipLaunchKernelGGL(reset_obs_kernel<float>, dim3(rb), dim3(64), 0, 0, e->params<float>(), e->n_tracks, e->reset_obs.p, d_sc.p);
    HIPCHK(hipGetLastError());
    std::vector<int> sc(e->n_tracks);
    HIPCHK(hipMemcpy(sc.data(), d_sc, e->n_tracks * sizeof(int), hipMemcpyDeviceToHost));
    for (int k = 0; k < e->n_tracks; ++k) e->hdr_host[k].start_collides = sc[k];
    HIPCHK(hipMemcpy(e->hdr, e->hdr_host.data(), e->n_tracks * sizeof(TrackHdr), hipMemcpyHostToDevice));
    return render_prepare(e, tracks);
}

int pc_env_create(int device, int64_t n_envs, int num_rays_nominal, const pc_track* const* tracks, int n_tracks,
                  const uint8_t* track_id, int dtype, pc_env** out) {
    if (!out || !tracks || n_tracks < 1 || n_tracks > 256 || n_envs < 1 || (dtype != PC_DTYPE_F32 && dtype != PC_DTYPE_F64))
        return PC_ERR_INVALID_ARG;
    if (num_rays_nominal < 4 || num_rays_nominal > 360) return PC_ERR_INVALID_ARG;
    for (int k = 0; k < n_tracks; ++k)
        if (!tracks[k] || tracks[k]->n_walls() < 1 || tracks[k]->n_gates() < 1) return PC_ERR_INVALID_ARG;
    if (track_id)
        for (int64_t i = 0; i < n_envs; ++i)
            if (track_id[i] >= n_tracks) return PC_ERR_INVALID_ARG;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    g_hip_err.clear();
    pc_env* e = new (std::nothrow) pc_env;
    if (!e) return PC_ERR_INVALID_ARG;
    e->device = device;
    e->dtype = dtype;
    e->N = n_envs;
    e->n_nominal = num_rays_nominal;
    e->R = pc_ray_count(num_rays_nominal);
    e->D = 6 + e->R;
    e->n_tracks = n_tracks;
    e->mixed = track_id != nullptr;
    int rc = e->choose_geometry();
    if (rc == PC_OK) rc = env_create_impl(e, tracks, track_id);
    if (rc != PC_OK) {
        pc_env_destroy(e);
        return rc;
    }
    *out = e;
    return PC_OK;
}

int pc_env_obs_dim(const pc_env* e) { return e ? e->D : PC_ERR_INVALID_ARG; }
int pc_env_num_actions(const pc_env* e) { return e ? 9 : PC_ERR_INVALID_ARG; }  // spaces.Discrete(9), car_env.py:525
int64_t pc_env_num_envs(const pc_env* e) { return e ? e->N : PC_ERR_INVALID_ARG; }

int pc_env_set_lanes_per_env(pc_env* e, int lanes) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e || lanes < 0 || lanes > 64 || (lanes & (lanes - 1))) return PC_ERR_INVALID_ARG;
    const int prev = e->lanes_override;
    e->lanes_override = lanes;
    const int rc = e->choose_geometry();
    if (rc != PC_OK) {
        e->lanes_override = prev;
        (void)e->choose_geometry();
    }
    return rc;
}

int pc_env_track_info(const pc_env* e, int track, int* n_walls, int* n_chain_vertices, int* n_scan_segments) {
    g_hip_err.clear();
    if (!e || track < 0 || track >= e->n_tracks) return PC_ERR_INVALID_ARG;
    const TrackHdr& h = e->hdr_host[track];
    if (n_walls) *n_walls = h.S;
    if (n_chain_vertices) *n_chain_vertices = h.n_chain;
    if (n_scan_segments) *n_scan_segments = (e->dtype == PC_DTYPE_F32 || h.sel_ok) ? h.n_scan : 0;
    return PC_OK;
}

int pc_env_last_rollout_kernel(const pc_env* e) { return e ? e->last_kernel : PC_ERR_INVALID_ARG; }

int pc_env_launch_info(const pc_env* e, int* lanes_per_env, int* rays_per_lane, int* blocks, int* threads) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;
    if (lanes_per_env) *lanes_per_env = 1 << e->lg;
    if (rays_per_lane) *rays_per_lane = e->rpl;
    if (blocks) *blocks = e->blocks;
    if (threads) *threads = 256;
    return PC_OK;
}

int pc_env_reset(pc_env* e, float* obs, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const int blocks = (int)((e->N + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    e->f64_offgrid = false;
    if (e->dtype == PC_DTYPE_F64)
        hipLaunchKernelGGL(env_reset_kernel<double>, dim3(blocks), dim3(256), 0, st, e->params<double>(), obs);
    else
        hipLaunchKernelGGL(env_reset_kernel<float>, dim3(blocks), dim3(256), 0, st, e->params<float>(), obs);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_env_step(pc_env* e, const int64_t* actions, double reward_scale, float* obs, float* reward, float* terminated,
                float* truncated, int32_t* gates_passed, float* final_obs, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e || !actions || !obs || !reward || !terminated || !truncated) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    // the table-driven form (K1f) where the handle has one
    if (e->opt.step_form == 2 || (e->opt.step_form == 0 && e->N >= PC_STEP_FAST_MIN_ENVS)) {
        const int rc = steps_fast_launch(e, actions, 1, reward_scale, obs, reward, terminated, truncated, false, st, gates_passed, final_obs);
        if (rc != PC_ERR_UNSUPPORTED) return rc;
    }
    return step_generic_launch(e, actions, reward_scale, obs, reward, terminated, truncated, gates_passed, final_obs, st);
}

int pc_env_step_many(pc_env* e, const int64_t* actions, int64_t T, double reward_scale, float* obs, float* reward, float* terminated,
                     float* truncated, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e || !actions || !obs || !reward || !terminated || !truncated || T < 1) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    if (e->opt.step_form != 1) {      // (one launch instead of T: worth it at any batch size)
        const int rc = steps_fast_launch(e, actions, T, reward_scale, obs, reward, terminated, truncated, T > 1, (hipStream_t)stream);
        if (rc != PC_ERR_UNSUPPORTED) return rc;
    }
    // no table-driven form for this handle: the same T steps as T launches of K1, row by row
    int rc = PC_OK;
    for (int64_t t = 0; t < T && rc == PC_OK; ++t)
        rc = step_generic_launch(e, actions + t * e->N, reward_scale, obs + t * e->N * e->D, reward + t * e->N, terminated + t * e->N, truncated + t * e->N,
                                 nullptr, nullptr, (hipStream_t)stream);
    return rc;
}

int pc_env_last_step_kernel(const pc_env* e) { return e ? e->last_step_kernel : PC_ERR_INVALID_ARG; }

int pc_env_observe_poses(const pc_env* e, const double* px, const double* py, const double* vx, const double* vy, const int32_t* turns,
                         const uint8_t* track_id, int64_t M, float* obs, uint8_t* collides, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e || !px || !py || !turns || !obs || M < 1) return PC_ERR_INVALID_ARG;      // (before the handle is looked at)
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const ObservePoses q{pose_rows<false>(e, px, py, vx, vy, turns, nullptr, nullptr, track_id, nullptr, M), 0};
    return by_dtype(e, [&](auto t) { return observe_launch<decltype(t), false>(e, q, obs, collides, (hipStream_t)stream); });
}

int pc_env_step_poses(const pc_env* e, double* px, double* py, double* vx, double* vy, int32_t* turns, int32_t* next_gate,
                      int32_t* time_step, const uint8_t* track_id, const int64_t* actions, const uint8_t* active, int64_t M,
                      double reward_scale, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated, uint8_t* gate,
                      void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;      // (this and the refusals below come before the handle is looked at)
    if (!px || !py || !vx || !vy || !turns || !next_gate || !time_step || !actions || !obs || !reward || !terminated || !truncated)
        return PC_ERR_INVALID_ARG;
    if (M < 1) return PC_ERR_INVALID_ARG;
    if (!std::isfinite(reward_scale)) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const StepPoses q{pose_rows<true>(e, px, py, vx, vy, turns, next_gate, time_step, track_id, active, M),
                      actions, reward, terminated, truncated, gate, reward_scale, 0};
    return by_dtype(e, [&](auto t) { return step_poses_launch<decltype(t)>(e, q, obs, (hipStream_t)stream); });
}

int pc_env_safe_actions(const pc_env* e, const double* px, const double* py, const double* vx, const double* vy, const int32_t* turns,
                        const int32_t* time_step, const uint8_t* track_id, const uint8_t* active, int64_t M, int depth, uint8_t* safe,
                        void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;      // (this and the refusals below come before the handle is looked at)
    if (!px || !py || !vx || !vy || !turns || !safe) return PC_ERR_INVALID_ARG;
    if (M < 1) return PC_ERR_INVALID_ARG;
    if (depth < 1 || depth > PC_SAFE_MAX_DEPTH) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const SafeActions q = pose_rows<false>(e, px, py, vx, vy, turns, nullptr, time_step, track_id, active, M);
    return by_dtype(e, [&](auto t) { return safe_actions_launch<decltype(t)>(e, q, depth, safe, (hipStream_t)stream); });
}

int pc_env_safe_actions_state(pc_env* e, int depth, uint8_t* safe, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e || !safe) return PC_ERR_INVALID_ARG;
    if (depth < 1 || depth > PC_SAFE_MAX_DEPTH) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const SafeActions q = state_rows(e);
    return by_dtype(e, [&](auto t) { return safe_actions_launch<decltype(t)>(e, q, depth, safe, (hipStream_t)stream); });
}

int pc_env_rollout_sequences(const pc_env* e, const double* px, const double* py, const double* vx, const double* vy, const int32_t* turns,
                             const int32_t* next_gate, const int32_t* time_step, const uint8_t* track_id, const uint8_t* active, int64_t M,
                             const uint8_t* actions, int64_t actions_state_stride, int K, int H, double reward_scale, double* ret,
                             int32_t* steps, uint8_t* status, int32_t* gates, int32_t* laps, int32_t* best_k, int64_t* best_action,
                             double* best_ret, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;      // (this and the refusals below come before the handle is looked at)
    if (!px || !py || !vx || !vy || !turns || M < 1) return PC_ERR_INVALID_ARG;
    Sequences q{};
    const int rc = sequences_args(q, actions, actions_state_stride, K, H, reward_scale, ret, steps, status, gates, laps, best_k, best_action, best_ret);
    if (rc != PC_OK) return rc;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    static_cast<PoseRows&>(q) = pose_rows<false>(e, px, py, vx, vy, turns, next_gate, time_step, track_id, active, M);
    return by_dtype(e, [&](auto t) { return sequences_launch<decltype(t)>(e, q, (hipStream_t)stream); });
}

int pc_env_rollout_sequences_state(pc_env* e, const uint8_t* actions, int64_t actions_state_stride, int K, int H, double reward_scale,
                                   double* ret, int32_t* steps, uint8_t* status, int32_t* gates, int32_t* laps, int32_t* best_k,
                                   int64_t* best_action, double* best_ret, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;
    Sequences q{};
    const int rc = sequences_args(q, actions, actions_state_stride, K, H, reward_scale, ret, steps, status, gates, laps, best_k, best_action, best_ret);
    if (rc != PC_OK) return rc;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    static_cast<PoseRows&>(q) = state_rows(e);
    return by_dtype(e, [&](auto t) { return sequences_launch<decltype(t)>(e, q, (hipStream_t)stream); });
}

int pc_env_observe(pc_env* e, float* obs, uint8_t* collides, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e || !obs) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const ObservePoses q{state_rows(e), 0};
    return by_dtype(e, [&](auto t) { return observe_launch<decltype(t), true>(e, q, obs, collides, (hipStream_t)stream); });
}

int pc_env_info(pc_env* e, int32_t* gates_passed, int32_t* time_passed, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    hipLaunchKernelGGL(env_info_kernel, dim3((unsigned)((e->N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, e->iv.p, e->N, gates_passed,
                       time_passed);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

#ifdef PC_DEV_MIN
int pc_build_ablate(void) { return 0x100 | PC_ABLATE; }     // a developer quick build is refused by the host layer like an ablation build
#else
int pc_build_ablate(void) { return PC_ABLATE; }
#endif

#ifdef PC_STAMPS
// developer build only (not declared in ppocar.h): copy the phase stamps of the last pc_rollout launch to the host
int pc_debug_read_stamps(unsigned long long* out, int n) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    const int total = 8 * STAMP_NT * STAMP_NPH;
    if (n < total) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), total * sizeof(unsigned long long)) != hipSuccess) return -3;
    return total;
}
int pc_debug_read_stamps_u(unsigned long long* out) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps_u), 16 * sizeof(unsigned long long)) != hipSuccess) return -3;
    return 16;
}
#endif

int pc_env_get_state(pc_env* e, double* px, double* py, double* vx, double* vy, double* rot, int64_t* time_step,
                     int64_t* next_gate, int64_t* passed) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const size_t N = (size_t)e->N;
    const bool f64 = e->dtype == PC_DTYPE_F64;
    HIPCHK(hipDeviceSynchronize());
    std::vector<int4> iv(N);
    HIPCHK(hipMemcpy(iv.data(), e->iv, N * sizeof(int4), hipMemcpyDeviceToHost));
    std::vector<double> pv(4 * N);
    HIPCHK(hipMemcpy(pv.data(), e->pv, 4 * N * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<double> r(N);
    std::vector<uint8_t> tid(N, 0);
    if (f64) HIPCHK(hipMemcpy(r.data(), e->rot, N * sizeof(double), hipMemcpyDeviceToHost));
    if (e->track_id) HIPCHK(hipMemcpy(tid.data(), e->track_id, N, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) {
        if (px) px[i] = pv[4 * i];
        if (py) py[i] = pv[4 * i + 1];
        if (vx) vx[i] = pv[4 * i + 2];
        if (vy) vy[i] = pv[4 * i + 3];
        if (rot) rot[i] = f64 ? r[i] : e->hdr_host[tid[i]].start_rot + 5.0 * iv[i].x;
        if (time_step) time_step[i] = iv[i].y;
        if (next_gate) next_gate[i] = iv[i].z;
        if (passed) passed[i] = iv[i].w;
    }
    return PC_OK;
}

int pc_env_set_state(pc_env* e, const double* px, const double* py, const double* vx, const double* vy, const double* rot,
                     const int64_t* time_step, const int64_t* next_gate, const int64_t* passed) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const size_t N = (size_t)e->N;
    const bool f64 = e->dtype == PC_DTYPE_F64;
    HIPCHK(hipDeviceSynchronize());
    std::vector<int4> iv(N);
    HIPCHK(hipMemcpy(iv.data(), e->iv, N * sizeof(int4), hipMemcpyDeviceToHost));
    std::vector<double> pv(4 * N);
    HIPCHK(hipMemcpy(pv.data(), e->pv, 4 * N * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<uint8_t> tid(N, 0);
    if (e->track_id) HIPCHK(hipMemcpy(tid.data(), e->track_id, N, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) {
        if (px) pv[4 * i] = px[i];
        if (py) pv[4 * i + 1] = py[i];
        if (vx) pv[4 * i + 2] = vx[i];
        if (vy) pv[4 * i + 3] = vy[i];
        if (rot && !f64) iv[i].x = (int)std::llround((rot[i] - e->hdr_host[tid[i]].start_rot) / 5.0);
        if (rot && f64) {      // the rotation's row of the track's rotation table, or -1: a value no episode reaches (the kernels then hash / evaluate it)
            uint64_t b;
            std::memcpy(&b, &rot[i], 8);
            const auto& ids = e->rot_ids[tid[i]];
            const auto it = ids.find(b);
            iv[i].x = it == ids.end() ? -1 : it->second;
        }
        if (time_step) iv[i].y = (int)time_step[i];
        if (next_gate) {
            if (next_gate[i] < 0 || next_gate[i] >= e->hdr_host[tid[i]].G) return PC_ERR_INVALID_ARG;
            iv[i].z = (int)next_gate[i];
        }
        if (passed) iv[i].w = (int)passed[i];
    }
    bool offgrid = false;
    if (f64) {      // can every env's episode stay inside its track's rotation table?  (what the selector kernel needs: rollout_f64_impl)
        for (size_t i = 0; i < N && !offgrid; ++i) {
            const std::vector<int>& depth = e->rot_depth[tid[i]];
            const int id = iv[i].x;
            offgrid = id < 0 || id >= (int)depth.size() || depth[id] > iv[i].y;
        }
        e->f64_offgrid = true;      // (until the copies below have succeeded: a half-written state must not reach the literal kernels)
    }
    HIPCHK(hipMemcpy(e->iv, iv.data(), N * sizeof(int4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->pv, pv.data(), 4 * N * sizeof(double), hipMemcpyHostToDevice));
    if (f64 && rot) HIPCHK(hipMemcpy(e->rot, rot, N * sizeof(double), hipMemcpyHostToDevice));
    if (f64) e->f64_offgrid = offgrid;
    return PC_OK;
}

// The reverse scan (K3, K3e, K3b, gae_kernel in kernels/gae_sample.hpp) for the four entries below, whose arguments are already
// checked.  The instance follows from the inputs: val (GAE), final_val (the truncation bootstrap), carry (episode statistics) and,
// without val, the layout.
static int gae_scan(int device, const float* rew, const float* val, const float* term, const float* trunc, const float* last_val,
                    const float* last_term, const float* last_trunc, const float* final_val, double gamma, double lam, int64_t T,
                    int64_t N, float* adv, float* ret, double reward_scale, double* carry, double* out, bool steps, void* stream) {
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    decltype(&gae_kernel<true, false, false, false>) k;
    if (!val) k = steps ? gae_kernel<false, false, true, true> : gae_kernel<false, false, true, false>;
    else if (final_val) k = carry ? gae_kernel<true, true, true, false> : gae_kernel<true, true, false, false>;
    else k = carry ? gae_kernel<true, false, true, false> : gae_kernel<true, false, false, false>;
    // gamma and gamma*lambda are Python floats that torch casts to float32 at the multiply
    hipLaunchKernelGGL(k, dim3((int)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rew, val, term, trunc, last_val, last_term,
                       last_trunc, (float)gamma, (float)(gamma * lam), T, N, adv, ret, final_val, carry ? 1.0 / reward_scale : 1.0,
                       carry, out);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_gae(int device, const float* rew, const float* val, const float* term, const float* trunc, const float* last_val,
           const float* last_term, const float* last_trunc, double gamma, double lam, int64_t T, int64_t N, float* adv,
           float* ret, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!rew || !val || !term || !trunc || !last_val || !last_term || !last_trunc || !adv || !ret || T < 1 || N < 1)
        return PC_ERR_INVALID_ARG;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    return gae_scan(device, rew, val, term, trunc, last_val, last_term, last_trunc, nullptr, gamma, lam, T, N, adv, ret, 1.0, nullptr,
                    nullptr, false, stream);
}

int pc_episode_stats(int device, const float* rew, const float* term, const float* trunc, const float* last_term,
                     const float* last_trunc, int64_t T, int64_t N, int layout, double reward_scale, double* carry, double* out,
                     void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!rew || !term || !trunc || !carry || !out || T < 1 || N < 1) return PC_ERR_INVALID_ARG;
    if (layout != PC_EPISODE_BUFFER && layout != PC_EPISODE_STEPS) return PC_ERR_INVALID_ARG;
    if (layout == PC_EPISODE_BUFFER && (!last_term || !last_trunc)) return PC_ERR_INVALID_ARG;
    if (!valid_reward_scale(reward_scale)) return PC_ERR_INVALID_ARG;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    return gae_scan(device, rew, nullptr, term, trunc, nullptr, last_term, last_trunc, nullptr, 0.0, 0.0, T, N, nullptr, nullptr,
                    reward_scale, carry, out, layout == PC_EPISODE_STEPS, stream);
}

int pc_gae_episodes(int device, const float* rew, const float* val, const float* term, const float* trunc, const float* last_val,
                    const float* last_term, const float* last_trunc, double gamma, double lam, int64_t T, int64_t N, float* adv,
                    float* ret, double reward_scale, double* carry, double* out, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!rew || !val || !term || !trunc || !last_val || !last_term || !last_trunc || !adv || !ret || !carry || !out || T < 1 || N < 1)
        return PC_ERR_INVALID_ARG;
    if (!valid_reward_scale(reward_scale)) return PC_ERR_INVALID_ARG;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    return gae_scan(device, rew, val, term, trunc, last_val, last_term, last_trunc, nullptr, gamma, lam, T, N, adv, ret, reward_scale,
                    carry, out, false, stream);
}

int pc_gae_bootstrap(int device, const float* rew, const float* val, const float* term, const float* trunc, const float* last_val,
                     const float* last_term, const float* last_trunc, const float* final_val, int64_t slots, double gamma, double lam,
                     int64_t T, int64_t N, float* adv, float* ret, double reward_scale, double* carry, double* out, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!rew || !val || !term || !trunc || !last_val || !last_term || !last_trunc || !final_val || !adv || !ret || T < 1 || N < 1)
        return PC_ERR_INVALID_ARG;
    if (slots < (T + PC_TIME_LIMIT - 1) / PC_TIME_LIMIT) return PC_ERR_INVALID_ARG;
    const bool epi = carry != nullptr || out != nullptr;
    if (epi && (!carry || !out)) return PC_ERR_INVALID_ARG;
    if (epi && !valid_reward_scale(reward_scale)) return PC_ERR_INVALID_ARG;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    return gae_scan(device, rew, val, term, trunc, last_val, last_term, last_trunc, final_val, gamma, lam, T, N, adv, ret, reward_scale,
                    carry, out, false, stream);
}

int pc_sample(int device, const float* logits, int64_t N, int A, uint64_t seed, uint64_t offset, int64_t* actions,
              float* logprob, float* entropy, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!logits || !actions || !logprob || N < 1 || A < 1) return PC_ERR_INVALID_ARG;
    if (A > 16) return PC_ERR_UNSUPPORTED;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const int blocks = (int)((N + 255) / 256);
    hipLaunchKernelGGL(sample_kernel<16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, N, A, seed, offset, actions,
                       logprob, entropy);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_first_episodes(int device, const float* rew, const float* term, const float* trunc, const float* last_term,
                      const float* last_trunc, int64_t T, int64_t N, int layout, double reward_scale, double* state, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!rew || !term || !trunc || !state || T < 1 || N < 1) return PC_ERR_INVALID_ARG;
    if (layout != PC_EPISODE_BUFFER && layout != PC_EPISODE_STEPS) return PC_ERR_INVALID_ARG;
    if (layout == PC_EPISODE_BUFFER && (!last_term || !last_trunc)) return PC_ERR_INVALID_ARG;
    if (!valid_reward_scale(reward_scale)) return PC_ERR_INVALID_ARG;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const auto k = layout == PC_EPISODE_STEPS ? first_episodes_kernel<true> : first_episodes_kernel<false>;
    hipLaunchKernelGGL(k, dim3((int)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rew, term, trunc, last_term, last_trunc, T, N,
                       1.0 / reward_scale, state);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_greedy(int device, const float* logits, int64_t N, int A, int64_t* actions, float* action_f32, float* logprob, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!logits || !actions || N < 1) return PC_ERR_INVALID_ARG;
    if (A < 1 || A > 16) return PC_ERR_UNSUPPORTED;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    hipLaunchKernelGGL(greedy_kernel<16>, dim3((int)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, N, A, actions,
                       action_f32, logprob);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

// K23 / K24: what both calls check of the table's shape, in the documented order
static bool cem_shape_ok(int64_t M, int H, int K) {
    return M >= 1 && H >= 1 && H <= PC_CEM_MAX_HORIZON && K >= 1 && K <= PC_SEQ_MAX_CANDIDATES;
}

int pc_cem_sample(int device, const uint32_t* weights, int64_t M, int H, int K, uint64_t seed, uint64_t offset, int const_columns,
                  const uint8_t* keep, const uint8_t* active, uint8_t* table, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!weights || !table) return PC_ERR_INVALID_ARG;
    if (!cem_shape_ok(M, H, K)) return PC_ERR_INVALID_ARG;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    unsigned blocks;
    const int rc = lanes_grid(M, (int64_t)H * K, blocks);
    if (rc != PC_OK) return rc;
    const CemSample q{weights, keep, active, table, M, H, K, const_columns, seed, offset};
    hipLaunchKernelGGL(cem_sample_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, q);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_cem_refit(int device, uint32_t* weights, const double* ret, const uint8_t* table, int64_t M, int H, int K, int E, int shift,
                 int w_min, const uint8_t* active, uint8_t* best_seq, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!weights || !ret || !table) return PC_ERR_INVALID_ARG;
    if (!cem_shape_ok(M, H, K)) return PC_ERR_INVALID_ARG;
    if (E < 1 || E > K) return PC_ERR_INVALID_ARG;
    if (shift < 0 || shift > 16) return PC_ERR_INVALID_ARG;
    if (w_min < 0 || w_min > (int)CEM_W_MAX) return PC_ERR_INVALID_ARG;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    if (M > INT_MAX) return PC_ERR_UNSUPPORTED;      // one workgroup per state
    const CemRefit q{weights, ret, table, active, best_seq, H, K, E, shift, (uint32_t)w_min};
    const CemLds lds{K, H};
    hipLaunchKernelGGL(cem_refit_kernel, dim3((unsigned)M), dim3(K <= 256 ? 64 : 256), lds.bytes(), (hipStream_t)stream, q);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

// K28: per-first-action returns of a score table, and the soft target over the actions that outlive their first step
int pc_sequences_action_values(int device, const double* ret, const uint8_t* actions, int64_t actions_state_stride, const int32_t* steps,
                               const uint8_t* status, const uint8_t* active, int64_t M, int K, int accumulate, double temperature, double* q,
                               int32_t* count, uint8_t* alive, float* target, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!ret || !actions || !q || !count || !alive) return PC_ERR_INVALID_ARG;
    if ((steps == nullptr) != (status == nullptr)) return PC_ERR_INVALID_ARG;
    if (M < 1) return PC_ERR_INVALID_ARG;
    if (K < 1 || K > PC_SEQ_MAX_CANDIDATES) return PC_ERR_INVALID_ARG;
    if (!std::isfinite(temperature) || temperature < 0.0) return PC_ERR_INVALID_ARG;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    if (M > INT_MAX) return PC_ERR_UNSUPPORTED;      // one wave per state
    const ActionValues p{ret, actions, actions_state_stride, steps, status, active, M, K, accumulate, temperature, q, count, alive, target};
    hipLaunchKernelGGL(action_values_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

// the compute-unit count of a device, asked once per device (ids from 64 on: 256).  The one cache of the library: two threads that
// race on an entry store the same value.
// pc_render_*: W and H of a scale on the list, false otherwise
static bool render_size(int scale, int* W, int* H) {
    if (scale != 1 && scale != 2 && scale != 4 && scale != 5 && scale != 8 && scale != 10) return false;
    *W = 1280 / scale;
    *H = 720 / scale;
    return true;
}
static int render_half_width(int nominal, int scale) { return std::max(nominal, 3 * scale); }

int pc_render_background(const pc_env* e, int scale, uint8_t* background, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    int W, H;
    if (!e || !background) return PC_ERR_INVALID_ARG;
    if (!render_size(scale, &W, &H)) return PC_ERR_INVALID_ARG;
    if ((uintptr_t)background & 3) return PC_ERR_INVALID_ARG;
    if (!e->render_err.empty()) {
        g_hip_err = e->render_err;
        return PC_ERR_UNSUPPORTED;
    }
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const int64_t blocks = ((int64_t)e->n_tracks * W * H + 255) / 256;      // (at most 256 tracks x 3600 blocks)
    hipLaunchKernelGGL(render_background_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, e->render_walls.p, e->render_gates.p,
                       e->render_trk.p, e->n_tracks, scale, W, H, render_half_width(10, scale), render_half_width(10, scale), background);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_render_frames(const pc_env* e, const float* obs, int64_t obs_ld, const int32_t* next_gate, const uint8_t* track_id, int64_t M,
                     int scale, const uint8_t* background, const uint8_t* palette, uint8_t* frames, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    static const uint8_t default_palette[PC_RENDER_COLORS][3] = {{24, 24, 28},  {58, 58, 66},   {235, 235, 235}, {60, 110, 60},      // render.py's COLORS, a road fill
                                                                 {90, 230, 90}, {70, 110, 200}, {250, 210, 70},  {240, 80, 60}};     // and a hit-disc colour
    int W, H;
    if (!e || !obs || !background || !frames || M < 1 || obs_ld < e->D) return PC_ERR_INVALID_ARG;
    if (!render_size(scale, &W, &H)) return PC_ERR_INVALID_ARG;
    if (((uintptr_t)background & 3) || ((uintptr_t)frames & 3)) return PC_ERR_INVALID_ARG;
    if (!e->render_err.empty()) {
        g_hip_err = e->render_err;
        return PC_ERR_UNSUPPORTED;
    }
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    RenderFrames a{};
    a.obs = obs; a.obs_ld = obs_ld; a.next_gate = next_gate; a.track_id = track_id;
    a.scale = scale; a.W = W; a.H = H;
    a.tiles_x = (W + PC_RENDER_TILE_W - 1) / PC_RENDER_TILE_W;
    a.tiles_y = (H + PC_RENDER_TILE_H - 1) / PC_RENDER_TILE_H;
    a.R = e->R; a.n_tracks = e->n_tracks;
    const int h_ray = render_half_width(2, scale), h_car = render_half_width(24, scale), h_gate = render_half_width(10, scale);
    a.h2_ray = h_ray * h_ray; a.h2_hit = 20 * 20; a.h2_car = h_car * h_car; a.h2_gate = h_gate * h_gate;
    a.h_max = std::max(h_car, 20);
    a.dirs = e->render_dirs; a.gates = e->render_gates; a.trk = e->render_trk; a.bg = background; a.frames = frames;
    const uint8_t (*pal)[3] = palette ? (const uint8_t (*)[3])palette : default_palette;
    for (int k = 0; k < PC_RENDER_COLORS; ++k) a.pal.rgb[k] = (uint32_t)pal[k][0] | ((uint32_t)pal[k][1] << 8) | ((uint32_t)pal[k][2] << 16);
    // a launch's grid stays below 2^32 threads: at most 2^24 - 1 workgroups, whole frames
    const int64_t tiles = (int64_t)a.tiles_x * a.tiles_y, per_launch = ((1ll << 24) - 1) / tiles;
    for (int64_t m0 = 0; m0 < M; m0 += per_launch) {
        a.m0 = m0;
        const int64_t n = std::min(per_launch, M - m0);
        hipLaunchKernelGGL(render_frames_kernel, dim3((unsigned)(n * tiles)), dim3(256), 0, (hipStream_t)stream, a);
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

static int device_cus(int device, int* out) {
    static std::atomic<int> n_cu[64];
    if (device < 0 || device >= 64) { *out = 256; return PC_OK; }
    int c = n_cu[device].load(std::memory_order_relaxed);
    if (c == 0) {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        c = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        n_cu[device].store(c, std::memory_order_relaxed);
    }
    *out = c;
    return PC_OK;
}

int pc_track_maps(int device, const float* obs, int64_t D, const float* term, const float* trunc, const float* last_term,
                  const float* last_trunc, int64_t T, int64_t N, int layout, const uint8_t* track_id, int n_tracks, int cell_px,
                  const double* first_state, int64_t* maps, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!obs || !term || !trunc || !maps || T < 1 || N < 1 || D < 4) return PC_ERR_INVALID_ARG;
    if (layout != PC_EPISODE_BUFFER && layout != PC_EPISODE_STEPS) return PC_ERR_INVALID_ARG;
    if (layout == PC_EPISODE_BUFFER && (!last_term || !last_trunc)) return PC_ERR_INVALID_ARG;
    if (n_tracks < 1 || n_tracks > 256) return PC_ERR_INVALID_ARG;
    if (cell_px < 4 || cell_px > 80 || 80 % cell_px != 0) return PC_ERR_INVALID_ARG;     // 4, 5, 8, 10, 16, 20, 40, 80
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    int cus = 256;
    if (const int rc = device_cus(device, &cus); rc != PC_OK) return rc;
    // one lane per env; without first_state the rows are cut so that about two workgroups per compute unit walk them side by side
    // (fewer, longer walks = fewer flushes of the LDS planes); with it every env's walk is the whole window
    const int64_t gx = (N + 1023) / 1024;
    int64_t gy = 1;
    if (!first_state) gy = std::clamp<int64_t>((2 * (int64_t)cus + gx - 1) / gx, 1, T);
    const int64_t rows = (T + gy - 1) / gy;
    gy = (T + rows - 1) / rows;
    const bool steps = layout == PC_EPISODE_STEPS;
    const auto k = first_state ? (steps ? track_maps_kernel<true, true> : track_maps_kernel<false, true>)
                               : (steps ? track_maps_kernel<true, false> : track_maps_kernel<false, false>);
    hipLaunchKernelGGL(k, dim3((unsigned)gx, (unsigned)gy), dim3(1024), 0, (hipStream_t)stream, obs, D, term, trunc, last_term, last_trunc,
                       T, N, rows, track_id, n_tracks, 1280 / cell_px, 720 / cell_px, first_state, (unsigned long long*)maps);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

static int policy_ks(int D) { return D <= 20 ? 5 : (D <= 24 ? 6 : 10); }
// Batches up to this size take the forms that cut the work of 32 envs over a whole workgroup (policy_kernel<SPLIT>,
// rollout_small_kernel): n_envs / 32 workgroups, so 16384 envs are two rounds of 256 -- about what the 128-env big form
// needs for anything up to 32768 envs.  The same bound for both kernels keeps the default per-step and persistent paths
// bit-identical.
// Up to this many envs the small form (32 or 16 envs per workgroup, the policy's hidden tiles split over the waves) beats 128-env
// workgroups of independent waves: its 256 workgroups of 32 envs fill the chip once; one env more starts a second round of them and the
// step takes 11.8 us where the big form takes 9.8 (tools/form_sweep.py, profiles/r5_form_sweep.txt: 16384 until round 5)
#define PC_SPLIT_MAX_ENVS 8192
// ... and up to this many the 16-envs-per-wave form of the big kernels (rollout_kernel<..., LGE = 2>: two waves per SIMD where 32-env
// waves leave one) beats them; above, 32-env waves come in pairs themselves
#define PC_MEDIUM_MAX_ENVS 32768
static const int64_t g_rollout_epw128_max = 32768;  // big form at or below this many envs: 128 envs (4 waves) per workgroup

// the arithmetic form a (D, A) shape gets when `requested` is asked for: the split forms cover D <= 40, A <= 9
static int policy_prec(int requested, int D, int A) { return (requested >= 1 && D <= 40 && A <= 9) ? requested : 0; }

// One policy step's configuration: shape, arithmetic form, work decomposition.  Immutable after creation; any number of
// handles with different forms can live in one process (each weight image belongs to the handle that packed it).
struct pc_policy {
    int device = 0, D = 0, H = 0, A = 0;
    int precision = 0;   // the form the shape actually gets (policy_prec)
    int split = -1;      // -1 automatic (by batch size), 0 never, 1 always
};

extern "C" {

int pc_policy_create(int device, int D, int H, int A, int precision, int split, pc_policy** out) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!out || precision < -1 || precision > 2 || split < -1 || split > 1) return PC_ERR_INVALID_ARG;
    if (!mlp_shape_ok(D, H, A)) return PC_ERR_UNSUPPORTED;  // the caller falls back to its own GEMMs
    pc_policy* p = new (std::nothrow) pc_policy;
    if (!p) return PC_ERR_INVALID_ARG;
    p->device = device;
    p->D = D;
    p->H = H;
    p->A = A;
    p->precision = policy_prec(precision < 0 ? kDefaultPolicyPrecision : precision, D, A);
    p->split = split;
    *out = p;
    return PC_OK;
}

void pc_policy_destroy(pc_policy* p) { delete p; }

int pc_policy_get(const pc_policy* p, int* precision, int* split, int64_t* image_floats) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!p) return PC_ERR_INVALID_ARG;
    if (precision) *precision = p->precision;
    if (split) *split = p->split;
    if (image_floats) *image_floats = p->precision ? polx_image_dwords(p->precision, pol_ng(policy_ks(p->D))) : pol_image_padded(policy_ks(p->D));
    return PC_OK;
}

int pc_env_set_option(pc_env* e, int option, int value) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;
    switch (option) {
        case PC_OPT_ROLLOUT_FORM:
            if (value < -1 || value > 4) return PC_ERR_INVALID_ARG;
            e->opt.rden = (value == 2 || value == 3) ? 0 : 1;
            e->opt.form = (value == 2 || value == 3) ? value - 2 : value;      // (4: the 16-envs-per-wave form, where the shape has one)
            return PC_OK;
        case PC_OPT_ROLLOUT_EPW:
            if (value != 0 && value != 16 && value != 32 && value != 128 && value != 256) return PC_ERR_INVALID_ARG;
            e->opt.epw_override = value;
            return PC_OK;
        case PC_OPT_ROLLOUT_FAST:
            if (value < 0 || value > 3) return PC_ERR_INVALID_ARG;
            e->opt.fast = value != 0;
            e->opt.nv28 = value == 1 || value == 3;
            e->opt.deinterleave = value != 3;
            return PC_OK;
        case PC_OPT_STEP_FORM:
            if (value < 0 || value > 2) return PC_ERR_INVALID_ARG;
            e->opt.step_form = value;
            return PC_OK;
        default: return PC_ERR_INVALID_ARG;
    }
}

int pc_env_get_option(const pc_env* e, int option, int* value) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e || !value) return PC_ERR_INVALID_ARG;
    switch (option) {
        case PC_OPT_ROLLOUT_FORM: *value = e->opt.form < 0 ? -1 : e->opt.form + (e->opt.rden ? 0 : 2); return PC_OK;
        case PC_OPT_ROLLOUT_EPW: *value = e->opt.epw_override; return PC_OK;
        case PC_OPT_ROLLOUT_FAST: *value = !e->opt.fast ? 0 : (!e->opt.nv28 ? 2 : (e->opt.deinterleave ? 1 : 3)); return PC_OK;
        case PC_OPT_STEP_FORM: *value = e->opt.step_form; return PC_OK;
        default: return PC_ERR_INVALID_ARG;
    }
}

}  // extern "C"

static int64_t policy_image_floats_impl(int prec, int D) { return prec ? polx_image_dwords(prec, pol_ng(policy_ks(D))) : pol_image_padded(policy_ks(D)); }

static int policy_pack_impl(int device, int prec, int D, int H, int A, const float* aW1, const float* ab1, const float* aW2, const float* ab2,
                            const float* cW1, const float* cb1, const float* cW2, const float* cb2, float* image, int* status, void* stream) {
    if (!aW1 || !ab1 || !aW2 || !ab2 || !cW1 || !cb1 || !cW2 || !cb2 || !image) return PC_ERR_INVALID_ARG;
    if (!mlp_shape_ok(D, H, A)) return PC_ERR_UNSUPPORTED;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    if (status) HIPCHK(hipMemsetAsync(status, 0, sizeof(int), (hipStream_t)stream));     // (forms without scaled domains leave it 0: no operand of theirs saturates)
#define PC_PACK(PRC, NGV)                                                                                                \
    hipLaunchKernelGGL((policy_pack16_kernel<PRC, NGV>), dim3(64), dim3(256), 0, (hipStream_t)stream, D, A, aW1, ab1, aW2, ab2, cW1, \
                       cb1, cW2, cb2, reinterpret_cast<unsigned*>(image), status)
    const int ng = pol_ng(policy_ks(D));
    if (prec == 1) { PC_FULL(if (ng == 5) PC_PACK(1, 5); else PC_PACK(1, 3)); }
    else if (prec == 2) { if (ng == 5) PC_PACK(2, 5); else PC_PACK(2, 3); }
#undef PC_PACK
    else
        PC_FULL(hipLaunchKernelGGL(policy_pack_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream, policy_ks(D), D, A, aW1, ab1, aW2, ab2,
                                   cW1, cb1, cW2, cb2, image));
    HIPCHK(hipGetLastError());
    return PC_OK;
}

static int policy_act_impl(int device, int prec, int split_mode, const float* obs, int64_t N, int D, int H, int A, const float* image, uint64_t seed,
                           uint64_t offset, const uint64_t* offset_dev, int64_t* action, float* action_f32, float* logprob, float* value,
                           float* logits_out, void* stream, bool greedy = false) {
    if (!obs || !image || !action || !logprob || !value || N < 1) return PC_ERR_INVALID_ARG;
    if (!mlp_shape_ok(D, H, A)) return PC_ERR_UNSUPPORTED;  // the caller falls back to its own GEMMs
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const int KS = policy_ks(D);
    const size_t lds = (size_t)((prec ? polx_image_dwords(prec, pol_ng(KS)) : pol_image_padded(KS)) + 8 * 32 * 20) * sizeof(float);
    int cus = 0;
    const int cu_rc = device_cus(device, &cus);
    if (cu_rc != PC_OK) return cu_rc;
    // too few 256-env workgroups to fill the chip: split the hidden tiles over the waves instead
    const bool split = split_mode < 0 ? N <= PC_SPLIT_MAX_ENVS : split_mode == 1;
    const int64_t chunks = split ? (N + 31) / 32 : (N + 255) / 256;
    const int blocks = (int)(chunks < cus ? chunks : cus);  // one ~100-KB-LDS workgroup per CU, persistent over env chunks
    hipStream_t st = (hipStream_t)stream;
    int (*run)(bool, int, int, size_t, hipStream_t, const PolicyArgs&) = nullptr;
    if (greedy) PC_FULL(run = prec == 2 ? policy_run_for<2, true>(KS) : prec == 1 ? policy_run_for<1, true>(KS) : policy_run_for<0, true>(KS));
    else if (prec == 2 && KS != 5) run = KS == 6 ? run_policy<6, 2> : run_policy<10, 2>;     // (what a quick build keeps)
    else PC_FULL(run = prec == 2 ? run_policy<5, 2> : prec == 1 ? policy_run_for<1>(KS) : policy_run_for<0>(KS));
    return run(split, device, blocks, lds, st, {obs, N, D, A, image, seed, offset, offset_dev, action, action_f32, logprob, value, logits_out});
}

int pc_policy_pack(const pc_policy* p, const float* aW1, const float* ab1, const float* aW2, const float* ab2, const float* cW1,
                   const float* cb1, const float* cW2, const float* cb2, float* image, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!p) return PC_ERR_INVALID_ARG;
    return policy_pack_impl(p->device, p->precision, p->D, p->H, p->A, aW1, ab1, aW2, ab2, cW1, cb1, cW2, cb2, image, nullptr, stream);
}

int pc_policy_pack_checked(const pc_policy* p, const float* aW1, const float* ab1, const float* aW2, const float* ab2, const float* cW1,
                           const float* cb1, const float* cW2, const float* cb2, float* image, int32_t* range_status, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!p || !range_status) return PC_ERR_INVALID_ARG;
    return policy_pack_impl(p->device, p->precision, p->D, p->H, p->A, aW1, ab1, aW2, ab2, cW1, cb1, cW2, cb2, image, range_status, stream);
}

int pc_policy_act(const pc_policy* p, const float* obs, int64_t N, const float* image, uint64_t seed, uint64_t offset,
                  const uint64_t* offset_dev, int64_t* action, float* action_f32, float* logprob, float* value, float* logits_out,
                  void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!p) return PC_ERR_INVALID_ARG;
    return policy_act_impl(p->device, p->precision, p->split, obs, N, p->D, p->H, p->A, image, seed, offset, offset_dev, action, action_f32,
                           logprob, value, logits_out, stream);
}

int pc_policy_act_greedy(const pc_policy* p, const float* obs, int64_t N, const float* image, int64_t* action, float* action_f32,
                         float* logprob, float* value, float* logits_out, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!p) return PC_ERR_INVALID_ARG;
    return policy_act_impl(p->device, p->precision, p->split, obs, N, p->D, p->H, p->A, image, 0, 0, nullptr, action, action_f32, logprob, value,
                           logits_out, stream, true);
}

}  // extern "C"

// K25, the policy step, K26: one lane per (state, sequence) as K22; pc_policy_act_greedy's launch over end_obs as M * K rows, its actions
// and log-probabilities into the caller's workspace; then a wave per state
static int64_t sequences_value_ws_bytes(const int64_t M, const int K) { return ((M * K * 12 + 15) / 16) * 16; }

template <typename T>
static int sequences_value_launch(const pc_env* e, const SequencesValue& q, const pc_policy* pp, const float* image, void* workspace,
                                  float* end_value, hipStream_t st) {
    unsigned blocks;
    const int rc = lanes_grid(q.M, q.K, blocks);
    if (rc != PC_OK) return rc;
    const EnvParams<T> p = e->params<T>();
    hipLaunchKernelGGL((sequences_value_kernel<T>), dim3(blocks), dim3(256), 0, st, p, q);
    HIPCHK(hipGetLastError());
    if (pp) {
        const int64_t N = q.M * q.K;
        int64_t* action = static_cast<int64_t*>(workspace);
        float* logprob = reinterpret_cast<float*>(action + N);
        const int prc = policy_act_impl(pp->device, pp->precision, pp->split, q.end_obs, N, pp->D, pp->H, pp->A, image, 0, 0, nullptr, action,
                                        nullptr, logprob, end_value, nullptr, st, true);
        if (prc != PC_OK) return prc;
    }
    if (pp || q.best_k || q.best_action || q.best_ret) {
        hipLaunchKernelGGL(sequences_combine_kernel, dim3((unsigned)((q.M + 3) / 4)), dim3(256), 0, st, q, p.track_id);
        HIPCHK(hipGetLastError());
    }
    return PC_OK;
}

// what the value form adds to sequences_args: refused before the handles are looked at, else filled into q
static int sequences_value_args(SequencesValue& q, double gamma, int bootstrap, const pc_policy* pp, const float* image, void* workspace,
                                float* end_obs, float* end_value, double* end_discount, double* ret_env) {
    if (!std::isfinite(gamma) || gamma < 0.0 || gamma > 1.0) return PC_ERR_INVALID_ARG;
    if (bootstrap != PC_SEQ_BOOTSTRAP_NONE && bootstrap != PC_SEQ_BOOTSTRAP_RUNNING && bootstrap != PC_SEQ_BOOTSTRAP_RUNNING_TRUNCATED)
        return PC_ERR_INVALID_ARG;
    if ((pp == nullptr) != (image == nullptr)) return PC_ERR_INVALID_ARG;
    if (bootstrap != PC_SEQ_BOOTSTRAP_NONE && !pp) return PC_ERR_INVALID_ARG;
    if (pp && (!end_obs || !end_value || !workspace)) return PC_ERR_INVALID_ARG;
    q.gamma = gamma; q.bootstrap = bootstrap;
    q.end_obs = end_obs; q.end_value = pp ? end_value : nullptr; q.end_discount = end_discount; q.ret_env = ret_env;
    return PC_OK;
}

extern "C" {

int64_t pc_env_rollout_sequences_value_workspace(int64_t M, int K) {
    if (M < 1 || K < 1 || K > PC_SEQ_MAX_CANDIDATES) return 0;
    return sequences_value_ws_bytes(M, K);
}

int pc_env_rollout_sequences_value(const pc_env* e, const double* px, const double* py, const double* vx, const double* vy, const int32_t* turns,
                                   const int32_t* next_gate, const int32_t* time_step, const uint8_t* track_id, const uint8_t* active, int64_t M,
                                   const uint8_t* actions, int64_t actions_state_stride, int K, int H, double reward_scale, double gamma,
                                   int bootstrap, const pc_policy* p, const float* image, void* workspace, double* ret, int32_t* steps,
                                   uint8_t* status, int32_t* gates, int32_t* laps, int32_t* best_k, int64_t* best_action, double* best_ret,
                                   float* end_obs, float* end_value, double* end_discount, double* ret_env, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;      // (this and the refusals below come before the handles are looked at)
    if (!px || !py || !vx || !vy || !turns || M < 1) return PC_ERR_INVALID_ARG;
    SequencesValue q{};
    int rc = sequences_args(q, actions, actions_state_stride, K, H, reward_scale, ret, steps, status, gates, laps, best_k, best_action, best_ret);
    if (rc == PC_OK) rc = sequences_value_args(q, gamma, bootstrap, p, image, workspace, end_obs, end_value, end_discount, ret_env);
    if (rc != PC_OK) return rc;
    if (p && (p->D != e->D || p->device != e->device)) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    static_cast<PoseRows&>(q) = pose_rows<false>(e, px, py, vx, vy, turns, next_gate, time_step, track_id, active, M);
    return by_dtype(e, [&](auto t) { return sequences_value_launch<decltype(t)>(e, q, p, image, workspace, end_value, (hipStream_t)stream); });
}

int pc_env_rollout_sequences_value_state(pc_env* e, const uint8_t* actions, int64_t actions_state_stride, int K, int H, double reward_scale,
                                         double gamma, int bootstrap, const pc_policy* p, const float* image, void* workspace, double* ret,
                                         int32_t* steps, uint8_t* status, int32_t* gates, int32_t* laps, int32_t* best_k, int64_t* best_action,
                                         double* best_ret, float* end_obs, float* end_value, double* end_discount, double* ret_env,
                                         void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!e) return PC_ERR_INVALID_ARG;
    SequencesValue q{};
    int rc = sequences_args(q, actions, actions_state_stride, K, H, reward_scale, ret, steps, status, gates, laps, best_k, best_action, best_ret);
    if (rc == PC_OK) rc = sequences_value_args(q, gamma, bootstrap, p, image, workspace, end_obs, end_value, end_discount, ret_env);
    if (rc != PC_OK) return rc;
    if (p && (p->D != e->D || p->device != e->device)) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    static_cast<PoseRows&>(q) = state_rows(e);
    return by_dtype(e, [&](auto t) { return sequences_value_launch<decltype(t)>(e, q, p, image, workspace, end_value, (hipStream_t)stream); });
}

int pc_ppo_gather(int device, const int64_t* idx, int B, int D, const float* obs, const float* act, const float* logprob,
                  const float* adv, const float* ret, float* o_obs, float* o_act, float* o_logprob, float* o_adv, float* o_ret,
                  void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!idx || !obs || !act || !logprob || !adv || !ret || !o_obs || !o_act || !o_logprob || !o_adv || !o_ret || B < 1 || D < 1)
        return PC_ERR_INVALID_ARG;
    if (device < 0) return PC_ERR_NO_DEVICE;      // (a machine without a device has no current one to tell -1 from: DeviceGuard would pass it)
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const int total = B * (D + 4);
    hipLaunchKernelGGL(ppo_gather_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, idx, B, D, obs, act,
                       logprob, adv, ret, o_obs, o_act, o_logprob, o_adv, o_ret);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

// 1.5 x target_kl as the kernels' float threshold (SB3's rule); target_kl <= 0 or NaN: 0 = never stop
static float kl_stop_of(double target_kl) { return target_kl > 0.0 ? (float)(1.5 * target_kl) : 0.0f; }

int pc_ppo_loss(int device, const float* logits, const float* values, const float* act, const float* old_logprob,
                const float* adv, const float* ret, int B, int A, double clip_ratio, double vf_coef, double ent_coef,
                float* dlogits, float* dvalues, float* metrics, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!logits || !values || !act || !old_logprob || !adv || !ret || !dlogits || !dvalues || !metrics) return PC_ERR_INVALID_ARG;
    if (B < 2 || B > 1024 || A < 1 || A > 16) return PC_ERR_UNSUPPORTED;
    if (device < 0) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const int threads = ((B + 63) / 64) * 64;
    hipLaunchKernelGGL((ppo_loss_kernel<16, false>), dim3(1), dim3(threads), 0, (hipStream_t)stream, logits, values, act, old_logprob, adv,
                       ret, B, A, (float)clip_ratio, (float)vf_coef, (float)ent_coef, dlogits, dvalues, metrics, nullptr, 0.0f);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_clip_adam(int device, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* step_count, const float* lr_dev,
                 int64_t n, double max_norm, double grad_scale, double beta1, double beta2, double eps, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step_count || !lr_dev || n < 1 || n > (1 << 26)) return PC_ERR_INVALID_ARG;
    if (device < 0) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    hipLaunchKernelGGL(clip_adam_kernel<false>, dim3(1), dim3(1024), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, step_count,
                       lr_dev, (int)n, (float)max_norm, (float)grad_scale, (float)beta1, (float)beta2, (float)eps, nullptr);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_ppo_loss_diag(int device, const float* logits, const float* values, const float* act, const float* old_logprob,
                     const float* adv, const float* ret, int B, int A, double clip_ratio, double vf_coef, double ent_coef,
                     float* dlogits, float* dvalues, float* metrics, float* diag, double target_kl, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!logits || !values || !act || !old_logprob || !adv || !ret || !dlogits || !dvalues || !metrics || !diag) return PC_ERR_INVALID_ARG;
    if (B < 2 || B > 1024 || A < 1 || A > 16) return PC_ERR_UNSUPPORTED;
    if (device < 0) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const int threads = ((B + 63) / 64) * 64;
    hipLaunchKernelGGL((ppo_loss_kernel<16, true>), dim3(1), dim3(threads), 0, (hipStream_t)stream, logits, values, act, old_logprob, adv,
                       ret, B, A, (float)clip_ratio, (float)vf_coef, (float)ent_coef, dlogits, dvalues, metrics, diag, kl_stop_of(target_kl));
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_clip_adam_diag(int device, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* step_count, const float* lr_dev,
                      int64_t n, double max_norm, double grad_scale, double beta1, double beta2, double eps, const float* diag,
                      void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step_count || !lr_dev || !diag || n < 1 || n > (1 << 26)) return PC_ERR_INVALID_ARG;
    if (device < 0) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    hipLaunchKernelGGL(clip_adam_kernel<true>, dim3(1), dim3(1024), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, step_count,
                       lr_dev, (int)n, (float)max_norm, (float)grad_scale, (float)beta1, (float)beta2, (float)eps, diag);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int64_t pc_explained_variance_workspace_doubles(int device) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    (void)device;        // (the same bound on every device: the grid is min(needed, 8 per compute unit, this))
    return 5 * (int64_t)PC_EV_MAX_BLOCKS;
}

int pc_explained_variance(int device, const float* val, const float* ret, int64_t M, double* workspace, double* out, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!val || !ret || !workspace || !out || M < 1) return PC_ERR_INVALID_ARG;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    int cus = 0;
    const int cu_rc = device_cus(device, &cus);
    if (cu_rc != PC_OK) return cu_rc;
    const int64_t cap = std::min<int64_t>(8 * (int64_t)cus, PC_EV_MAX_BLOCKS);
    const int64_t need = (M + 8 * 256 - 1) / (8 * 256);      // 8 samples per thread and pass
    const int blocks = (int)std::max<int64_t>(1, std::min(need, cap));
    const int vec = (((uintptr_t)val | (uintptr_t)ret) & 15) == 0;
    hipLaunchKernelGGL(explained_variance_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, val, ret, M, vec, workspace);
    hipLaunchKernelGGL(explained_variance_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, workspace, blocks, out);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_clip_adam_advanced(int device, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* step_count,
                          const float* lr_dev, int64_t n, double max_norm, double grad_scale, double beta1, double beta2, double eps,
                          void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step_count || !lr_dev || n < 1 || n > (1 << 26)) return PC_ERR_INVALID_ARG;
    if (device < 0) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    hipLaunchKernelGGL(clip_adam_mb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, const_cast<float*>(grad),
                       exp_avg, exp_avg_sq, step_count, lr_dev, (int)n, (float)max_norm, (float)grad_scale, (float)beta1, (float)beta2, (float)eps);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

// pc_rollout's choice for this handle and call: PC_OK with `p` filled, or PC_ERR_UNSUPPORTED (the caller then runs the per-step kernels,
// which fill the same buffers bit for bit).  The rules run in order of preference.  F32 and F64 handles share the two-track and the
// 16-envs-per-wave forms (LIT: an F64 handle, whose env step is the literal form); every other rule belongs to one dtype.
// `greedy` (pc_rollout_greedy): the same form as for the sampled call on this handle -- kernel id, envs per workgroup, blocks, LDS bytes, 1/den
// table -- where that form is on the greedy menu (greedy_big / greedy_small and the 16-envs-per-wave form), else PC_ERR_UNSUPPORTED.
static int plan_rollout(const pc_env* e, int prec, int A, int vec_ok, bool greedy, RolloutPlan& p) {
    const bool lit = e->dtype == PC_DTYPE_F64;
    if (lit ? A != 9 : (A < 1 || A > 15)) return PC_ERR_UNSUPPORTED;
    if (greedy && (lit || prec != 2 || A != 9)) return PC_ERR_UNSUPPORTED;
    const RolloutOpts& o = e->opt;
    const TrackFacts& f = e->facts;
    const bool all_nv28 = o.nv28 != 0 && f.nv28, all_loops = o.nv28 != 0 && f.loops;
    // mixed tracks interleaved inside a wave (no aligned block of 32 envs on one track; car_env.py:621-628 makes that legal): F32 handles
    // take the BIG form's generic mode, whose env step runs once per distinct track id of a wave (K1's waterfall), F64 handles the generic
    // kernel K9d -- the fast and literal forms stage ONE track's tables per workgroup, and the small form's sweep parts meet across
    // workgroup barriers that a per-wave loop cannot contain
    const bool interleaved = e->track_id && !e->track_blocks32;
    if (greedy && interleaved) return PC_ERR_UNSUPPORTED;     // (the two-track modes 6 / 7 and the generic mode: not on the greedy menu)
    const int KS = policy_ks(e->D);
    const int img = prec ? polx_image_dwords(prec, pol_ng(KS)) : pol_image_padded(KS);
    // 12 / 16 / 32 nominal rays: 12 / 17 / 33 actual, D = 18 / 23 / 39 (KS = 5 / 6 / 10), 6 / 9 / 17 ray slots on two lanes per env
    const bool rays12 = e->n_nominal == 12, rays16 = e->n_nominal == 16, rays32 = e->n_nominal == 32;
    const int epw = o.epw_override >= 128 ? o.epw_override : (e->N <= g_rollout_epw128_max ? 128 : 256);   // big form: envs per workgroup
    p.epw = epw;
    p.blocks = (int)((e->N + epw - 1) / epw);
    p.vec_ok = vec_ok;
    if (lit && prec == 0) {
        // THE STRICTEST CELL: float64 env (the literal form) AND the policy GEMMs as the exact fp32 chain (v_mfma_f32_16x16x4_f32) -- every
        // number of the rollout in the reference's own arithmetic -- as one persistent launch: K9's literal form with the fp32 weight
        // image (16 -> 17 rays, the big form, the generic sweeps; the fp32 image leaves no room for the 1/den table, as for F32
        // handles).  Other shapes: the per-step kernels.
        p.lds = (size_t)k9_fast_lds_floats(img, 32, e->D, true, 0) * sizeof(float);
        if (!(f.tabs && rays16 && !e->f64_offgrid && !interleaved && e->D >= 17 && f.max_G <= TAB_MAX_GATES && f.max_nV <= FT_VTX_MAX && o.fast &&
              (!e->track_id || e->track_block >= epw) && p.lds <= 160 * 1024))
            return PC_ERR_UNSUPPORTED;
        PC_FULL(p.launch = roll_big<6, 9, 0, 1, true>);
        p.kernel = PC_KERNEL_K9_LITERAL;
        return PC_OK;
    }
    if (!lit && interleaved && o.form == 1) return PC_ERR_UNSUPPORTED;
    const bool want_m = o.form == 4 || (o.form < 0 && o.epw_override == 0 && e->N > PC_SPLIT_MAX_ENVS && e->N <= PC_MEDIUM_MAX_ENVS);
    // ---- tracks interleaved inside the waves, the reference's own pair (two tracks, each two equal loops of 13 or 9 chain vertices,
    // 16 -> 17 rays, fp16 x 2): both tracks' tables in LDS, the table-driven env step once per track of a wave (mode 6); where every block
    // is split evenly between the two, the block's two waves de-interleave it (mode 7).  16 envs per wave (4 lanes per env) where the
    // 16-envs-per-wave form is wanted, as for single-track and block-mixed batches of that size: two waves on every SIMD
    if (interleaved && o.fast && o.nv28 != 0 && e->n_tracks == 2 && rays16 && A == 9 && prec == 2 && e->D >= 17 && e->D <= 40 && f.loops &&
        f.max_nV <= FT_VTX_MAX && f.max_G <= TAB_MAX_GATES && (!lit || (f.tabs && !e->f64_offgrid))) {
        const int ts6 = (ft_floats(false, true) + 3) & ~3;
        const size_t lds6 = (size_t)k9_fast_lds_floats(img, 32, e->D, true, ts6) * sizeof(float);
        if (lds6 <= 160 * 1024 && want_m) {
            if (e->track_bal32 && o.deinterleave) PC_FULL(p.launch = lit ? roll_big<6, 5, 2, 7, true, 2> : roll_big<6, 5, 2, 7, false, 2>);
            else PC_FULL(p.launch = lit ? roll_big<6, 5, 2, 6, true, 2> : roll_big<6, 5, 2, 6, false, 2>);
            p.blocks = (int)((e->N + 127) / 128);
            p.lds = (size_t)k9_fast_lds_floats(img, 16, e->D, true, ts6) * sizeof(float);
            p.epw = 128;
            p.lg = 2;
            p.kernel = lit ? PC_KERNEL_K9M_LITERAL : PC_KERNEL_K9M;
            return PC_OK;
        }
        if (lds6 <= 160 * 1024) {
            if (e->track_bal64 && o.deinterleave) PC_FULL(p.launch = lit ? roll_big<6, 9, 2, 7, true> : roll_big<6, 9, 2, 7>);
            else PC_FULL(p.launch = lit ? roll_big<6, 9, 2, 6, true> : roll_big<6, 9, 2, 6>);
            p.lds = lds6;
            p.kernel = lit ? PC_KERNEL_K9_LITERAL : PC_KERNEL_K9;
            return PC_OK;
        }
    }
    // K9's literal form (F64 handles) stages the 1/den table where it fits: 12 / 16 rays up to ~36 chain vertices (33 rays: no room -- the
    // sweep forms 1/den itself, as for F32 handles)
    int rden_sel = rays32 ? 0 : 361 * f.max_nV;
    size_t lds_sel = (size_t)k9_fast_lds_floats(img, 32, e->D, !rays32, rden_sel) * sizeof(float);
    if (rden_sel && lds_sel > 160 * 1024) {
        rden_sel = 0;
        lds_sel = (size_t)k9_fast_lds_floats(img, 32, e->D, true, 0) * sizeof(float);
    }
    // ---- the 16-envs-per-wave form (rollout_kernel<6, 5, 2, MD, LIT, 2>): 17 rays, fp16 x 2, the chain-packed sweeps' track layouts, the
    // 1/den table in LDS; automatic between PC_SPLIT_MAX_ENVS and PC_MEDIUM_MAX_ENVS envs, PC_OPT_ROLLOUT_FORM = 4 at any size.  (Never
    // a batch of the small form, whose rules below it therefore does not overtake.)
    {
        const int rden_m = 361 * f.max_nV;
        const size_t lds_m = (size_t)k9_fast_lds_floats(img, 16, e->D, true, rden_m) * sizeof(float);
        if (want_m && rays16 && prec == 2 && A == 9 && e->D >= 17 && e->D <= 40 && f.max_G <= TAB_MAX_GATES && f.max_nV <= FT_VTX_MAX && o.fast &&
            o.rden != 0 && (all_nv28 || all_loops) && (!e->track_id || e->track_block >= 128) && lds_m <= 160 * 1024 &&
            (!lit || (f.tabs && !e->f64_offgrid && (!e->track_id || e->track_block >= epw) && lds_sel <= 160 * 1024))) {
            if (greedy) PC_FULL(p.launch = all_nv28 ? roll_big<6, 5, 2, 3, false, 2, true> : roll_big<6, 5, 2, 5, false, 2, true>);
            else if (lit) { if (all_nv28) PC_DEV(8, p.launch = roll_big<6, 5, 2, 3, true, 2>); else PC_FULL(p.launch = roll_big<6, 5, 2, 5, true, 2>); }
            else { if (all_nv28) PC_DEV(7, p.launch = roll_big<6, 5, 2, 3, false, 2>); else PC_FULL(p.launch = roll_big<6, 5, 2, 5, false, 2>); }
            p.blocks = (int)((e->N + 127) / 128);
            p.lds = lds_m;
            p.rden_lds = rden_m;
            p.epw = 128;
            p.lg = 2;
            p.kernel = lit ? PC_KERNEL_K9M_LITERAL : PC_KERNEL_K9M;
            return PC_OK;
        }
    }
    if (lit) {
        // ---- the SELECTOR form: K9 itself (rollout_kernel<..., LIT>) -- the float32 sweep picks each ray's wall, the reference's literal
        // float64 arithmetic measures it (env_step_fast's literal form, lit_fast / lit_careful).  What it needs: every track inside the
        // selector's limits with its rotation table built, every env's rotation a row of that table for the rest of its episode
        // (f64_offgrid), the fast modes' shape (12, 16 or 32 nominal rays, fp16 x 2 policy arithmetic, PC_OPT_ROLLOUT_FAST not 0) and LDS
        // for the tables and (12 / 16 rays) the 1/den table.  The sweep is chosen as for F32 handles: chain-packed for two equal loops of 13
        // vertices (big_track.json) or, mixed, of 13 or 9; the generic sweeps for any other track.  Up to PC_SPLIT_MAX_ENVS envs at 12 / 16
        // rays the SMALL form (K9s: 16 envs per workgroup up to 4096 envs, wave-owned envs -- env_step_wave's literal form --, else 32 with
        // the sweep parts on four waves), chosen as for F32 handles (PC_OPT_ROLLOUT_FORM / _EPW).  Anything else: the filter form below.
        const bool small = o.form == 1 || (o.form < 0 && e->N <= PC_SPLIT_MAX_ENVS);
        const bool epw16 = o.epw_override == 16 || (o.epw_override != 32 && e->N <= 4096);
        const int rden_small = 361 * f.max_nV;
        size_t lds_small = (size_t)(img + 8 * 32 * 17 + 32 * 40 + 32 + 128 + ft_floats(true, true)) * sizeof(float);
        const int rden_small_lds = (o.rden != 0 && lds_small + (size_t)rden_small * sizeof(float) <= 160 * 1024) ? rden_small : 0;
        lds_small += (size_t)rden_small_lds * sizeof(float);
        if (f.tabs && !e->f64_offgrid && !interleaved && (rays16 || rays12) && prec == 2 && small && f.max_G <= TAB_MAX_GATES &&
            f.max_nV <= FT_VTX_MAX && o.fast && lds_small <= 160 * 1024) {
            if (rays16 && epw16) PC_DEV(6, p.launch = (roll_small<6, 5, 2, 1, 16, true>));    // wave-owned envs (env_step_wave)
            else if (rays16) PC_FULL(p.launch = (roll_small<6, 5, 2, 1, 32, true>));         // four sweep parts = waves (env_step_fast<..., 2, 4>)
            else PC_FULL(p.launch = epw16 ? roll_small<5, 3, 2, 1, 16, true> : roll_small<5, 3, 2, 1, 32, true>);     // 12 rays: three ray slots per lane
            p.blocks = (int)(epw16 ? (e->N + 15) / 16 : (e->N + 31) / 32);
            p.lds = lds_small;
            p.rden_lds = rden_small_lds;
            p.lg = 2;
            p.kernel = PC_KERNEL_K9S_LITERAL;
            return PC_OK;
        }
        const bool shape = (rays16 || rays12 || rays32) && prec == 2 && e->D >= 17 && e->D <= 40 && f.max_G <= TAB_MAX_GATES &&
                           f.max_nV <= FT_VTX_MAX && o.fast && o.rden != 0 && (!e->track_id || e->track_block >= epw) && lds_sel <= 160 * 1024;
        if (f.tabs && shape && !e->f64_offgrid && !interleaved) {
            if (rays16 && all_nv28) PC_DEV(3, p.launch = (roll_big<6, 9, 2, 3, true>));        // big_track.json's layout
            else if (rays16 && all_loops) PC_FULL(p.launch = (roll_big<6, 9, 2, 5, true>));    // ... mixed with track.json's
            else if (rays16) PC_FULL(p.launch = rden_sel ? roll_big<6, 9, 2, 2, true> : roll_big<6, 9, 2, 1, true>);    // any other track: the generic sweeps
            else if (rays32) PC_DEV(5, p.launch = (roll_big<10, 17, 2, 1, true>));             // 32 -> 33 rays: no room for the 1/den table
            else PC_FULL(p.launch = rden_sel ? roll_big<5, 6, 2, 2, true> : roll_big<5, 6, 2, 1, true>);                // 12 rays
            p.lds = lds_sel;
            p.rden_lds = rden_sel;
            p.kernel = PC_KERNEL_K9_LITERAL;
            return PC_OK;
        }
        // K9d: the generic kernel.  With PC_OPT_ROLLOUT_FAST = 0 every (ray, wall) pair is tested in float64 (the FILTER form: no float32
        // anywhere); otherwise tracks inside the selector's limits step as the per-step kernel does (sweep over the chain in global
        // memory, literal cast: rollout_f64_kernel<..., SEL>) -- what is left for this kernel by default are tracks too long for the
        // LDS tables and rotations off the table; bf16 x 3 keeps the filter.
        p.lds = (size_t)(img + 256 * (4 * KS + 1)) * sizeof(float);
        if (p.lds > 160 * 1024) return PC_ERR_UNSUPPORTED;
        const int rpl = (e->R + 1) / 2;
        const bool sel = o.fast && f.sel && prec == 2;      // (the selector variant for the fp16 x 2 forms only: bf16 x 3 -- 12 rays -- keeps the filter)
        if (KS == 5 && rpl == 6) {                         // 12 rays, D = 18
            PC_FULL(p.launch = sel ? roll_f64<5, 6, 2, true> : prec == 2 ? roll_f64<5, 6, 2, false> : roll_f64<5, 6, 1, false>);
        } else if (KS == 6 && rpl == 9) {                  // 16 -> 17 rays, D = 23 (bf16 x 3 there spills 3 registers: not built)
            if (prec != 2) return PC_ERR_UNSUPPORTED;
            if (sel) PC_FULL(p.launch = (roll_f64<6, 9, 2, true>)); else PC_DEV(4, p.launch = (roll_f64<6, 9, 2, false>));
        } else return PC_ERR_UNSUPPORTED;     // (32 -> 33 rays: 17 float64 ray slots per lane beside the policy state spill 96 registers -- not built;
                                              //  the per-step kernels run that shape)
        p.kernel = sel ? PC_KERNEL_K9D_SELECTOR : PC_KERNEL_K9D_FILTER;
        return PC_OK;
    }
    // ---- F32 handles.  Large batches: the BIG form, 128 / 256 envs per workgroup, every wave independent; small batches: the SMALL form, 16 or
    // 32 envs per workgroup, hidden tiles and wall-sweep parts split over the waves
    const bool small = !interleaved && (o.form == 1 || (o.form < 0 && e->N <= PC_SPLIT_MAX_ENVS));
    // fast mode: Discrete(9), every gather table in LDS behind LDS pointers, dense observation rows (big form: each wave's output
    // tile aliases its own 32 observation rows -- dead between the policy pass's operand load and the env step's store of the
    // next observation: needs D >= 17).  A workgroup stages ONE track's tables: single-track batches, or mixed ones in which
    // every workgroup's block of envs lies on one track.
    // The fast kernels carry their observation width as a compile-time constant derived from the ray slots per lane (12 / 17 /
    // 33 rays) and cast exactly four collision rays at the reward gate: num_rays 12 / 16 / 32 (what BASELINE's configs name).  Any
    // other count that maps onto the same slots (17 or 18 nominal rays -> 18 actual: the slots of 17; 31 -> 33 with five
    // collision rays) takes the generic mode, which reads all of that from the handle.
    const bool fast_shape = A == 9 && (rays12 || rays16 || rays32) && e->D >= 17 && e->D <= 40 && f.max_G <= TAB_MAX_GATES && o.fast;
    // (the float64 refinement gathers the chain from LDS: at most FT_VTX_MAX vertices; a shape whose fast-mode tables do not fit
    // beside the weight image -- the fp32 image at 33 rays -- takes the generic mode)
    const size_t lds_fast_big = (size_t)k9_fast_lds_floats(img, 32, e->D, KS != 10, 0) * sizeof(float);   // (33 rays: one turn of the float64 lattice)
    const bool fast = !small && fast_shape && f.max_nV <= FT_VTX_MAX && (!e->track_id || e->track_block >= epw) && lds_fast_big <= 160 * 1024;
    const size_t lds_big = fast ? lds_fast_big : (size_t)(img + 256 * (4 * KS + 1) + 256 + TAB_FLOATS) * sizeof(float);
    const size_t lds_fast_small = (size_t)(img + 8 * 32 * 17 + 32 * 40 + 32 + 128 + ft_floats(true, true)) * sizeof(float);
    const bool fast_small = small && fast_shape && f.max_nV <= FT_VTX_MAX && lds_fast_small <= 160 * 1024;     // (a small-form workgroup is 16 or 32 envs)
    const size_t lds_small = fast_small ? lds_fast_small : (size_t)(img + 8 * 32 * 17 + 32 * (4 * KS + 1) + 32 + 128 + TAB_FLOATS) * sizeof(float);
    p.lds = small ? lds_small : lds_big;
    if (p.lds > 160 * 1024) return PC_ERR_UNSUPPORTED;
    // the track's 1/den table rides along in LDS when it fits (big_track: 361 x 28 floats = 40 KB); else the sweep forms
    // den and its reciprocal itself -- same bits either way.  Mixed batches: in the fast modes only (room for the largest track).
    // (the big form at 33 rays has 4 KB left: no closed track's table fits, so that shape is built without the table mode)
    p.rden_lds = 361 * f.max_nV;
    if (!f.rden || o.rden == 0 || (e->track_id && !(small ? fast_small : fast)) || p.lds + (size_t)p.rden_lds * sizeof(float) > 160 * 1024 ||
        (!small && KS == 10))
        p.rden_lds = 0;
    p.lds += (size_t)p.rden_lds * sizeof(float);
    const int mode = (fast || fast_small) ? (p.rden_lds ? 2 : 1) : 0;
    if (greedy && !mode) return PC_ERR_UNSUPPORTED;           // (the generic mode)
    if (!small) {
        const int rpl = (e->R + 1) / 2;       // 2 lanes per env
        if (greedy) {                        // the instance the rules below pick, in its greedy form
            const bool r16 = KS == 6 && rpl == 9;
            const int md = (r16 && mode == 2 && all_nv28) ? 3 : (r16 && mode == 2 && all_loops) ? 5 : (r16 && mode == 1 && all_nv28) ? 4 : mode;
            const int rc = greedy_big(KS, rpl, md, p.launch);
            if (rc != PC_OK) return rc;
        } else if (KS == 5 && rpl == 6) {    // 12 rays, D = 18
            PC_FULL(p.launch = prec == 2 ? roll_big_mode<5, 6, 2>(mode) : prec ? roll_big_mode<5, 6, 1>(mode) : roll_big_mode<5, 6, 0>(mode));
        } else if (KS == 6 && rpl == 9) {    // 16 -> 17 rays, D = 23; fp16 x 2: the chain-of-28 and chain-packed kernels
            if (prec == 2 && mode == 2 && all_nv28) PC_DEV(0, p.launch = (roll_big<6, 9, 2, 3>));
            else if (prec == 2 && mode == 2 && all_loops) PC_FULL(p.launch = (roll_big<6, 9, 2, 5>));
            else if (prec == 2 && mode == 1 && all_nv28) PC_FULL(p.launch = (roll_big<6, 9, 2, 4>));
            else PC_FULL(p.launch = prec == 2 ? roll_big_mode<6, 9, 2>(mode) : prec ? roll_big_mode<6, 9, 1>(mode) : roll_big_mode<6, 9, 0>(mode));
        } else if (KS == 10 && rpl == 17 && prec) {     // 32 -> 33 rays, D = 39
            // (the chain-of-28 variant spills: not built.  The GENERIC mode at 33 rays -- a mixed-track batch whose workgroups straddle
            // tracks, fast mode switched off -- spilled 100+ registers beside the split operands' policy state: not built either; that
            // shape is PC_ERR_UNSUPPORTED here and runs through the per-step kernels, bit-identical by construction)
            if (!mode) return PC_ERR_UNSUPPORTED;
            if (prec == 2) PC_DEV(2, p.launch = (roll_big<10, 17, 2, 1>)); else PC_FULL(p.launch = (roll_big<10, 17, 1, 1>));
        } else return PC_ERR_UNSUPPORTED;
        p.kernel = PC_KERNEL_K9;
        return PC_OK;
    }
    // small form: 16 envs per workgroup up to 4096 envs (<= 256 workgroups: one per CU), else 32
    const int epw_small = (o.epw_override == 16 || o.epw_override == 32) ? o.epw_override
                          : ((fast_small && prec != 0 && e->R <= 17 && e->N <= 4096) ? 16 : 32);
    if (epw_small == 16 && !(fast_small && prec != 0 && e->R <= 17)) return PC_ERR_UNSUPPORTED;
    const bool epw16 = mode && epw_small == 16;
    const int rpl = (e->R + 3) / 4;           // 4 lanes per env (x 4 sweep parts)
    if (greedy) {                            // the instance the rules below pick, in its greedy form
        const int rc = greedy_small(KS, rpl, epw16, p.rden_lds != 0, p.launch);
        if (rc != PC_OK) return rc;
    } else if (KS == 5 && rpl == 3) {        // 12 rays
        PC_FULL(p.launch = prec == 2 ? roll_small_mode<5, 3, 2>(mode, epw16) : prec ? roll_small_mode<5, 3, 1>(mode, epw16) : roll_small_mode<5, 3, 0>(mode, epw16));
    } else if (KS == 6 && rpl == 5) {        // 16 -> 17 rays (configs[1]'s kernel: with the 1/den table in LDS the env step is compiled for it)
        if (prec == 2 && epw16 && p.rden_lds) PC_DEV(1, p.launch = (roll_small<6, 5, 2, 2, 16>));
        else PC_FULL(p.launch = prec == 2 ? roll_small_mode<6, 5, 2>(mode, epw16) : prec ? roll_small_mode<6, 5, 1>(mode, epw16) : roll_small_mode<6, 5, 0>(mode, epw16));
    } else if (KS == 10 && rpl == 9) {       // 32 -> 33 rays
        if (prec == 1 && !mode) return PC_ERR_UNSUPPORTED;    // (bf16 x 3 in the generic mode spilled: the caller's per-step kernels take that shape)
        PC_FULL(p.launch = prec == 2 ? roll_small_mode<10, 9, 2>(mode, false) : prec ? roll_small<10, 9, 1, 1, 32> : roll_small_mode<10, 9, 0>(mode, false));
    } else return PC_ERR_UNSUPPORTED;
    p.blocks = (int)((e->N + epw_small - 1) / epw_small);
    p.lg = 2;
    p.kernel = PC_KERNEL_K9S;
    return PC_OK;
}

static int rollout_run(pc_env* e, const pc_policy* p, const float* image, int64_t T, double reward_scale, uint64_t seed, uint64_t offset,
                       const uint64_t* offset_dev, float* obs_buf, float* act_buf, float* rew_buf, float* val_buf, float* term_buf,
                       float* trunc_buf, float* logprob_buf, float* next_obs, float* next_term, float* next_trunc, float* last_value,
                       float* reward_sum, float* final_obs, hipStream_t stream, bool greedy = false);

int pc_rollout(pc_env* e, const pc_policy* p, const float* image, int64_t T, double reward_scale, uint64_t seed, uint64_t offset,
               const uint64_t* offset_dev, float* obs_buf, float* act_buf, float* rew_buf, float* val_buf, float* term_buf,
               float* trunc_buf, float* logprob_buf, float* next_obs, float* next_term, float* next_trunc, float* last_value,
               float* reward_sum, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    return rollout_run(e, p, image, T, reward_scale, seed, offset, offset_dev, obs_buf, act_buf, rew_buf, val_buf, term_buf, trunc_buf, logprob_buf,
                       next_obs, next_term, next_trunc, last_value, reward_sum, nullptr, (hipStream_t)stream);
}

int pc_rollout_final_obs(pc_env* e, const pc_policy* p, const float* image, int64_t T, double reward_scale, uint64_t seed,
                         uint64_t offset, const uint64_t* offset_dev, float* obs_buf, float* act_buf, float* rew_buf, float* val_buf,
                         float* term_buf, float* trunc_buf, float* logprob_buf, float* next_obs, float* next_term, float* next_trunc,
                         float* last_value, float* reward_sum, float* final_obs, int64_t slots, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!final_obs || T < 1 || slots < (T + PC_TIME_LIMIT - 1) / PC_TIME_LIMIT) return PC_ERR_INVALID_ARG;
    return rollout_run(e, p, image, T, reward_scale, seed, offset, offset_dev, obs_buf, act_buf, rew_buf, val_buf, term_buf, trunc_buf, logprob_buf,
                       next_obs, next_term, next_trunc, last_value, reward_sum, final_obs, (hipStream_t)stream);
}

int pc_rollout_greedy(pc_env* e, const pc_policy* p, const float* image, int64_t T, double reward_scale, float* obs_buf, float* act_buf,
                      float* rew_buf, float* val_buf, float* term_buf, float* trunc_buf, float* logprob_buf, float* next_obs, float* next_term,
                      float* next_trunc, float* last_value, float* reward_sum, float* final_obs, int64_t slots, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (final_obs && (T < 1 || slots < (T + PC_TIME_LIMIT - 1) / PC_TIME_LIMIT)) return PC_ERR_INVALID_ARG;
    return rollout_run(e, p, image, T, reward_scale, 0, 0, nullptr, obs_buf, act_buf, rew_buf, val_buf, term_buf, trunc_buf, logprob_buf, next_obs,
                       next_term, next_trunc, last_value, reward_sum, final_obs, (hipStream_t)stream, true);
}

// pc_rollout / pc_rollout_final_obs / pc_rollout_greedy: one dispatch (plan_rollout), one launch
static int rollout_run(pc_env* e, const pc_policy* p, const float* image, int64_t T, double reward_scale, uint64_t seed, uint64_t offset,
                       const uint64_t* offset_dev, float* obs_buf, float* act_buf, float* rew_buf, float* val_buf, float* term_buf,
                       float* trunc_buf, float* logprob_buf, float* next_obs, float* next_term, float* next_trunc, float* last_value,
                       float* reward_sum, float* final_obs, hipStream_t stream, bool greedy) {
    if (!e || !p) return PC_ERR_INVALID_ARG;
    if (p->D != e->D || p->device != e->device) return PC_ERR_INVALID_ARG;     // the policy was built for another observation width / device
    if (!image || !obs_buf || !act_buf || !rew_buf || !val_buf || !term_buf || !trunc_buf || !logprob_buf || !next_obs || !next_term || !next_trunc ||
        T < 1 || T > (1 << 24))
        return PC_ERR_INVALID_ARG;
    // 16-byte stores of the waves' 32-row blocks: the rows' offsets inside the buffers AND the buffers themselves are aligned
    const int vec_ok = ((e->N * e->D) % 4 == 0 && (((uintptr_t)obs_buf | (uintptr_t)next_obs) & 15) == 0) ? 1 : 0;
    RolloutPlan plan;
    int rc = plan_rollout(e, policy_prec(p->precision, e->D, p->A), p->A, vec_ok, greedy, plan);
    if (rc != PC_OK) return rc;
    DeviceGuard guard(e->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const RolloutIO io{image, p->A, (int)T, reward_scale, seed, offset, offset_dev, obs_buf, act_buf, rew_buf, val_buf, term_buf, trunc_buf, logprob_buf,
                       next_obs, next_term, next_trunc, last_value, reward_sum, final_obs};
    rc = plan.launch(e, plan, io, stream);
    if (rc != PC_OK) return rc;
    e->last_kernel = plan.kernel;
    return PC_OK;
}

// ---- the PPO minibatch step (kernels/update.hpp, update_large.hpp): one shape menu (with_mlp_shape), one workspace layout, one launch sequence
static bool mb_defer_shape(int D, int A) {      // the menu's entries with the shape compiled in
    bool compiled = false;
    with_mlp_shape(D, A, [&](auto, auto ac, auto) { compiled = decltype(ac)::value > 0; });
    return compiled;
}
static bool small_batch(int B) { return B >= 2 && B <= 1024; }      // K10: one workgroup per 8 samples, statistics by one workgroup
static bool large_shape(int B, int D, int H, int A) { return mlp_shape_ok(D, H, A) && B > 1024 && B <= PC_PPO_LARGE_MAX_B; }

// The workspace of one minibatch step -- the ONLY place that knows its layout: n_part gradient partials (K10: one per group of 8
// samples; parts > 0: K10L's fixed grid, pc_ppo_large_parts), their (pl, vl, ent, -) partials, K11's squared-norm partials and, for
// the diagnostics forms alone, a second per-workgroup partial (sum of KL terms, clipped samples).
struct MbPlan {
    int n_param, n_part, n_blk, n_pad, HD, mid_end;
    float *partial, *metric_partial, *norm_partial, *diag_partial;
    MbPlan(int B, int D, int H, int A, float* workspace, int parts = 0) {
        n_param = (int)mlp_n_param(D, H, A);
        n_part = parts > 0 ? parts : (B + FB_S - 1) / FB_S;
        n_blk = (n_param + 255) / 256;
        n_pad = (int)pad4(n_param);          // a partial's row stride
        HD = H * D;
        mid_end = HD + H + A * H + A;        // natural offset of critic.0.weight (ppo_fwdbwd_body's o_cW1)
        partial = workspace;
        metric_partial = partial + (size_t)n_part * n_pad;
        norm_partial = metric_partial + n_part * 4;
        diag_partial = norm_partial + n_blk;
    }
    int64_t floats(bool diag) const { return (int64_t)n_part * n_pad + n_part * 4 + n_blk + (diag ? 2 * n_part : 0); }
};

int64_t pc_ppo_workspace_floats(int B, int D, int H, int A) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!mlp_shape_ok(D, H, A) || !small_batch(B)) return PC_ERR_UNSUPPORTED;
    return MbPlan(B, D, H, A, nullptr).floats(false);
}

int64_t pc_ppo_diag_workspace_floats(int B, int D, int H, int A) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!mlp_shape_ok(D, H, A) || !small_batch(B)) return PC_ERR_UNSUPPORTED;
    return MbPlan(B, D, H, A, nullptr).floats(true);
}

// One minibatch step as the entry points hand it over
struct MbSamples {      // the rollout's tensors and this minibatch's indices, or (prep) a block ppo_prepare_kernel gathered
    const int64_t* idx; const float *obs, *act, *old_logprob, *adv, *ret, *prep;
    bool bc = false;        // the cross-entropy step (K27): act = the labels, ret = the critic's targets or nullptr, no old_logprob / adv
    bool soft = false;      // with bc: act = soft targets [M][A] (pc_bc_minibatch_soft)
    bool complete() const { return bc ? idx && obs && act : prep || (idx && obs && act && old_logprob && adv && ret); }
};
struct MbState { float *param, *grad, *exp_avg, *exp_avg_sq, *step_count; const float* lr_dev; };
struct MbCoef { double clip_ratio, vf_coef, ent_coef, max_norm, beta1, beta2, eps; };
struct MbStep {
    MbSamples in; MbState s; MbCoef c;
    float *metrics, *workspace;
    int apply;                  // 0: gradient only; 1: + clip + Adam; 2: + the step counter (the caller exchanges, then pc_clip_adam_advanced)
    float* diag = nullptr; double target_kl = 0.0;      // the diagnostics forms
};
// the minibatch entry points share their parameter names: their step, IN the samples, then (diag, target_kl) for the diagnostics forms
#define PC_MB_STEP(IN, ...)                                                                                                              \
    MbStep{IN, {param, grad, exp_avg, exp_avg_sq, step_count, lr_dev}, {clip_ratio, vf_coef, ent_coef, max_norm, beta1, beta2, eps}, \
           metrics, workspace, apply, ##__VA_ARGS__}
static int check_apply_args(const MbStep& m) {
    if (!m.s.param || !m.s.grad || !m.metrics || !m.workspace) return PC_ERR_INVALID_ARG;
    if (m.apply == 1 && (!m.s.exp_avg || !m.s.exp_avg_sq || !m.s.step_count || !m.s.lr_dev)) return PC_ERR_INVALID_ARG;
    if (m.apply == 2 && !m.s.step_count) return PC_ERR_INVALID_ARG;
    // K10 / K10L / K27 fetch W1 out of `param` as 16-byte vectors and store the [H][D] blocks of every partial (the head of the
    // workspace, rows of n_pad = a multiple of 4 floats) the same way: no other pointer of the step is accessed wider than 4 bytes
    if ((((uintptr_t)m.s.param | (uintptr_t)m.workspace) & 15) != 0) return PC_ERR_INVALID_ARG;
    return m.apply < 0 || m.apply > 2 ? PC_ERR_INVALID_ARG : PC_OK;
}

// K10 (its diagnostics form with `diag`, its deferred form with df.grad; K27 with in.bc) on `param`
static void launch_fwdbwd(const MbPlan& pl, int B, int D, int A, const MbSamples& in, const float* param, const MbCoef& c, const AdamDefer& df,
                          const float* diag, hipStream_t st) {
    with_mlp_shape(D, A, [&](auto dm, auto ac, auto dc) {
        constexpr int DM = decltype(dm)::value, AC = decltype(ac)::value, DC = decltype(dc)::value;
        auto go = [&](auto kernel, auto... extra) {
            hipLaunchKernelGGL(kernel, dim3(pl.n_part), dim3(256), 0, st, in.idx, B, D, A, in.obs, in.act, in.old_logprob, in.adv, in.ret, param,
                               (float)c.clip_ratio, (float)c.vf_coef, (float)c.ent_coef, pl.partial, pl.metric_partial, in.prep, extra...);
        };
        if (in.bc && in.soft) {
            hipLaunchKernelGGL((bc_soft_fwdbwd_kernel<DM, AC, DC>), dim3(pl.n_part), dim3(256), 0, st, in.idx, B, D, A, in.obs, in.act, in.ret, param,
                               (float)c.vf_coef, (float)c.ent_coef, pl.partial, pl.metric_partial);
            return;
        }
        if (in.bc) {
            hipLaunchKernelGGL((bc_fwdbwd_kernel<DM, AC, DC>), dim3(pl.n_part), dim3(256), 0, st, in.idx, B, D, A, in.obs, in.act, in.ret, param,
                               (float)c.vf_coef, (float)c.ent_coef, pl.partial, pl.metric_partial);
            return;
        }
        if (diag) return go(ppo_fwdbwd_diag_kernel<DM, AC, DC>, diag, pl.diag_partial);
        if constexpr (AC > 0) if (df.grad) return go(ppo_fwdbwd_kernel<DM, AC, DC, true>, df);
        go(ppo_fwdbwd_kernel<DM, AC, DC, false>, df);
    });
}
// K11 (its diagnostics form with `diag`)
static void launch_reduce(const MbPlan& pl, int B, const MbCoef& c, float* grad, float* metrics, float* step_count, hipStream_t st,
                          float* diag = nullptr, double target_kl = 0.0) {
    auto go = [&](auto kernel, auto... extra) {
        hipLaunchKernelGGL(kernel, dim3(pl.n_blk), dim3(256), 0, st, pl.partial, pl.n_part, pl.n_param, pl.HD, pl.mid_end, pl.n_pad, grad,
                           pl.norm_partial, pl.metric_partial, B, (float)c.vf_coef, (float)c.ent_coef, metrics, step_count, extra...);
    };
    if (diag) go(grad_reduce_diag_kernel, diag, (const float*)pl.diag_partial, kl_stop_of(target_kl));
    else go(grad_reduce_kernel);
}
// K12 (its diagnostics form with `diag`): state `in` -> state `out`
static void launch_adam(const MbPlan& pl, const float* p_in, const float* m_in, const float* v_in, const MbState& out, const MbCoef& c, hipStream_t st,
                        const float* diag = nullptr) {
    auto go = [&](auto kernel, auto... extra) {
        hipLaunchKernelGGL(kernel, dim3(pl.n_blk), dim3(256), 0, st, p_in, m_in, v_in, out.grad, out.param, out.exp_avg, out.exp_avg_sq,
                           (const float*)out.step_count, out.lr_dev, (const float*)pl.norm_partial, pl.n_blk, pl.n_param, (float)c.max_norm,
                           (float)c.beta1, (float)c.beta2, (float)c.eps, extra...);
    };
    if (diag) go(adam_diag_kernel, diag);
    else go(adam_kernel);
}
// what follows K10 / K10L in every step: the reduction, and with apply == 1 clip + Adam in place
static void launch_reduce_apply(const MbPlan& pl, int B, const MbStep& m, hipStream_t st) {
    launch_reduce(pl, B, m.c, m.s.grad, m.metrics, m.apply ? m.s.step_count : nullptr, st, m.diag, m.target_kl);
    if (m.apply == 1) launch_adam(pl, m.s.param, m.s.exp_avg, m.s.exp_avg_sq, m.s, m.c, st, m.diag);
}

static int ppo_minibatch_impl(int device, int B, int D, int H, int A, const MbStep& m, void* stream) {
    if (const int rc = check_apply_args(m); rc != PC_OK || !m.in.complete()) return PC_ERR_INVALID_ARG;
    if (!mlp_shape_ok(D, H, A) || !small_batch(B)) return PC_ERR_UNSUPPORTED;
    if (m.diag && m.apply == 2) return PC_ERR_UNSUPPORTED;      // (the ranks of a multi-rank step would have to agree on the stop)
    if ((m.diag || m.in.bc) && device < 0) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const MbPlan pl(B, D, H, A, m.workspace);
    hipStream_t st = (hipStream_t)stream;
    launch_fwdbwd(pl, B, D, A, m.in, m.s.param, m.c, AdamDefer{}, m.diag, st);
    launch_reduce_apply(pl, B, m, st);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_ppo_minibatch(int device, const int64_t* idx, int B, int D, int H, int A, const float* obs, const float* act,
                     const float* old_logprob, const float* adv, const float* ret, float* param, float* grad, float* exp_avg,
                     float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef, double ent_coef,
                     double max_norm, double beta1, double beta2, double eps, float* metrics, float* workspace, int apply,
                     void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    return ppo_minibatch_impl(device, B, D, H, A, PC_MB_STEP((MbSamples{idx, obs, act, old_logprob, adv, ret, nullptr})), stream);
}

int pc_ppo_minibatch_diag(int device, const int64_t* idx, int B, int D, int H, int A, const float* obs, const float* act,
                          const float* old_logprob, const float* adv, const float* ret, float* param, float* grad, float* exp_avg,
                          float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef, double ent_coef,
                          double max_norm, double beta1, double beta2, double eps, float* metrics, float* workspace, int apply,
                          float* diag, double target_kl, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!diag) return PC_ERR_INVALID_ARG;
    return ppo_minibatch_impl(device, B, D, H, A, PC_MB_STEP((MbSamples{idx, obs, act, old_logprob, adv, ret, nullptr}), diag, target_kl), stream);
}

// K27 + K11 + K12: one supervised minibatch step (cross-entropy against labels, optionally the critic's regression)
int pc_bc_minibatch(int device, const int64_t* idx, int B, int D, int H, int A, const float* obs, const float* label, const float* target,
                    float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* step_count, const float* lr_dev, double vf_coef,
                    double ent_coef, double max_norm, double beta1, double beta2, double eps, float* metrics, float* workspace, int apply,
                    void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!target && vf_coef != 0.0) return PC_ERR_INVALID_ARG;      // (NaN too: a value term needs its targets)
    const double clip_ratio = 0.0;                                 // (the cross-entropy head has no clip)
    return ppo_minibatch_impl(device, B, D, H, A, PC_MB_STEP((MbSamples{idx, obs, label, nullptr, nullptr, target, nullptr, true})), stream);
}

// the same step against soft targets [M][A] (the LOSS_BC_SOFT head)
int pc_bc_minibatch_soft(int device, const int64_t* idx, int B, int D, int H, int A, const float* obs, const float* soft, const float* target,
                         float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* step_count, const float* lr_dev, double vf_coef,
                         double ent_coef, double max_norm, double beta1, double beta2, double eps, float* metrics, float* workspace, int apply,
                         void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!target && vf_coef != 0.0) return PC_ERR_INVALID_ARG;      // (NaN too: a value term needs its targets)
    const double clip_ratio = 0.0;                                 // (the cross-entropy head has no clip)
    return ppo_minibatch_impl(device, B, D, H, A, PC_MB_STEP((MbSamples{idx, obs, soft, nullptr, nullptr, target, nullptr, true, true})), stream);
}

int64_t pc_ppo_prepared_floats(int B, int D) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (D < 1 || D > 40 || !small_batch(B)) return PC_ERR_UNSUPPORTED;
    return (int64_t)B * (D + 4) + 4;
}

int pc_ppo_prepare(int device, const int64_t* idx, int64_t idx_ld, int n_mb, int B, int D, const float* obs, const float* act,
                   const float* old_logprob, const float* adv, const float* ret, float* prepared, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!idx || !obs || !act || !old_logprob || !adv || !ret || !prepared || n_mb < 1 || idx_ld < B) return PC_ERR_INVALID_ARG;
    if (D < 1 || D > 40 || !small_batch(B)) return PC_ERR_UNSUPPORTED;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    hipLaunchKernelGGL(ppo_prepare_kernel, dim3(n_mb), dim3(256), 0, (hipStream_t)stream, idx, idx_ld, B, D, obs, act, old_logprob, adv, ret,
                       prepared, (int64_t)B * (D + 4) + 4);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_ppo_minibatch_prepared(int device, const float* prepared_mb, int B, int D, int H, int A, float* param, float* grad, float* exp_avg,
                              float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef,
                              double ent_coef, double max_norm, double beta1, double beta2, double eps, float* metrics,
                              float* workspace, int apply, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!prepared_mb) return PC_ERR_INVALID_ARG;
    return ppo_minibatch_impl(device, B, D, H, A, PC_MB_STEP((MbSamples{.prep = prepared_mb})), stream);
}

int pc_ppo_minibatch_prepared_diag(int device, const float* prepared_mb, int B, int D, int H, int A, float* param, float* grad, float* exp_avg,
                                   float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef,
                                   double ent_coef, double max_norm, double beta1, double beta2, double eps, float* metrics,
                                   float* workspace, int apply, float* diag, double target_kl, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!prepared_mb || !diag) return PC_ERR_INVALID_ARG;
    return ppo_minibatch_impl(device, B, D, H, A, PC_MB_STEP((MbSamples{.prep = prepared_mb}), diag, target_kl), stream);
}

// ---- the large-minibatch step (kernels/update_large.hpp): 1024 < B <= PC_PPO_LARGE_MAX_B.  K10L's grid = its number of partials: one
// workgroup per group of 8 samples up to one per compute unit.  The ONE expression the workspace size, the launch and pc_ppo_large_parts share.
static int large_parts(int device, int B, int* out) {
    if (device < 0) return PC_ERR_NO_DEVICE;
    int cus = 0;
    if (device_cus(device, &cus) != PC_OK) return PC_ERR_NO_DEVICE;
    *out = std::min((B + FB_S - 1) / FB_S, cus);
    return PC_OK;
}

int pc_ppo_large_parts(int device, int B) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (B <= 1024 || B > PC_PPO_LARGE_MAX_B) return PC_ERR_UNSUPPORTED;
    int parts = 0;
    const int rc = large_parts(device, B, &parts);
    return rc != PC_OK ? rc : parts;
}

int64_t pc_ppo_large_workspace_floats(int device, int B, int D, int H, int A) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!large_shape(B, D, H, A)) return PC_ERR_UNSUPPORTED;
    int parts = 0;
    const int rc = large_parts(device, B, &parts);
    return rc != PC_OK ? rc : MbPlan(B, D, H, A, nullptr, parts).floats(false);
}

int64_t pc_ppo_adv_stats_workspace_doubles(int n_mb, int B) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (n_mb < 1) return PC_ERR_INVALID_ARG;
    if (B <= 1024 || B > PC_PPO_LARGE_MAX_B) return PC_ERR_UNSUPPORTED;
    return (int64_t)n_mb * adv_stats_parts(B) * 2;
}

int pc_ppo_adv_stats(int device, const int64_t* idx, int64_t idx_ld, int n_mb, int B, const float* adv, float* stats, double* workspace,
                     void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!idx || !adv || !stats || !workspace || n_mb < 1 || n_mb > 65535 || idx_ld < B) return PC_ERR_INVALID_ARG;
    if (B <= 1024 || B > PC_PPO_LARGE_MAX_B) return PC_ERR_UNSUPPORTED;
    if (device < 0) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const int P = adv_stats_parts(B);
    hipLaunchKernelGGL(ppo_adv_stats_large_kernel, dim3(P, n_mb), dim3(AS_THREADS), 0, (hipStream_t)stream, idx, idx_ld, B, adv, workspace);
    hipLaunchKernelGGL(ppo_adv_stats_merge_kernel, dim3(n_mb), dim3(64), 0, (hipStream_t)stream, idx, idx_ld, B, P, adv, workspace, stats);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_ppo_minibatch_large(int device, const int64_t* idx, int B, int D, int H, int A, const float* obs, const float* act,
                           const float* old_logprob, const float* adv, const float* ret, const float* adv_stats, float* param, float* grad,
                           float* exp_avg, float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef,
                           double ent_coef, double max_norm, double beta1, double beta2, double eps, float* metrics, float* workspace,
                           int apply, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    const MbStep m = PC_MB_STEP((MbSamples{idx, obs, act, old_logprob, adv, ret, nullptr}));
    if (check_apply_args(m) != PC_OK || !m.in.complete() || !adv_stats) return PC_ERR_INVALID_ARG;
    if (!large_shape(B, D, H, A)) return PC_ERR_UNSUPPORTED;
    int parts = 0;
    if (const int rc = large_parts(device, B, &parts); rc != PC_OK) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const MbPlan pl(B, D, H, A, workspace, parts);
    hipStream_t st = (hipStream_t)stream;
    with_mlp_shape(D, A, [&](auto dm, auto ac, auto dc) {
        hipLaunchKernelGGL((ppo_fwdbwd_large_kernel<decltype(dm)::value, decltype(ac)::value, decltype(dc)::value>), dim3(pl.n_part), dim3(256), 0, st,
                           idx, B, D, A, obs, act, old_logprob, adv, ret, adv_stats, (const float*)param, (float)clip_ratio, (float)vf_coef,
                           (float)ent_coef, pl.partial, pl.metric_partial);
    });
    launch_reduce_apply(pl, B, m, st);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

#undef PC_MB_STEP

int64_t pc_ppo_epoch_state_floats(int D, int H, int A) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!mlp_shape_ok(D, H, A)) return PC_ERR_UNSUPPORTED;
    return 3 * pad4(mlp_n_param(D, H, A));
}

int pc_ppo_epoch_prepared(int device, const float* prepared, int n_mb, int B, int D, int H, int A, float* param, float* grad, float* exp_avg,
                          float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef, double ent_coef,
                          double max_norm, double beta1, double beta2, double eps, float* metrics, float* workspace, float* state2,
                          void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!prepared || !param || !grad || !exp_avg || !exp_avg_sq || !step_count || !lr_dev || !metrics || !workspace || !state2 || n_mb < 1)
        return PC_ERR_INVALID_ARG;
    if (!mlp_shape_ok(D, H, A) || !small_batch(B)) return PC_ERR_UNSUPPORTED;
    if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)state2) & 15) != 0) return PC_ERR_INVALID_ARG;   // 16-byte loads / stores
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    const MbPlan pl(B, D, H, A, workspace);
    hipStream_t st = (hipStream_t)stream;
    const MbState home{param, grad, exp_avg, exp_avg_sq, step_count, lr_dev};
    const MbCoef c{clip_ratio, vf_coef, ent_coef, max_norm, beta1, beta2, eps};
    // two generations of (param, exp_avg, exp_avg_sq): the caller's tensors and `state2`
    float* P[2] = {param, state2};
    float* M[2] = {exp_avg, state2 + pl.n_pad};
    float* V[2] = {exp_avg_sq, state2 + 2 * (size_t)pl.n_pad};
    const int64_t pf = (int64_t)B * (D + 4) + 4;
    int cur = 0;
    const bool defer = mb_defer_shape(D, A);     // (other shapes: the generic kernels, three launches per minibatch -- the same bits)
    for (int m = 0; m < n_mb; ++m) {
        AdamDefer df{};
        if (!defer && m > 0) launch_adam(pl, param, exp_avg, exp_avg_sq, home, c, st);
        if (defer && m > 0)      // the previous minibatch's gradient is applied by this launch as it loads the parameters
            df = AdamDefer{grad, M[cur], V[cur], P[cur ^ 1], M[cur ^ 1], V[cur ^ 1], pl.norm_partial, pl.n_blk, step_count, lr_dev,
                           (float)max_norm, (float)beta1, (float)beta2, (float)eps};
        launch_fwdbwd(pl, B, D, A, {.prep = prepared + (size_t)m * pf}, P[cur], c, df, nullptr, st);
        if (defer && m > 0) cur ^= 1;
        launch_reduce(pl, B, c, grad, metrics, step_count, st);
    }
    // the last gradient, and the state home to the caller's tensors
    launch_adam(pl, P[cur], M[cur], V[cur], home, c, st);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

// ---- pc_xchg: one-shot all-reduce over peer-mapped staging buffers (kernels/exchange.hpp) --------------------------------
}  // extern "C"

struct pc_xchg {
    int device = 0, rank = 0, world = 1;
    int64_t n = 0;
    int n_pad = 0, n_chunks = 0;
    char* local = nullptr;                       // this rank's staging allocation (uncached device memory)
    char* peer[XCHG_MAX_RANKS] = {nullptr};      // every rank's allocation as mapped here (peer[rank] == local)
    bool ipc[XCHG_MAX_RANKS] = {false};          // peer[r] came from hipIpcOpenMemHandle (closed at destroy); false: a pointer of this process
    bool connected = false;
    double timeout_s = 20.0;
    size_t data_bytes() const { return (size_t)2 * world * n_pad * sizeof(float); }
    size_t flag_bytes() const { return (size_t)2 * world * n_chunks * sizeof(unsigned); }
    size_t total_bytes() const { return data_bytes() + flag_bytes() + (size_t)n_chunks * sizeof(unsigned) + 64; }
    XchgView view() const {
        XchgView v;
        for (int r = 0; r < XCHG_MAX_RANKS; ++r) {
            char* b = r < world ? peer[r] : nullptr;
            v.data[r] = reinterpret_cast<float*>(b);
            v.flags[r] = reinterpret_cast<unsigned*>(b ? b + data_bytes() : nullptr);
        }
        v.epoch = reinterpret_cast<unsigned*>(local + data_bytes() + flag_bytes());
        v.error = reinterpret_cast<int*>(local + data_bytes() + flag_bytes() + (size_t)n_chunks * sizeof(unsigned));
        v.rank = rank;
        v.world = world;
        v.n = (int)n;
        v.n_pad = n_pad;
        v.n_chunks = n_chunks;
        v.timeout_ticks = (unsigned long long)(timeout_s * XCHG_TICKS_PER_SECOND);
        return v;
    }
};

extern "C" {

int pc_xchg_create(int device, int rank, int world, int64_t n_floats, pc_xchg** out) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!out || world < 1 || world > XCHG_MAX_RANKS || rank < 0 || rank >= world || n_floats < 1 || n_floats > (1 << 24)) return PC_ERR_INVALID_ARG;
    if (!valid_device(device)) return PC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    pc_xchg* x = new (std::nothrow) pc_xchg;
    if (!x) return PC_ERR_INVALID_ARG;
    x->device = device;
    x->rank = rank;
    x->world = world;
    x->n = n_floats;
    x->n_chunks = (int)((n_floats + XCHG_CHUNK - 1) / XCHG_CHUNK);
    x->n_pad = x->n_chunks * XCHG_CHUNK;
    void* p = nullptr;
    // uncached, fine-grained device memory: a peer's stores must be visible to a kernel that is already running here
    hipError_t e = hipExtMallocWithFlags(&p, x->total_bytes(), hipDeviceMallocUncached);
    if (e != hipSuccess) e = hipExtMallocWithFlags(&p, x->total_bytes(), hipDeviceMallocFinegrained);
    if (e != hipSuccess) {
        g_hip_err = std::string("hipExtMallocWithFlags: ") + hipGetErrorString(e);
        delete x;
        return PC_ERR_HIP;
    }
    x->local = static_cast<char*>(p);
    x->peer[rank] = x->local;
    if (hipMemset(p, 0, x->total_bytes()) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(p);
        delete x;
        return PC_ERR_HIP;
    }
    x->connected = world == 1;
    *out = x;
    return PC_OK;
}

// The handle a rank publishes = the hipIpcMemHandle_t of its staging buffer (64 bytes) followed by the PCI bus id of the device the
// buffer lives on (NUL-terminated text, hipDeviceGetPCIBusId): a peer resolves THAT to its own ordinal of the device -- the
// pointer a peer gets from hipIpcOpenMemHandle says nothing reliable about the owning device (hipPointerGetAttributes on an IPC
// mapping reports the opener's device or fails).
int pc_xchg_local_handle(pc_xchg* x, void* handle_out) {
    if (!x || !handle_out) return PC_ERR_INVALID_ARG;
    static_assert(sizeof(hipIpcMemHandle_t) == 64 && PC_XCHG_HANDLE_BYTES == 128, "handle layout");
    g_hip_err.clear();
    DeviceGuard guard(x->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    hipIpcMemHandle_t h;
    HIPCHK(hipIpcGetMemHandle(&h, x->local));
    char* out = static_cast<char*>(handle_out);
    memset(out, 0, PC_XCHG_HANDLE_BYTES);
    memcpy(out, &h, sizeof(h));
    HIPCHK(hipDeviceGetPCIBusId(out + sizeof(h), PC_XCHG_HANDLE_BYTES - (int)sizeof(h) - 1, x->device));
    return PC_OK;
}

int pc_xchg_connect(pc_xchg* x, const void* all_handles) {
    if (!x || !all_handles) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(x->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    g_hip_err.clear();
    const char* all = static_cast<const char*>(all_handles);
    // a failed connect leaves the handle as it was: the mappings opened by THIS call are closed again, and no HIP error stays
    // behind for an unrelated later call to report
    std::vector<int> opened;
    auto fail = [&](int code, const std::string& why) {
        for (int r : opened) { (void)hipIpcCloseMemHandle(x->peer[r]); x->peer[r] = nullptr; }
        (void)hipGetLastError();
        g_hip_err = why;
        return code;
    };
    // 1. every peer's DEVICE must be reachable from ours before a kernel of ours writes into its memory: resolve the published
    //    PCI bus id to this process's ordinal and verify / enable peer access -- a distinct error NOW, not a 20-second wait for a
    //    flag that can never arrive
    for (int r = 0; r < x->world; ++r) {
        if (r == x->rank || x->peer[r]) continue;
        char bus[PC_XCHG_HANDLE_BYTES - 64];
        memcpy(bus, all + (size_t)r * PC_XCHG_HANDLE_BYTES + 64, sizeof(bus));
        bus[sizeof(bus) - 1] = 0;
        int pdev = -1;
        const hipError_t be = bus[0] ? hipDeviceGetByPCIBusId(&pdev, bus) : hipErrorInvalidValue;
        if (be != hipSuccess || pdev < 0)
            return fail(PC_ERR_UNSUPPORTED, "pc_xchg_connect: rank " + std::to_string(r) + "'s device (PCI " + std::string(bus) +
                        ") is not visible to this process (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES hide it, or the rank is on another node): "
                        "peer-mapped exchange impossible, use PPOConfig.exchange = \"rccl\"");
        if (pdev == x->device) continue;     // the same device (a one-GPU rehearsal): nothing to enable
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, x->device, pdev) != hipSuccess || !can)
            return fail(PC_ERR_UNSUPPORTED, "pc_xchg_connect: device " + std::to_string(x->device) + " has no peer access to rank " + std::to_string(r) +
                        "'s device " + std::to_string(pdev) + " (PCI " + std::string(bus) + "; xGMI / PCIe P2P unavailable): use PPOConfig.exchange = \"rccl\"");
        const hipError_t pe = hipDeviceEnablePeerAccess(pdev, 0);
        (void)hipGetLastError();     // (hipErrorPeerAccessAlreadyEnabled is sticky otherwise)
        if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled)
            return fail(PC_ERR_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(pe));
    }
    // 2. map the peers' staging buffers
    for (int r = 0; r < x->world; ++r) {
        if (r == x->rank || x->peer[r]) continue;
        hipIpcMemHandle_t h;
        memcpy(&h, all + (size_t)r * PC_XCHG_HANDLE_BYTES, sizeof(h));
        void* q = nullptr;
        const hipError_t oe = hipIpcOpenMemHandle(&q, h, hipIpcMemLazyEnablePeerAccess);
        if (oe != hipSuccess || !q) return fail(PC_ERR_HIP, std::string("hipIpcOpenMemHandle(rank ") + std::to_string(r) + "): " + hipGetErrorString(oe));
        x->peer[r] = static_cast<char*>(q);
        x->ipc[r] = true;
        opened.push_back(r);
    }
    x->connected = true;
    return PC_OK;
}

// The same exchange with every rank's handle in THIS process (one process driving several devices, or -- the tests' use -- several
// ranks on one device, each on its own stream): the peers' staging buffers are plain pointers here, no IPC handle is involved.
int pc_xchg_connect_local(pc_xchg* x, pc_xchg* const* ranks) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!x || !ranks) return PC_ERR_INVALID_ARG;
    for (int r = 0; r < x->world; ++r) {
        const pc_xchg* q = ranks[r];
        if (!q || q->rank != r || q->world != x->world || q->n != x->n || (r == x->rank && q != x)) return PC_ERR_INVALID_ARG;
    }
    DeviceGuard guard(x->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    for (int r = 0; r < x->world; ++r) {
        if (r == x->rank || ranks[r]->device == x->device) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, x->device, ranks[r]->device) != hipSuccess || !can) {
            g_hip_err = "pc_xchg_connect_local: device " + std::to_string(x->device) + " has no peer access to device " + std::to_string(ranks[r]->device);
            return PC_ERR_UNSUPPORTED;
        }
        const hipError_t pe = hipDeviceEnablePeerAccess(ranks[r]->device, 0);
        (void)hipGetLastError();
        if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) {
            g_hip_err = std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(pe);
            return PC_ERR_HIP;
        }
    }
    for (int r = 0; r < x->world; ++r)
        if (r != x->rank) { x->peer[r] = ranks[r]->local; x->ipc[r] = false; }
    x->connected = true;
    return PC_OK;
}

int pc_xchg_set_timeout(pc_xchg* x, double seconds) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!x || !(seconds > 0.0) || seconds > 3600.0) return PC_ERR_INVALID_ARG;
    x->timeout_s = seconds;
    return PC_OK;
}

int pc_xchg_allreduce(pc_xchg* x, float* bucket, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!x || !bucket) return PC_ERR_INVALID_ARG;
    if (!x->connected) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(x->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    hipLaunchKernelGGL(xchg_allreduce_kernel, dim3(x->n_chunks), dim3(256), 0, (hipStream_t)stream, x->view(), bucket);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_xchg_allreduce_group(pc_xchg* const* ranks, float* const* buckets, void* stream) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!ranks || !buckets || !ranks[0]) return PC_ERR_INVALID_ARG;
    const int W = ranks[0]->world;
    XchgGroup g = {};
    for (int r = 0; r < W; ++r) {
        const pc_xchg* x = ranks[r];
        // one device, one launch: every rank's handle connected in this process, all on the launching device
        if (!x || !buckets[r] || x->rank != r || x->world != W || x->n != ranks[0]->n || !x->connected || x->device != ranks[0]->device) return PC_ERR_INVALID_ARG;
        for (int q = 0; q < W; ++q)
            if (x->peer[q] != ranks[q]->local) return PC_ERR_INVALID_ARG;      // (connected to THESE handles: pc_xchg_connect_local)
        g.v[r] = x->view();
        g.bucket[r] = buckets[r];
    }
    DeviceGuard guard(ranks[0]->device);
    if (!guard.ok) return PC_ERR_NO_DEVICE;
    // a workgroup waits for the same chunk's workgroups of the other ranks: the whole grid must be resident at once
    int per_cu = 0, cus = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, xchg_allreduce_group_kernel, 256, 0));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ranks[0]->device));
    if ((int64_t)ranks[0]->n_chunks * W > (int64_t)per_cu * cus) {
        g_hip_err = "pc_xchg_allreduce_group: " + std::to_string((int64_t)ranks[0]->n_chunks * W) + " workgroups cannot be co-resident on " +
                    std::to_string(cus) + " compute units";
        return PC_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(xchg_allreduce_group_kernel, dim3(ranks[0]->n_chunks, W), dim3(256), 0, (hipStream_t)stream, g);
    HIPCHK(hipGetLastError());
    return PC_OK;
}

int pc_xchg_status(pc_xchg* x) {
    g_hip_err.clear();   // (pc_last_hip_error speaks of THIS call)
    if (!x) return PC_ERR_INVALID_ARG;
    DeviceGuard guard(x->device);
    int err = 0;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(&err, x->view().error, sizeof(int), hipMemcpyDeviceToHost));
    return err ? PC_ERR_TIMEOUT : PC_OK;
}

void pc_xchg_destroy(pc_xchg* x) {
    if (!x) return;
    DeviceGuard guard(x->device);
    (void)hipDeviceSynchronize();
    for (int r = 0; r < x->world; ++r)
        if (r != x->rank && x->peer[r] && x->ipc[r]) (void)hipIpcCloseMemHandle(x->peer[r]);
    (void)hipFree(x->local);
    delete x;
}

}  // extern "C"
