/*
 * ppocar.h -- C-ABI of the MI355X-native CarEnv hot path (libppocar.so).
 *
 * The reference (ProfessorNova/PPO-Car) is pure Python and has no FFI layer; the boundary
 * this library sits behind is the gymnasium vector-env protocol exactly as train.py uses
 * it, plus Buffer.calculate_advantages.  Each entry point names the reference interface
 * it replaces (file:line in the reference tree).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, int status return: 0 = PC_OK, negative = error
 *     (pc_strerror).  No exceptions cross the boundary.
 *   - Array arguments of pc_env_reset/pc_env_step/pc_gae/pc_sample are DEVICE pointers owned
 *     by the caller (e.g. torch tensors) on the device the handle was created for; they must
 *     stay alive until the stream has executed the call.  The library owns only its opaque
 *     handles and the env state inside them.
 *   - Launches are asynchronous on the caller-supplied hipStream_t (`stream`, NULL = the
 *     default stream).  The library never synchronises in reset/step/gae/sample.
 *   - There is NO CPU fallback: every compute entry point needs a gfx950 device and fails
 *     with PC_ERR_NO_DEVICE / PC_ERR_HIP otherwise.
 *   - One handle per device; a handle is not thread-safe; different handles are independent.  The library keeps NO process-wide
 *     state: every launch option lives in a handle (pc_policy: arithmetic form and work decomposition of the policy step;
 *     pc_env: pc_env_set_option).
 */
#ifndef PPOCAR_H
#define PPOCAR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PC_OK 0
#define PC_ERR_INVALID_ARG (-1)
#define PC_ERR_IO (-2)          /* track file missing / unreadable (the reference prints and returns None, car_env.py:624-628; here it is a hard error) */
#define PC_ERR_PARSE (-3)       /* track JSON malformed or schema violated */
#define PC_ERR_HIP (-4)         /* a HIP runtime call failed */
#define PC_ERR_UNSUPPORTED (-5) /* e.g. more rays than the kernel menu covers */
#define PC_ERR_NO_DEVICE (-6)   /* no usable gfx950 device */
#define PC_ERR_TIMEOUT (-7)     /* pc_xchg: a peer rank did not arrive at the gradient exchange */

#define PC_DTYPE_F32 0 /* float64 kinematic state; every ray's wall segment SELECTED in float32, its distance (the observation
                        * entry, the < 10 px tests) recomputed in float64 under the reference's strict test: the throughput path */
#define PC_DTYPE_F64 1 /* float64 throughout, in the reference's operation order, with glibc's cos / sin values looked up for every
                        * angle an episode can reach (up to 16 tracks per handle; other angles use the device's): the exact-parity
                        * path -- observations, rewards, events and the float64 state equal the reference's bit for bit.  (Where a
                        * float32 sweep runs first it only chooses WHICH wall's literal cast is evaluated; every produced value is
                        * the literal arithmetic's.) */

typedef struct pc_track pc_track;
typedef struct pc_env pc_env;
typedef struct pc_policy pc_policy;
typedef struct pc_xchg pc_xchg;

/* ---- track data: CarEnv.load_track (car_env.py:535-567) + the wall / gate lists that
 * CarEnv.reset builds (car_env.py:651-676).  Host-side, no GPU needed. ------------------ */

/* Parse a track JSON file (schema written by track_editor.py:50-56,126-127): scales x by
 * 1280 and y by 720, builds walls = outer segments then inner segments and gates = consecutive
 * point pairs. */
int pc_track_load_json(const char* path, pc_track** out);
/* Same from memory: walls [S][4], gates [G][4] = x1,y1,x2,y2 in pixels. */
int pc_track_from_arrays(const double* walls, int n_walls, const double* gates, int n_gates, double start_x,
                         double start_y, double start_angle_deg, pc_track** out);
/* *n_walls, *n_gates, start[3] = {x, y, angle_deg}; any pointer may be NULL. */
int pc_track_info(const pc_track* t, int* n_walls, int* n_gates, double* start);
/* Copy the geometry out (host): walls [S][4], gates [G][4]; either may be NULL. */
int pc_track_geometry(const pc_track* t, double* walls, double* gates);
void pc_track_destroy(pc_track* t);

/* ---- the vector environment: gym.vector.AsyncVectorEnv([make_env]*N) (train.py:138-139)
 * of CarEnv (car_env.py:472-760) wrapped in TransformReward (train.py:65,68). ------------ */

/* number of rays the reference generates for a nominal `num_rays`: len(range(0, 360, 360 // n))
 * (car_env.py:269) -- 12 -> 12, 16 -> 17, 32 -> 33.  Negative on invalid n. */
int pc_ray_count(int num_rays_nominal);

/* Create n_envs environments on `device` (HIP ordinal).  `tracks`/`n_tracks`: the track table;
 * `track_id` (host, [n_envs], may be NULL = all on track 0) picks each env's track -- the
 * reference allows a different track per env through reset(options=...) (car_env.py:621-628).
 * Replaces: CarEnv.__init__ (car_env.py:475-533) x N + AsyncVectorEnv construction.
 * F32 handles check what their float32 selector assumes of a track (car_env.py:155-184 puts no constraint on the walls): the
 * walls' bounding box must fit 2000 px and a track may have at most 8192 chain vertices (PC_ERR_UNSUPPORTED; pc_last_hip_error
 * names the track's index and which of the two limits it breaks: use PC_DTYPE_F64); walls that cross or touch without being chain neighbours, spikes sharper than ~13 degrees and
 * walls shorter than the corner margin are accepted and resolved exactly (every ray that selects one of them takes the float64
 * scan of the whole chain): slower on those rays, never different from the reference. */
int pc_env_create(int device, int64_t n_envs, int num_rays_nominal, const pc_track* const* tracks, int n_tracks,
                  const uint8_t* track_id, int dtype, pc_env** out);
void pc_env_destroy(pc_env* e); /* envs.close() (train.py:296) */

int pc_env_obs_dim(const pc_env* e);    /* 6 + R: envs.single_observation_space.shape[0] (train.py:141) as the reference actually produces it */
int pc_env_num_actions(const pc_env* e); /* 9: envs.single_action_space.n (train.py:142, car_env.py:525) */
int64_t pc_env_num_envs(const pc_env* e);

/* envs.reset(options={"track_path": p}) (train.py:159; CarEnv.reset car_env.py:605-691):
 * every env to its track's start state; obs [n_envs][D] float32 (device). */
int pc_env_reset(pc_env* e, float* obs, void* stream);

/* envs.step(actions) (train.py:185): CarEnv.step (car_env.py:693-760) for every env, reward *
 * reward_scale (TransformReward, train.py:65,68; computed in float64 then rounded to float32
 * exactly as `rew_buf[ptr] = rew` does, buffer.py:29), and gymnasium's same-step auto-reset:
 * an env that terminated or truncated is reset and `obs` holds its reset observation.
 *   actions     [N] int64, values 0..8 (anything else is treated as 8 = do nothing, car_env.py:721)
 *   obs         [N][D] float32   -- may point straight into Buffer.obs_buf[t+1]
 *   reward, terminated, truncated  [N] float32 (flags 0.0 / 1.0, what train.py:191-192 builds)
 *   gates_passed [N] int32 or NULL -- info["gates_passed"] of the step (before auto-reset)
 *   final_obs   [N][D] float32 or NULL -- the observation CarEnv.step itself returned
 *                                         (gymnasium's info["final_observation"] on done envs) */
int pc_env_step(pc_env* e, const int64_t* actions, double reward_scale, float* obs, float* reward,
                float* terminated, float* truncated, int32_t* gates_passed, float* final_obs, void* stream);

/* T successive pc_env_step calls as ONE call -- `for t in range(T): envs.step(actions[t])`, the env alone under pre-generated
 * actions (SURVEY 8(d)'s level (i)); train.py:185 without the policy in front of it.  actions [T][N] int64; row t of obs [T][N][D],
 * reward / terminated / truncated [T][N] = what the t-th pc_env_step writes, bit for bit, and the handle's state afterwards is the
 * state after those T calls.  Where the handle has the table-driven form (below) the T steps are ONE launch with the env state in
 * registers throughout; otherwise T launches of the per-step kernel, enqueued by this call. */
int pc_env_step_many(pc_env* e, const int64_t* actions, int64_t T, double reward_scale, float* obs, float* reward,
                     float* terminated, float* truncated, void* stream);
/* Which kernel the last pc_env_step / pc_env_step_many on this handle launched (0 before the first; both fill the same outputs bit for bit):
 *   PC_STEP_K1         env_step_kernel: any ray count 4..360, any track, per-env track ids; 2^k lanes per env chosen from the batch size
 *   PC_STEP_K1F        env_steps_fast_kernel: the table-driven env step of the persistent rollout kernel -- 12 / 16 / 32 nominal rays, the
 *                      track's gather tables staged in LDS per launch (mixed batches: one track per workgroup, or two tracks interleaved in
 *                      evenly split blocks of 64 envs, de-interleaved by wave), 2 lanes per env, the chain-packed / unrolled selector sweep; F64
 *                      handles: its literal form (tracks inside the selector's limits, rotations on the rotation table).  Taken by
 *                      pc_env_step from 8192 envs on, by pc_env_step_many at any batch size; PC_OPT_STEP_FORM decides otherwise
 *   PC_STEP_K1F_TABLE  the same with the track's 1/den table staged too (pc_env_step_many, T > 1, when it fits) */
#define PC_STEP_NONE 0
#define PC_STEP_K1 1
#define PC_STEP_K1F 2
#define PC_STEP_K1F_TABLE 3
int pc_env_last_step_kernel(const pc_env* e);

/* CarEnv._get_info (car_env.py:599-603) of every env's CURRENT state: info["gates_passed"] and info["time_passed"]
 * as the vector env's `infos` hold them after a step (an env auto-reset in that step reports its reset state, 0 / 0;
 * the finished episode's count is pc_env_step's `gates_passed`).  [N] int32 device arrays, either may be NULL. */
int pc_env_info(pc_env* e, int32_t* gates_passed, int32_t* time_passed, void* stream);

/* ---- observing without stepping (opt-in: the entry points above are untouched): CarEnv._get_obs (car_env.py:569-597) and
 * Car.check_collision (car_env.py:376-392) for poses the caller names.  One launch of one kernel; the env state is neither read
 * (pc_env_observe_poses) nor written (both).  Every ray is measured against the track's WHOLE wall list in float64 -- poses may
 * lie on a wall, on a vertex or outside the track --, F32 handles by the float64 chain scan the step's refinement falls back to,
 * which reports the bits the step reports: pc_env_observe right after a pc_env_step returns that step's observation, bit for
 * bit (an env the step auto-reset shows its reset observation).  F64 handles: the reference's own arithmetic.
 * pc_env_observe_poses: M poses, all DEVICE arrays of M entries.  M is independent of the handle's n_envs.
 *   px, py      float64 position in pixels (Car.position); any value, the frame is not enforced (car_env.py:578-579 do not either)
 *   vx, vy      float64 velocity in px per step, or NULL = 0: only entries 2-3 of the observation depend on it (:580-581)
 *   turns       int32: the heading is the track's start angle + 5 degrees * turns (Car.move_car only ever adds +-5.0,
 *               car_env.py:440-442).  F32 handles take any count (the heading tables are periodic in 72).  F64 handles: a count in
 *               -1000 .. 1000 (an episode makes at most PC_TIME_LIMIT turns) means the float64 rotation the start angle becomes after
 *               that many turns ONE way, every sum rounded as Car.move_car rounds it; each of them is a row of the handle's rotation
 *               table, so cos / sin are glibc's, the reference's bits.  (A car that turned both ways can hold a rotation a few ulps
 *               from it.)  A count outside that range takes start_angle + 5.0 * turns through the angle hash where it holds the
 *               angle and the device's cos / sin otherwise (last-place differences from glibc are possible there).
 *   track_id    uint8, or NULL = track 0.  A pose whose track_id >= the handle's track count gets a row of zeros and collides = 0.
 *   obs         [M][D] float32: entries 0-3 = x / 1280, y / 720, vx / 10, vy / 10 (:578-581), 4-5 = cos / sin of the heading
 *               (:584-588), 6 .. = each ray's min(distance, 1000) / 1000 (:590-595)
 *   collides    [M] uint8 or NULL: 1 iff one of check_collision's rays, r in range(0, n, n // 4) (:389), is shorter than 10 px (:390)
 * pc_env_observe: the same for the handle's CURRENT state, obs [n_envs][D], collides [n_envs] or NULL; the heading is taken from
 *   the state as pc_env_step takes it.  The state is not modified.
 * Checked before any device call, in this order: NULL handle, NULL px / py / turns / obs or M < 1 (pc_env_observe: NULL handle or
 * obs): PC_ERR_INVALID_ARG; then as pc_env_step.  Neither call synchronises. */
int pc_env_observe_poses(const pc_env* e, const double* px, const double* py, const double* vx, const double* vy,
                         const int32_t* turns, const uint8_t* track_id, int64_t M, float* obs, uint8_t* collides, void* stream);
int pc_env_observe(pc_env* e, float* obs, uint8_t* collides, void* stream);

/* ---- stepping without committing (opt-in: the entry points above are untouched): one CarEnv.step (car_env.py:693-760) of M states the
 * caller names, on the handle's tracks.  One launch of one kernel (K20); no auto-reset; the handle's own env state is neither read
 * nor written.  All arrays are DEVICE arrays of M entries, obs is [M][D]; M is independent of the handle's n_envs.
 *   px, py, vx, vy        float64, IN / OUT: position in pixels and velocity in px per step
 *   turns                 int32, IN / OUT: the heading, pc_env_observe_poses' rule; out: turns - 1 (a left turn), + 1 (right) or as it was
 *   next_gate, time_step  int32, IN / OUT.  Only gate[next_gate] can fire; the last gate wraps next_gate to 0.  A next_gate outside
 *                         0 .. G - 1 of the row's track: no gate can fire, the value is left as it is.
 *     After the call the seven arrays hold the state CarEnv.step leaves -- also for a row that terminated or truncated: nothing is
 *     reset, the position is the pose of the impact.  The update is IN PLACE: the arrays must not overlap one another.
 *   actions     int64: CarEnv's 0 .. 8; anything else acts as 8 (no thrust, no turn)
 *   track_id    uint8, or NULL = track 0            active   uint8, or NULL = every row
 *   obs         [M][D] float32: the observation CarEnv.step itself returned (what pc_env_step writes to final_obs)
 *   reward      float32, (float)(r * reward_scale) as pc_env_step scales and rounds it
 *   terminated, truncated   uint8 0 / 1: a wall was hit; else time_step + 1 >= PC_TIME_LIMIT
 *   gate        uint8 0 / 1 or NULL: a gate fired in this step (a lap closed iff gate and the new next_gate is 0)
 * Rows that are not stepped: active[m] == 0 -- NOTHING of the row is written, in any array; a track_id the handle does not have --
 * obs row zeros, reward 0, flags 0, the state untouched.
 * Bits: on an F32 handle obs / reward / flags / the new state are pc_env_step's for the same state and action (the wall distances by
 * the exhaustive float64 scan pc_env_observe_poses takes, so states on a wall or outside the track are fine).  On an F64 handle they
 * are the reference's from any rotation `turns` names: the turn itself is the literal rot +- 5.0 of Car.move_car.  The new count
 * turns +- 1 names the ONE-WAY rotation again, so a chained call after a turn back re-enters that row, which can lie a few ulps from
 * rot +- 5.0 (on big_track 10 of 2000 turn-backs differ, on track 6, on oval64 4): as pc_env_observe_poses, a car that turned both
 * ways can hold a rotation the count does not name.
 * Checked before any device call, in this order: NULL handle; NULL px / py / vx / vy / turns / next_gate / time_step / actions / obs /
 * reward / terminated / truncated; M < 1; reward_scale not finite: PC_ERR_INVALID_ARG; then as pc_env_observe_poses.  The call never
 * synchronises. */
int pc_env_step_poses(const pc_env* e, double* px, double* py, double* vx, double* vy, int32_t* turns, int32_t* next_gate,
                      int32_t* time_step, const uint8_t* track_id, const int64_t* actions, const uint8_t* active, int64_t M,
                      double reward_scale, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated, uint8_t* gate,
                      void* stream);

/* ---- safe-action masks (opt-in: the entry points above are untouched): which of the 9 actions can still avoid a crash within `depth`
 * steps.  With step = CarEnv.step without auto-reset, as pc_env_step_poses defines it:
 *   safe(s, a, 1) = not terminated(step(s, a))
 *   safe(s, a, d) = not terminated(s' = step(s, a)) and (truncated(s') or exists a' in 0 .. 8: safe(s', a', d - 1))
 * A branch that reaches the time limit without a crash ended its episode alive: safe.  `terminated` is pc_env_step_poses': one of
 * check_collision's rays r in range(0, n, n // 4) at the NEW pose is shorter than 10 px, or the track's start pose collides.  Gates
 * and rewards play no part.  One launch of one kernel (K21): an exhaustive search over the action sequences, one lane per (state, first
 * action), the state in registers, no observation computed or stored; a level ends at its first surviving action.
 * pc_env_safe_actions: M states, all DEVICE arrays of M entries, read only; M is independent of the handle's n_envs and the handle's
 * env state is not read.
 *   px, py, vx, vy   float64 position and velocity         turns   int32, pc_env_observe_poses' heading rule
 *   time_step        int32, or NULL = 0                     track_id   uint8, or NULL = track 0        active   uint8, or NULL = every row
 *   depth            1 .. PC_SAFE_MAX_DEPTH: the worst case is 9 + 81 + 729 + 6561 crash tests per state at depth 4
 *   safe             [M][9] uint8, 0 / 1.  active[m] == 0: the row's 9 bytes are not written.  A track_id the handle does not have: 9 zeros.
 * pc_env_safe_actions_state: the same for the handle's CURRENT state, safe [n_envs][9]; the heading is taken from the state as
 *   pc_env_step takes it.  The state is not modified.
 * Bits: on an F32 handle safe[m][a] is what enumerating all action sequences with chained pc_env_step_poses calls on that handle gives
 * (the turn count is periodic there, so the chain is exact).  On an F64 handle it is that enumeration on the reference from the rotation
 * `turns` names: inside the search the heading moves as Car.move_car moves it, the literal rot +- 5.0, and never re-enters the one-way
 * row of a count -- exact also where chained pc_env_step_poses calls are a few ulps off after a turn back (the note above).
 * Checked before any device call, in this order: NULL handle; NULL px / py / vx / vy / turns / safe; M < 1; depth outside 1 ..
 * PC_SAFE_MAX_DEPTH (pc_env_safe_actions_state: NULL handle or safe; depth): PC_ERR_INVALID_ARG; then as pc_env_observe_poses.
 * Neither call synchronises. */
#define PC_SAFE_MAX_DEPTH 4
int pc_env_safe_actions(const pc_env* e, const double* px, const double* py, const double* vx, const double* vy,
                        const int32_t* turns, const int32_t* time_step, const uint8_t* track_id, const uint8_t* active, int64_t M,
                        int depth, uint8_t* safe, void* stream);
int pc_env_safe_actions_state(pc_env* e, int depth, uint8_t* safe, void* stream);

/* ---- scoring action sequences (opt-in: the entry points above are untouched): what each of K action sequences of H steps earns from
 * each of M states.  With step = CarEnv.step without auto-reset, as pc_env_step_poses defines it, sequence k of state m is stepped
 * until it terminates, truncates or has taken its H steps; an ended sequence takes no further step and adds nothing.  One launch of
 * one kernel (K22), one lane per (state, sequence), the state in registers, no observation computed or stored; where a best_* array
 * is asked for, a second small launch in the same call picks each state's best sequence.
 * pc_env_rollout_sequences: M states, all DEVICE arrays of M entries, read only; M is independent of the handle's n_envs and the
 * handle's env state is not read.
 *   px, py, vx, vy   float64 position and velocity         turns   int32, pc_env_observe_poses' heading rule
 *   next_gate        int32, or NULL = 0 (pc_env_step_poses' rule: only gate[next_gate] can fire)         time_step   int32, or NULL = 0
 *   track_id         uint8, or NULL = track 0               active  uint8, or NULL = every row
 *   actions          uint8, TIME-MAJOR [H][K]: entry (t, k) is the action of sequence k in its step t; anything outside 0 .. 8 acts
 *                    as 8.  actions_state_stride == 0: one table shared by all states; == H * K (bytes): M tables, state m's at
 *                    actions + m * H * K.  Any other stride is refused.
 *   K                1 .. PC_SEQ_MAX_CANDIDATES             H   1 .. PC_TIME_LIMIT
 *   reward_scale     each step's reward is (float)(r * reward_scale), as pc_env_step scales and rounds it
 * Per (state, sequence), [M][K]:
 *   ret      float64: the sum, in step order, of those float32 rewards widened to double
 *   steps    int32: steps taken, 1 .. H
 *   status   uint8: PC_FIRST_RUNNING, PC_FIRST_TERMINATED or PC_FIRST_TRUNCATED after the last step taken (a crash in the step in which
 *            the time limit falls due: TERMINATED)
 *   gates, laps   int32 or NULL: gates fired; gates that wrapped next_gate to 0
 * Per state, [M], each or NULL:
 *   best_k        int32: the LOWEST k whose ret is the row's maximum, compared as float64
 *   best_action   int64: that sequence's first action after the 0 .. 8 mapping, ready for pc_env_step
 *   best_ret      float64: ret[m][best_k]
 * Rows that are not rolled out: active[m] == 0 -- NOTHING of the row is written, in any output array; a track_id the handle does not
 * have -- ret 0, steps 0, status PC_FIRST_RUNNING, gates and laps 0, best_k 0, best_action 8, best_ret 0.
 * pc_env_rollout_sequences_state: the same for the handle's CURRENT state (M = n_envs, its own next_gate, time_step and track ids);
 *   the heading is taken from the state as pc_env_step takes it.  The state is not modified.
 * Bits: on an F32 handle every output is what H chained pc_env_step_poses calls on that handle give for the replicated rows (the turn
 * count is periodic there, so the chain is exact).  On an F64 handle it is the reference's from the rotation `turns` names: inside a
 * sequence the heading moves as Car.move_car moves it, the literal rot +- 5.0, as in pc_env_safe_actions.
 * Checked before any device call, in this order: NULL handle; NULL px / py / vx / vy / turns / actions / ret / steps / status
 * (pc_env_rollout_sequences_state: actions / ret / steps / status); M < 1; K outside 1 .. PC_SEQ_MAX_CANDIDATES; H outside 1 ..
 * PC_TIME_LIMIT; a stride other than 0 or H * K; reward_scale not finite: PC_ERR_INVALID_ARG; then as pc_env_observe_poses.  Neither
 * call synchronises. */
#define PC_SEQ_MAX_CANDIDATES 4096
int pc_env_rollout_sequences(const pc_env* e, const double* px, const double* py, const double* vx, const double* vy,
                             const int32_t* turns, const int32_t* next_gate, const int32_t* time_step, const uint8_t* track_id,
                             const uint8_t* active, int64_t M, const uint8_t* actions, int64_t actions_state_stride, int K, int H,
                             double reward_scale, double* ret, int32_t* steps, uint8_t* status, int32_t* gates, int32_t* laps,
                             int32_t* best_k, int64_t* best_action, double* best_ret, void* stream);
int pc_env_rollout_sequences_state(pc_env* e, const uint8_t* actions, int64_t actions_state_stride, int K, int H, double reward_scale,
                                   double* ret, int32_t* steps, uint8_t* status, int32_t* gates, int32_t* laps, int32_t* best_k,
                                   int64_t* best_action, double* best_ret, void* stream);

/* ---- scoring action sequences with a discount and the critic's value of the state they end in (opt-in: the entry points above are
 * untouched): the n-step return plus gamma^n * V(end state), the quantity the PPO loop's GAE estimates.  Three launches on the stream:
 * K25 (K22's lane and loop with the discount, then the observation of the lane's end state), the policy step over end_obs, K26 (the
 * combination and each state's best sequence).  Every argument pc_env_rollout_sequences[_state] takes keeps its meaning and its rules;
 * in addition:
 *   gamma        double, finite, 0 <= gamma <= 1
 *   bootstrap    PC_SEQ_BOOTSTRAP_NONE: no lane; PC_SEQ_BOOTSTRAP_RUNNING: the lanes whose status is PC_FIRST_RUNNING after their last
 *                step; PC_SEQ_BOOTSTRAP_RUNNING_TRUNCATED: those and the lanes that ended at the time limit (PC_FIRST_TRUNCATED), the
 *                planning-side twin of the PPO loop's truncation_bootstrap = "final_obs".  A terminated lane is never bootstrapped,
 *                a crash in the step in which the time limit falls due included.
 *   p, image     the policy handle and the weight image it packed (pc_policy_pack), or NULL and NULL: allowed only with
 *                PC_SEQ_BOOTSTRAP_NONE.  With a policy given, its D must be the env handle's obs dim and its device the env handle's.
 *   workspace    DEVICE memory of pc_env_rollout_sequences_value_workspace(M, K) bytes, 16-byte aligned, for what the policy step
 *                writes besides the value (its actions and log-probabilities); required with a policy, else ignored (may be NULL).
 *                Nothing is allocated inside the call.  pc_env_rollout_sequences_value_workspace returns 0 for M < 1 or K outside
 *                1 .. PC_SEQ_MAX_CANDIDATES.
 * New outputs, per (state, sequence), [M][K], after the existing ones:
 *   end_obs        float32 [M][K][D]: required with a policy, else optional
 *   end_value      float32: required with a policy; without one it is not written
 *   end_discount   float64 or NULL
 *   ret_env        float64 or NULL
 * Definitions.  Every arithmetic step is a separately rounded IEEE float64 operation, never contracted into an fma, so that plain numpy
 * reproduces the bits:
 *   ret = 0.0; disc = 1.0
 *   every step a lane takes:   ret  = ret + disc * (double)r      r = the float32 scaled reward, as pc_env_rollout_sequences has it
 *                              disc = disc * gamma
 *   after its last step:       ret_env = ret;  end_discount = disc
 *   end_obs[m][k]   = the observation CarEnv.step returned in the lane's LAST step taken: the observation of the pose the lane ends at
 *                     (F32 handle: pc_env_step_poses' bits; F64 handle: the reference's), for every rolled-out lane, terminated ones
 *                     included (the pose of the impact)
 *   end_value       = what ONE pc_policy_act_greedy call over end_obs viewed as N = M * K rows writes to `value` (the form, and
 *                     therefore the last bits, depend on N: it is one call, not one per state)
 *   ret[m][k]       = ret_env + end_discount * (double)end_value      where the mode bootstraps the lane's status; else ret_env
 *   best_k / best_action / best_ret: pc_env_rollout_sequences' rule (the lowest k of the maximum, compared as float64) on this ret
 * Consequences:
 *   - with gamma == 1.0, PC_SEQ_BOOTSTRAP_NONE and no policy every output equals pc_env_rollout_sequences' bit for bit;
 *   - steps, status, gates and laps never depend on gamma, bootstrap or the policy;
 *   - active[m] == 0: the row is not written in any array except end_value, which holds the policy step's output for whatever the
 *     caller's end_obs memory held there and is unspecified;
 *   - a track_id the handle does not have: pc_env_rollout_sequences' zeros, an end_obs row of zeros, end_discount 1, ret_env 0; the
 *     lane is never bootstrapped (end_value is the policy's value of the zero observation).
 * The second launch (K26) runs whenever a policy is given or a best_* array is asked for.
 * Checked before any device call, in this order: everything pc_env_rollout_sequences[_state] checks, in its order; gamma not finite or
 * outside 0 .. 1; a bootstrap other than the three; one of p / image NULL and the other not; a bootstrap without a policy; a policy
 * without end_obs, end_value or workspace; a policy whose D or device is not the env handle's:
 * PC_ERR_INVALID_ARG; then as pc_env_rollout_sequences and pc_policy_act_greedy.  Neither call synchronises. */
#define PC_SEQ_BOOTSTRAP_NONE 0
#define PC_SEQ_BOOTSTRAP_RUNNING 1
#define PC_SEQ_BOOTSTRAP_RUNNING_TRUNCATED 2
int64_t pc_env_rollout_sequences_value_workspace(int64_t M, int K);
int pc_env_rollout_sequences_value(const pc_env* e, const double* px, const double* py, const double* vx, const double* vy,
                                   const int32_t* turns, const int32_t* next_gate, const int32_t* time_step, const uint8_t* track_id,
                                   const uint8_t* active, int64_t M, const uint8_t* actions, int64_t actions_state_stride, int K, int H,
                                   double reward_scale, double gamma, int bootstrap, const pc_policy* p, const float* image,
                                   void* workspace, double* ret, int32_t* steps, uint8_t* status, int32_t* gates, int32_t* laps,
                                   int32_t* best_k, int64_t* best_action, double* best_ret, float* end_obs, float* end_value,
                                   double* end_discount, double* ret_env, void* stream);
int pc_env_rollout_sequences_value_state(pc_env* e, const uint8_t* actions, int64_t actions_state_stride, int K, int H,
                                         double reward_scale, double gamma, int bootstrap, const pc_policy* p, const float* image,
                                         void* workspace, double* ret, int32_t* steps, uint8_t* status, int32_t* gates, int32_t* laps,
                                         int32_t* best_k, int64_t* best_action, double* best_ret, float* end_obs, float* end_value,
                                         double* end_discount, double* ret_env, void* stream);

/* Per-handle launch options of pc_rollout (below).  Every choice gives bit-identical buffers; they exist so that the variant a
 * benchmark size takes can be checked at other batch sizes, and for A/B timing.
 *   PC_OPT_ROLLOUT_FORM  -1 (default) automatic: above 8192 envs independent waves of 32 envs, 256 envs per workgroup (128 up to
 *                        32768 envs), else 16 / 32 envs per workgroup with the policy's hidden tiles and the wall sweep split over the
 *                        waves; between 8193 and 32768 envs at 16 rays the first form with 16 envs per wave; 0 / 1 force the first /
 *                        second form, 4 the 16-envs-per-wave one (where the shape has it); 2 / 3 = forms 0 / 1 with the env step forming 1/den
 *                        arithmetically instead of reading the track's 1/den table from LDS (what happens anyway when it does not fit)
 *   PC_OPT_ROLLOUT_EPW   envs per workgroup: 0 (default) automatic; 128 / 256 force the big form's choice, 16 / 32 the small form's
 *   PC_OPT_ROLLOUT_FAST  1 (default) = batches whose workgroups each lie on one track take the mode whose gather tables sit in LDS
 *                        behind LDS pointers -- at 16 (17) rays in the kernels compiled for the chain layout of the reference's tracks
 *                        when every track of the batch has it; 2 = that mode but never those specialised kernels; 0 = always the
 *                        generic mode (what mixed-track batches whose workgroups straddle tracks take).  F64 handles: 1 / 2 = the
 *                        selector form (with / without the specialised sweeps), 0 = the filter form.  3 = as 1, but two tracks interleaved
 *                        in evenly split blocks keep the per-track passes inside every wave instead of being de-interleaved by wave
 *                        (what unevenly interleaved batches take anyway; a test / timing knob) */
#define PC_OPT_ROLLOUT_FORM 1
#define PC_OPT_ROLLOUT_EPW 2
#define PC_OPT_ROLLOUT_FAST 3
/*   PC_OPT_STEP_FORM     pc_env_step / pc_env_step_many: 0 (default) automatic (see PC_STEP_K1F), 1 = always PC_STEP_K1, 2 = PC_STEP_K1F
 *                        wherever the handle has it, at any batch size */
#define PC_OPT_STEP_FORM 4
int pc_env_set_option(pc_env* e, int option, int value);
int pc_env_get_option(const pc_env* e, int option, int* value);

/* Teacher forcing for parity tests: copy the env state from / to HOST arrays of length n_envs
 * (any pointer may be NULL).  `rot` is the heading in degrees.  Synchronous.
 * F32 handles store the heading as a count of 5-degree turns from the track's start angle
 * (Car.move_car only ever adds +-5.0, car_env.py:440-442), so set_state rounds `rot` to that grid. */
int pc_env_get_state(pc_env* e, double* px, double* py, double* vx, double* vy, double* rot, int64_t* time_step,
                     int64_t* next_gate, int64_t* passed);
int pc_env_set_state(pc_env* e, const double* px, const double* py, const double* vx, const double* vy,
                     const double* rot, const int64_t* time_step, const int64_t* next_gate, const int64_t* passed);

/* ---- Buffer.calculate_advantages (buffer.py:36-64): GAE(lambda) with separate terminated /
 * truncated masks, float32, same operation order as the reference's torch expression (bit-exact
 * with it).  rew, val, term, trunc, adv, ret: [T][N] row-major; last_*: [N].  All device. */
int pc_gae(int device, const float* rew, const float* val, const float* term, const float* trunc,
           const float* last_val, const float* last_term, const float* last_trunc, double gamma, double lam,
           int64_t T, int64_t N, float* adv, float* ret, void* stream);

/* ---- episode statistics (gymnasium's RecordEpisodeStatistics: return and length, plus gates and laps decoded from each step's
 * reward k = rint(r / reward_scale): a gate iff k in {1, 11, -2, 8}, a lap iff k in {11, 8}).  Per env, float64, all device:
 *   carry [4][N] (in / out): return (scaled), length, gates, laps of the episode in progress.  Length 0 = a fresh episode;
 *                -1 = its start was not observed: the episode that closes from there is dropped and the carry restarts at 0.
 *   out   [7][N] (ACCUMULATED: the caller initialises 0, 0, 0, 0, 0, +inf, -inf): finished episodes, the sum of their scaled
 *                returns, lengths, gates, laps; min and max scaled return.  Counts are exact float64 integers; the sums are exact
 *                (every reward is an integer multiple of ulp(float(0.01 * reward_scale)); see kernels/gae_sample.hpp) while a
 *                per-env sum stays below 2^53 of those units.
 * pc_episode_stats: rew, term, trunc [T][N] float32 in one of two layouts:
 *   PC_EPISODE_BUFFER  the rollout buffer's: step t's flags in row t + 1, step T - 1's in last_term / last_trunc [N]; row 0 is not read
 *   PC_EPISODE_STEPS   pc_env_step / pc_env_step_many rows: flags[t] belong to rew[t]; last_term / last_trunc are not read (may be NULL)
 * pc_gae_episodes: pc_gae (same arguments, same adv / ret bits) with the statistics of the Buffer layout taken on the same loads.
 * reward_scale must be finite and > 0 (else PC_ERR_INVALID_ARG). */
#define PC_EPISODE_BUFFER 0
#define PC_EPISODE_STEPS 1
int pc_episode_stats(int device, const float* rew, const float* term, const float* trunc, const float* last_term,
                     const float* last_trunc, int64_t T, int64_t N, int layout, double reward_scale, double* carry, double* out,
                     void* stream);
int pc_gae_episodes(int device, const float* rew, const float* val, const float* term, const float* trunc,
                    const float* last_val, const float* last_term, const float* last_trunc, double gamma, double lam,
                    int64_t T, int64_t N, float* adv, float* ret, double reward_scale, double* carry, double* out, void* stream);

/* ---- truncation bootstrap (Pardo et al., "Time Limits in Reinforcement Learning", 2018): pc_gae with V(final observation) in place of
 * the next row's value at a time-limit truncation.  The reference bootstraps a truncated step t from val[t + 1] (buffer.py:53-61), but
 * gymnasium's same-step auto-reset has already put the reset observation in row t + 1: that value is V(start line).
 * Slots: CarEnv truncates at time >= PC_TIME_LIMIT (car_env.py:749) and any done restarts the env's time at 0, so two truncations of
 * one env are at least PC_TIME_LIMIT steps apart; the truncation of env n at rollout step t goes to slot t / PC_TIME_LIMIT, and a
 * rollout of T steps needs slots >= ceil(T / PC_TIME_LIMIT).
 *   final_val [slots][N] float32 (device): V(final observation) of env n's truncation in slot k; its values are USED only at
 *             truncated steps (trunc[t + 1][n] != 0 for t < T - 1, last_trunc[n] != 0 for t = T - 1): the other entries may hold
 *             anything, finite or not (the kernel loads them next to the rows, every entry of the [slots][N] array must be readable).
 * Per step, in the reference's float32 operation order:
 *   next_v   = truncated(t) ? final_val[t / PC_TIME_LIMIT][n] : (t == T - 1 ? last_val[n] : val[t + 1][n])
 *   delta    = (rew[t] + (gamma * next_v) * term_mask) - val[t]
 *   last_gae = delta + (((gamma * lam) * term_mask) * trunc_mask) * last_gae     (the trace is still cut at the truncation)
 * With final_val equal to the next-row values the result is pc_gae's, bit for bit.  carry / out: NULL (both) = no episode statistics;
 * else pc_gae_episodes' arrays, accumulated by the same launch (the same statistics bits).  Every argument is checked before any
 * device call; slots < ceil(T / PC_TIME_LIMIT) is PC_ERR_INVALID_ARG. */
#define PC_TIME_LIMIT 1000
int pc_gae_bootstrap(int device, const float* rew, const float* val, const float* term, const float* trunc, const float* last_val,
                     const float* last_term, const float* last_trunc, const float* final_val, int64_t slots, double gamma, double lam,
                     int64_t T, int64_t N, float* adv, float* ret, double reward_scale, double* carry, double* out, void* stream);

/* ---- Agent.get_action_and_value's sampling tail (model.py:35-40): for logits [N][A] float32
 * draw action ~ Categorical(logits) and return log_prob(action) and (optionally) the entropy.
 * Counter-based RNG (Philox-4x32-10) keyed by (seed, offset): the same (seed, offset, N, A)
 * gives the same actions on any launch geometry.  actions [N] int64, logprob/entropy [N] float32
 * (entropy may be NULL).  All device.  A <= 16, else PC_ERR_UNSUPPORTED.
 * THE STREAM (a contract: pc_sample, pc_policy_act and pc_rollout draw from it alike; tests/draw_reference.py is its plain
 * reference and tests/test_policy_draw_*.py hold the kernels to it element by element).  Draw number `offset` of element idx (the
 * element's position in THAT call, 0 .. N - 1; both 64-bit) is
 *   block   = Philox-4x32-10 (Salmon et al., Random123: multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85) of
 *             counter = (idx low 32 bits, idx high, (offset >> 2) low, (offset >> 2) high), key = (seed low, seed high)
 *   x       = word (offset & 3) of the block: four consecutive offsets of an element share one block
 *   u       = min(((float)(x >> 8) + 0.5f) * 2^-24, 1 - 2^-24) in float32: strictly inside (0, 1).  (k + 0.5 is rounded to float32
 *             for k >= 2^23; without the bound k = 2^24 - 1 gave 1.0f.)
 *   action  = the number of bins i < A - 1 of the float32 inclusive CDF of softmax(logits) with u >= cdf_i: the draw of an element
 *             depends on its logits and (seed, offset, idx), nothing else.  The last bin absorbs the rounding of the float32 CDF's
 *             end (a few ulp below 1): a last action of probability 0 can be drawn only by a u within 2e-6 of 1. */
int pc_sample(int device, const float* logits, int64_t N, int A, uint64_t seed, uint64_t offset, int64_t* actions,
              float* logprob, float* entropy, void* stream);

/* ---- the cross-entropy method around pc_env_rollout_sequences (opt-in: the entry points above are untouched): draw every state's K
 * action sequences from that state's own per-step distribution (K23), score them with pc_env_rollout_sequences on one table per state
 * (actions_state_stride = H * K), move the distributions towards the E best sequences (K24), repeat.  All arithmetic is integer: the
 * results are exact and do not depend on the launch geometry.  No env handle: a device index and a stream, as pc_sample.  All DEVICE.
 * WEIGHTS  uint32 [M][H][9]: the unnormalised probability of action a in step t of state m, 65536 = one.  Both calls read a value above
 *   65536 as 65536 and a row [9] that sums to 0 as nine ones.
 * pc_cem_sample: table uint8 [M][H][K], state m's at table + m * H * K in pc_env_rollout_sequences' time-major [H][K] layout.
 *   Element (m, t, k) has idx = (m * H + t) * K + k.  With x = word (offset & 3) of THE STREAM's block for (seed, offset >> 2, idx) -- the
 *   raw 32-bit word, not the float uniform --, S the row's weight sum and r = ((uint64_t)x * S) >> 32, the action is the least a with
 *   r < w[0] + ... + w[a].  An action of weight 0 is never drawn.
 *   const_columns != 0   columns k < min(K, 9) hold the constant action k instead
 *   keep                 uint8 [M][H] or NULL; given and K > 9: column 9 holds keep[m][t], copied as stored
 *   active               uint8 [M] or NULL = every row; NOTHING of a row with 0 is written
 * pc_cem_refit: per state, from ret [M][K] float64 (pc_env_rollout_sequences' output) and the table those returns belong to:
 *   1. the K sequences in the order "ret descending, then k ascending", values compared as float64 (-0.0 == 0.0; ret holds no NaN)
 *   2. the elites are the first E of that order
 *   3. c[t][a] = the number of elites whose table entry at step t is a (an entry above 8 counts as 8, as it acts)
 *   4. f = (c << 16) / E, integer division
 *   5. w' = min(65536, max(w_min, w - (w >> shift) + (f >> shift))), written in place (w as read: see WEIGHTS).  shift = 0 replaces the
 *      weights by the elites' frequencies, a larger shift moves them a 2^-shift part of the way
 *   6. best_seq uint8 [M][H] or NULL: the rank-0 column of the table, copied as stored
 *   active as above: a row with 0 is not touched.  ret, table and active are only read.
 *   One workgroup per state; the E-th key by 8-bit radix passes in LDS, ties at the threshold by a prefix count in k order.
 * Limits: M >= 1; H 1 .. PC_CEM_MAX_HORIZON; K 1 .. PC_SEQ_MAX_CANDIDATES; E 1 .. K; shift 0 .. 16; w_min 0 .. 65536.
 * Checked before any device call, in this order: NULL weights / table (pc_cem_refit: weights / ret / table); M < 1; H outside its
 * limits; K outside its limits; then for pc_cem_refit E, shift, w_min: PC_ERR_INVALID_ARG; then the device (PC_ERR_NO_DEVICE); a grid
 * the device cannot take (M * H * K above 2^39; pc_cem_refit: M above 2^31 - 1): PC_ERR_UNSUPPORTED.  Neither call synchronises. */
#define PC_CEM_MAX_HORIZON 256
int pc_cem_sample(int device, const uint32_t* weights, int64_t M, int H, int K, uint64_t seed, uint64_t offset, int const_columns,
                  const uint8_t* keep, const uint8_t* active, uint8_t* table, void* stream);
int pc_cem_refit(int device, uint32_t* weights, const double* ret, const uint8_t* table, int64_t M, int H, int K, int E, int shift,
                 int w_min, const uint8_t* active, uint8_t* best_seq, void* stream);

/* ---- per-action returns of a score table (opt-in; K28): what the best sequence BEGINNING WITH each of the nine actions earned, and a
 * soft target over the actions.  The scoring launches report the row's best sequence and its first action only; this says how the other
 * eight first actions fared, whether two of them tie, and by how much the best one wins.  No env handle: a device index and a stream, as
 * pc_cem_refit.  All DEVICE.
 *   ret      float64 [M][K]: pc_env_rollout_sequences[_value][_state]'s output
 *   actions  the table those returns belong to; only its first time row is read: state m, sequence k is the byte at
 *            actions[m * actions_state_stride + k] (stride 0: a shared table); a byte above 8 counts as 8, as it acts
 *   steps    int32, status uint8 [M][K]: the same launch's outputs, both given or both NULL.  A sequence is DEAD AT ONCE iff status is
 *            given, its status is PC_FIRST_TERMINATED and its steps is 1 (it crashes in its first step)
 *   active   uint8 [M] or NULL = every row; NOTHING of a row with 0 is written
 * Outputs, [M][9] each:
 *   count    int32: the number of sequences whose first action is a
 *   q        float64: the return of the first maximum among them, compared as float64 in k ascending order, with that return's bits;
 *            -inf where count is 0
 *   alive    uint8: 1 iff a sequence of a is not dead at once (without status: iff count > 0)
 *   accumulate != 0 merges the row's previous outputs first: q is replaced only by a strictly greater return, count is added, alive
 *   is or-ed (the cross-entropy planner's iterations score the same state: their tables pool).  The first call of a state passes 0.
 *   target   float32 or NULL, from the merged row.  S = the alive actions, qmax = the maximum of q over S.  S empty: nine zeros.
 *            temperature == 0: (float)(1.0 / n) on the n actions of S with q == qmax -- exact ties share the mass --, 0 elsewhere.
 *            temperature > 0: e_a = exp((q_a - qmax) / temperature) in float64 for a in S, summed in ascending a;
 *            target_a = (float)(e_a / sum); 0 outside S.
 *   One wave per state (4 per workgroup), nine running maxima per lane, nine butterflies with ties to the lower k; no atomics, no LDS:
 *   exact for every launch geometry, two calls give the same bits.
 * Checked before any device call, in this order: NULL ret / actions / q / count / alive; exactly one of steps / status NULL; M < 1;
 * K outside 1 .. PC_SEQ_MAX_CANDIDATES; a temperature that is not finite or is negative: PC_ERR_INVALID_ARG; then the device
 * (PC_ERR_NO_DEVICE); M above 2^31 - 1: PC_ERR_UNSUPPORTED.  Does not synchronise. */
int pc_sequences_action_values(int device, const double* ret, const uint8_t* actions, int64_t actions_state_stride,
                               const int32_t* steps, const uint8_t* status, const uint8_t* active, int64_t M, int K, int accumulate,
                               double temperature, double* q, int32_t* count, uint8_t* alive, float* target, void* stream);

/* ---- batched evaluation (opt-in: the entry points above are untouched): the FIRST episode of every env and its lap times, and the
 * deterministic action.  What the reference's log_video answers with one fresh episode (train.py:23-50) and every PPO library with
 * evaluate_policy: N fresh episodes from the start line, one per env.
 * pc_first_episodes: a FORWARD scan over rew, term, trunc [T][N] float32 in pc_episode_stats' two layouts (PC_EPISODE_BUFFER: step t's
 *   flags in row t + 1, step T - 1's in last_term / last_trunc [N]; PC_EPISODE_STEPS: flags[t] belong to rew[t], last_* are not read
 *   and may be NULL).  state [PC_FIRST_ROWS][N] float64 (device, in / out; the caller initialises rows 0-5 to 0 and rows 6-7 to +inf):
 *     row 0  return of the first episode: the float64 sum of the float32 (scaled) rewards -- exact (kernels/gae_sample.hpp: an episode
 *            has at most PC_TIME_LIMIT steps), so the bits are those of a forward sum in any grouping
 *     row 1  length in steps            row 2  gates, row 3  laps (decoded as pc_episode_stats does: k = rint(r / reward_scale))
 *     row 4  status: PC_FIRST_RUNNING, PC_FIRST_TERMINATED or PC_FIRST_TRUNCATED (both flags on the closing step: terminated)
 *     row 5  the episode's step count at its last lap close (0 = no lap yet) = the sum of its lap times
 *     row 6  best lap in steps: the steps between consecutive lap closes, the first lap from the episode's start; +inf = none
 *     row 7  first lap in steps; +inf = none
 *   An env whose status is not RUNNING on entry is left untouched; after the step that closes its episode the rest of the window is
 *   ignored.  Windows chain: one call over T rows and any split of the same rows into consecutive calls leave the same state bits.
 *   Checked before any device call, in pc_episode_stats' order: NULL rew / term / trunc / state, T < 1, N < 1, a layout other than
 *   the two, NULL last_* in the Buffer layout, a reward_scale pc_episode_stats refuses: PC_ERR_INVALID_ARG; then device < 0 or
 *   unknown: PC_ERR_NO_DEVICE.  Never synchronises.
 * pc_greedy: for logits [N][A] float32 (finite), actions[i] = the FIRST index of the maximum of row i (torch.argmax's tie rule);
 *   action_f32 [N] = its float copy, or NULL; logprob [N] = log_softmax(logits[i])[actions[i]] in pc_sample's arithmetic (the bits
 *   pc_sample gives for that action), or NULL.  It sits behind pc_policy_act(..., logits_out) for callers that hold logits; pc_policy_act_greedy / pc_rollout_greedy
 *   (below) take the argmax inside the policy step itself.
 *   NULL logits / actions or N < 1: PC_ERR_INVALID_ARG (checked before any device call); A < 1 or A > 16: PC_ERR_UNSUPPORTED. */
#define PC_FIRST_ROWS 8
#define PC_FIRST_RUNNING 0
#define PC_FIRST_TERMINATED 1
#define PC_FIRST_TRUNCATED 2
int pc_first_episodes(int device, const float* rew, const float* term, const float* trunc, const float* last_term,
                      const float* last_trunc, int64_t T, int64_t N, int layout, double reward_scale, double* state, void* stream);
int pc_greedy(int device, const float* logits, int64_t N, int A, int64_t* actions, float* action_f32, float* logprob, void* stream);

/* ---- track telemetry maps (opt-in: the entry points above are untouched): WHERE on the track the cars drive, how fast, and where
 * they crash.  One streaming pass over observation rows that are already on the device (entries 0-3 of an observation are x / 1280,
 * y / 720, vx / max_speed, vy / max_speed, car_env.py:578-581), reduced to integer counters per cell of cell_px x cell_px pixels.
 * pc_track_maps: obs [T][N][D] float32 -- in both layouts row t is the observation the policy acted on at step t, i.e. the car's pose
 *   BEFORE step t; only entries 0-3 of a row are read.  term / trunc / last_* / layout exactly as pc_first_episodes takes them
 *   (PC_EPISODE_BUFFER: step t's flags in row t + 1, step T - 1's in last_*, row 0 never read; PC_EPISODE_STEPS: flags[t] belong to
 *   step t, last_* may be NULL).  track_id [N] uint8 (device), NULL = every env on track 0.
 *   maps [n_tracks][PC_MAP_PLANES][GH][GW] int64 (device), GW = 1280 / cell_px, GH = 720 / cell_px: ACCUMULATED, the caller zeroes it
 *   once.  cell_px is one of 4, 5, 8, 10, 16, 20, 40, 80 (the divisors of 80 from 4 upward).
 *   first_state: NULL = every sample counts; or pc_first_episodes' [PC_FIRST_ROWS][N] state as it stands BEFORE that window's scan
 *   (read-only, only row 4 is read; call pc_track_maps before pc_first_episodes for each window): a sample then counts only if env
 *   n's status on entry is PC_FIRST_RUNNING and no earlier step of this window had env n's term or trunc flag set -- the closing step
 *   itself counts, everything after it does not: pc_first_episodes' own rule, so the maps cover exactly the first episodes.
 *   Per counted sample (t, n):
 *     cell   cx = clamp((int)floorf(o0 * (float)GW), 0, GW - 1), cy = clamp((int)floorf(o1 * (float)GH), 0, GH - 1), each product ONE
 *            float32 multiply.  A sample whose o0 or o1 is not finite, or whose track_id[n] >= n_tracks, is skipped entirely.
 *     speed  q = (int64)rint(sqrt((double)o2 * o2 + (double)o3 * o3) * PC_MAP_SPEED_UNIT): both products exact in float64, one
 *            rounding in the sum, a correctly rounded sqrt -- a numpy float64 expression gives the same integer.  (A speed that is
 *            not finite, or above 9e18 units, counts as q = 0; the env's own rows have |o2|, |o3| <= 1.)
 *     VISITS += 1, SPEED += q; CRASHES += 1 when step t's term flag is non-zero (a truncation is not a crash).
 *   The crash cell is the cell of the LAST OBSERVATION BEFORE the hit: the pose the failing action was chosen in, not the point of
 *   impact -- the car moves at most max_speed = 10 px per axis in that step, so the impact lies in that cell or next to it.
 *   All accumulation is integer (64-bit adds, no floating-point atomics): the maps are bit-identical whatever the launch geometry
 *   or the order in which samples arrive.
 *   Checked before any device call, in this order: NULL obs / term / trunc / maps, T < 1, N < 1, D < 4, a layout other than the two,
 *   NULL last_* in the Buffer layout, n_tracks < 1 or > 256, a cell_px off the list: PC_ERR_INVALID_ARG; then device < 0 or unknown:
 *   PC_ERR_NO_DEVICE.  Never synchronises. */
#define PC_MAP_VISITS 0      /* samples whose car was in the cell */
#define PC_MAP_SPEED 1       /* sum over those samples of q = speed in units of max_speed / PC_MAP_SPEED_UNIT */
#define PC_MAP_CRASHES 2     /* samples whose step terminated (a wall hit); a truncation is not a crash */
#define PC_MAP_PLANES 3
#define PC_MAP_SPEED_UNIT 1024
int pc_track_maps(int device, const float* obs, int64_t D, const float* term, const float* trunc, const float* last_term,
                  const float* last_trunc, int64_t T, int64_t N, int layout, const uint8_t* track_id, int n_tracks, int cell_px,
                  const double* first_state, int64_t* maps, void* stream);

/* ---- frames on the device (opt-in: the entry points above are untouched): CarEnv.render() in rgb_array mode (car_env.py:762-807)
 * and log_video's frames (train.py:23-50), as a pure function of (observation row, track, next-gate index).  An observation row holds
 * the car's position (entries 0-1), the cos / sin of its heading (4-5) and every ray's length (6 ..), so M rows that are already on the
 * device -- a rollout or evaluation buffer -- become M RGB frames without an env, a re-simulation or a host round trip.  The look is
 * this project's (no sprite, no anti-aliasing); the rule is exact integer arithmetic, so every pixel is defined (DESIGN.md 4.11;
 * tests/render_reference.py is its numpy form):
 *   grid       quarter pixels (q), int32.  W = 1280 / scale, H = 720 / scale, scale one of 1, 2, 4, 5, 8, 10; the centre of pixel (i, j)
 *              is P = (4 scale i + 2 scale, 4 scale j + 2 scale).  Q(v) = (int32)rint(v * 4.0) on a float64 v.
 *   static     walls and gates: pc_track_geometry's float64 pixel coordinates, each through Q.
 *   per row o  x = (double)o[0] * 1280.0, y = (double)o[1] * 720.0, c = (double)o[4], s = (double)o[5].  Ray i of R = pc_ray_count(n):
 *              (ci, si) = the HOST's float64 cos / sin of radians(i * (360 / n)) (a table made at pc_env_create; the device's own
 *              cos / sin is never used), dx = c ci - s si, dy = s ci + c si, d = 1000.0 * (double)o[6 + i] clamped to [0, 1000] (a
 *              non-finite entry: 0); the ray runs from (Q(x), Q(y)) to (Q(x + d dx), Q(y + d dy)).  The car is the capsule from
 *              (Q(x - 8.0 c), Q(y - 8.0 s)) to (Q(x + 14.0 c), Q(y + 14.0 s)).
 *   coverage   a segment (A, B) of half-width h covers P, with u = (P - A).(B - A) and L = |B - A|^2: L == 0 or u <= 0: |P - A|^2 <= h^2;
 *              u >= L: |P - B|^2 <= h^2; else cross(P - A, B - A)^2 <= h^2 L.  A disc is a segment with A == B.  Half-widths in q:
 *              max(nominal, 3 scale) with nominal 10 (wall), 10 (gate), 2 (ray), 24 (car); a hit disc has radius 20, not widened.
 *   road       P is road iff an odd number of its track's walls have (A.y > P.y) != (B.y > P.y) and cross P's row strictly to its right:
 *              cross(P - A, B - A) < 0 where B.y > A.y, > 0 where B.y < A.y.
 *   layers     later wins: grass, road, walls, plain gates (in index order), the highlighted gate, rays, one hit disc at every ray's
 *              end, the car.  With next_gate: gate g is drawn iff g >= next_gate[m] (the reference hides the gates passed in this lap,
 *              car_env.py:725-741, 788-793) and gate next_gate[m], if the track has it, in PC_RENDER_NEXT_GATE.  NULL: all gates plain.
 *   guards     a row draws the static layers only, every gate plain, if o[0], o[1], o[4] or o[5] is not finite, |o[4]| or |o[5]| > 1,
 *              the car lies outside [-1024, 2304] x [-1024, 1744] px, or its track_id is not a track of the handle (track 0 is shown).
 * pc_render_background: the static layers of every track of the handle at `scale`, once per (handle, scale):
 *   background [n_tracks][2][H][W] uint8 (device, 4-byte aligned): plane 0 = PC_RENDER_GRASS / _ROAD / _WALL, plane 1 = 1 + the highest
 *              gate index that covers the pixel, 0 = none.
 * pc_render_frames: M rows -> frames [M][H][W][3] uint8 (device, 4-byte aligned; r, g, b).
 *   obs        row m at obs + m * obs_ld, obs_ld >= D: one env's rows of a [T][N][D] buffer are obs_ld = N * D
 *   next_gate  [M] int32 (device) or NULL;  track_id [M] uint8 (device) or NULL = track 0
 *   background what pc_render_background wrote for the same handle and scale
 *   palette    HOST [PC_RENDER_COLORS][3] uint8 (r, g, b per PC_RENDER_* index) or NULL = the default; copied into the launch's arguments
 *   M is independent of the handle's env count.  Neither call reads or writes env state; neither synchronises.
 * Checked before any device call, in this order: NULL handle / background (pc_render_frames: / obs / frames, M < 1, obs_ld < D), a
 * scale off the list, a background or frames pointer that is not 4-byte aligned: PC_ERR_INVALID_ARG; then a handle one of whose tracks
 * has a wall or gate coordinate outside [-1024, 2304] x [-1024, 1744] px (or not finite), or more than 255 gates: PC_ERR_UNSUPPORTED
 * with the reason in pc_last_hip_error. */
#define PC_RENDER_GRASS 0
#define PC_RENDER_ROAD 1
#define PC_RENDER_WALL 2
#define PC_RENDER_GATE 3
#define PC_RENDER_NEXT_GATE 4
#define PC_RENDER_RAY 5
#define PC_RENDER_HIT 6
#define PC_RENDER_CAR 7
#define PC_RENDER_COLORS 8
int pc_render_background(const pc_env* e, int scale, uint8_t* background, void* stream);
int pc_render_frames(const pc_env* e, const float* obs, int64_t obs_ld, const int32_t* next_gate, const uint8_t* track_id,
                     int64_t M, int scale, const uint8_t* background, const uint8_t* palette, uint8_t* frames, void* stream);

/* ---- the whole of Agent.get_action_and_value(x) as the rollout calls it (model.py:34-41, train.py:181):
 * both 1-hidden-layer MLPs (actor D->H->A, critic D->H->1, ReLU), the categorical draw, log_prob and the
 * value, in one launch on the matrix cores.  A policy step's configuration is a HANDLE: shape (D, H, A), arithmetic form of the
 * two GEMMs and work decomposition.  Handles are immutable and independent: two of them with different forms can pack and run
 * side by side in one process; a weight image belongs to the handle that packed it.
 *   precision  2 (= -1, the default) fp16x2 in scaled domains: every fp32 operand v = h + l, h = fp16(v), l = fp16(v - h); a product
 *                is a_h b_l + a_l b_h + a_h b_h into ONE fp32 accumulator (v_mfma_f32_16x16x32_f16, three per K block); max error
 *                vs float64 on this MLP 1.1e-7 (a plain fp32 GEMM: 0.8e-7); operands saturate at fp16's finite range in their
 *                scaled domain.  Needs D <= 40, A <= 9, else the shape gets form 0.
 *              1 bf16x3: three bf16 pieces per operand, six piece products (v_mfma_f32_16x16x32_bf16); 1.0e-7; same shapes.
 *              0 fp32-input MFMA (v_mfma_f32_16x16x4_f32), bit-for-bit an fp32 fmaf chain.
 *   split      -1 automatic (hidden tiles split across the waves of a workgroup up to 8192 envs), 0 never, 1 always; the two
 *              forms differ in fp32 summation order (last-bit differences).
 * pc_policy_create: PC_ERR_UNSUPPORTED unless H == 256, A <= 15, D <= 40 (the caller then uses its own GEMMs + pc_sample).
 * pc_policy_get reports the form the shape actually got and the number of floats its weight image needs.
 * The weights do not change during a rollout, so they are packed ONCE into the kernel's LDS image:
 *   pc_policy_pack  builds the image (device buffer `image`) from the eight torch.nn.Linear tensors: aW1 [H][D], ab1 [H],
 *                   aW2 [A][H], ab2 [A], cW1 [H][D], cb1 [H], cW2 [1][H], cb2 [1]
 *   pc_policy_pack_checked  the same, and *range_status (a DEVICE int32, written asynchronously on `stream`) := 0 or a mask of
 *                   PC_POLICY_RANGE_*: the weights leave precision 2's numeric domain -- a weight saturates in its scaled fp16 domain
 *                   (|W1| > 4094, |W2| > 1023.5), or a hidden unit can reach the hidden layer's saturation point 255.87 on observations
 *                   within +-4 (|b1| + 4 sum_j |W1_uj| > 255.87; CarEnv's observations lie in [-1, 1.6]).  With the status 0 NO operand of
 *                   the policy pass can saturate, so the rollout kernels carry no run-time check.  A set bit means: results of
 *                   pc_policy_act / pc_rollout with this image are NOT model.py's within 4e-6 -- pack with a precision-0 handle instead
 *                   (the host layer does: Agent.pack_policy).  Forms 0 and 1 have no scaled domains: always 0.
 *   pc_policy_act   one policy step for obs [N][D] using the image.  RNG as pc_sample, with offset = `offset` + *offset_dev when
 *                   offset_dev != NULL (a device counter, so a captured HIP graph can be replayed with a fresh stream of draws).
 *                   action [N] int64; action_f32 [N] (the float copy Buffer.act_buf stores, buffer.py:13) or NULL; logprob,
 *                   value [N]; logits_out [N][A] or NULL. */
int pc_policy_create(int device, int D, int H, int A, int precision, int split, pc_policy** out);
void pc_policy_destroy(pc_policy* p);
int pc_policy_get(const pc_policy* p, int* precision, int* split, int64_t* image_floats);
int pc_policy_pack(const pc_policy* p, const float* aW1, const float* ab1, const float* aW2, const float* ab2, const float* cW1,
                   const float* cb1, const float* cW2, const float* cb2, float* image, void* stream);
#define PC_POLICY_RANGE_W1 1       /* a first-layer weight (actor or critic) saturates in its scaled fp16 domain */
#define PC_POLICY_RANGE_W2 2       /* an actor output-layer weight does */
#define PC_POLICY_RANGE_HIDDEN 4   /* a hidden activation can */
int pc_policy_pack_checked(const pc_policy* p, const float* aW1, const float* ab1, const float* aW2, const float* ab2, const float* cW1,
                           const float* cb1, const float* cW2, const float* cb2, float* image, int32_t* range_status, void* stream);
int pc_policy_act(const pc_policy* p, const float* obs, int64_t N, const float* image, uint64_t seed, uint64_t offset,
                  const uint64_t* offset_dev, int64_t* action, float* action_f32, float* logprob, float* value, float* logits_out,
                  void* stream);
/* pc_policy_act's GREEDY form: the same policy step with action [i] = the FIRST index of the maximum logit of row i (float equality: -0.0
 * and +0.0 tie and the lower index wins -- torch.argmax's rule and pc_greedy's; logits are finite by contract) in place of the draw.  No seed,
 * offset or offset_dev: no random number is generated.  logits_out and value carry pc_policy_act's bits on the same inputs; logprob [i] =
 * logit[action] - logsumexp in the kernel's own arithmetic, i.e. the bits pc_policy_act writes wherever it draws that action.  Every form a
 * policy handle can have (precision 0 / 1 / 2, split or not, A = 1 .. 15).  Argument checks, their order and the status codes: pc_policy_act's. */
int pc_policy_act_greedy(const pc_policy* p, const float* obs, int64_t N, const float* image, int64_t* action, float* action_f32,
                         float* logprob, float* value, float* logits_out, void* stream);

/* ---- the whole rollout of one epoch (train.py:173-195) as ONE persistent launch: for t in 0..T-1
 *   (action, logprob, value) = Agent.get_action_and_value(obs_t)      [pc_policy_act's arithmetic and RNG, offset + t]
 *   obs_{t+1}, reward, terminated, truncated = envs.step(action)      [pc_env_step's arithmetic]
 *   Buffer.store(...)                                                 [rows written in place]
 * Inputs: the env handle (single track, or mixed tracks with every aligned block of 32 envs on one track -- when the
 * blocks are as large as the launch's workgroups, 128 / 256 envs in the large form and 16 / 32 in the small one, each
 * workgroup stages its track's tables in LDS as for a single track, else every wave reads them from global memory), the
 * policy handle and the weight image it packed, and next_obs / next_term / next_trunc [N] = observation and flags the rollout
 * starts from (the caller has copied them into row 0 of obs_buf / term_buf / trunc_buf, as Trainer does).
 * Outputs: obs_buf [T][N][D] rows 1..T-1, act_buf (float32, buffer.py:13), rew_buf, val_buf, logprob_buf [T][N] rows 0..T-1,
 * term_buf / trunc_buf rows 1..T-1, and next_obs / next_term / next_trunc overwritten with the state after step T-1 -- bit-identical
 * to T x (pc_policy_act; pc_env_step) -- plus two per-env outputs [N] float32 (each may be NULL) so that an epoch needs nothing
 * else between the rollout and Buffer.calculate_advantages:
 *   last_value : the critic's value of the FINAL observation -- agent.get_value(next_obs), train.py:200 -- from one more policy
 *                pass inside the launch (the fused policy step's arithmetic, i.e. what val_buf's rows hold for the other steps);
 *   reward_sum : the sum over the T steps of the env's (scaled) rewards, accumulated in float32 in step order -- the numerator
 *                of train.py:272's average reward without re-reading rew_buf.
 * F64 handles (PC_DTYPE_F64) take the same call: the launch then steps the env in the reference's own float64 (the per-step
 * kernel's env_step arithmetic, bit for bit: observations, rewards, events and the float64 state equal the reference's) -- Discrete(9),
 * the split-operand policy forms, 12, 16 or 32 nominal rays; other shapes are PC_ERR_UNSUPPORTED (the caller's per-step kernels run them).
 * Two kernels fill the same bits (pc_env_last_rollout_kernel says which ran): by default the selector form -- K9 with a float32
 * sweep that only SELECTS each ray's wall and the reference's literal arithmetic on that wall (fp16 x 2 policy arithmetic, tracks of
 * at most 8192 chain vertices inside 2000 px, every env's rotation one that reset and stepping produce; up to 8192 envs at 12 / 16 rays
 * inside the small form, whose policy arithmetic is the split policy step's) --, else the filter form,
 * which tests every (ray, wall) pair in float64 (any track, any state, bf16 x 3 at 12 rays; not built for 32 rays); tracks of more
 * than 64 chain vertices and rotations set off the table take the generic kernel with the selector step (PC_KERNEL_K9D_SELECTOR).
 * With a precision-0 policy handle an F64 handle at 16 rays runs the literal form with the fp32 weight image: every number of the
 * rollout in the reference's own arithmetic, still one launch.
 * Mixed-track handles: track ids constant inside aligned blocks of 32 envs (or more: whole workgroups) run the fast modes per block;
 * track ids that change INSIDE a block (car_env.py:621-628 puts every env on its own track: e.g. track_id = i & 1) run the big form with
 * the env step once per track present in a wave -- two tracks of the reference's layout (two equal loops of 13 or 9 chain vertices) at
 * 16 rays in the table-driven two-track form (both tracks' tables in LDS; F32 and F64 handles), anything else in the generic mode.
 * When every aligned block of 64 envs (32 in the 16-envs-per-wave form) is split evenly between the two tracks -- i & 1 is -- the
 * block's two waves DE-INTERLEAVE it: each wave steps the block's envs of ONE track (one pass; an env's rows, state and random stream stay
 * the env's own, so the buffers are the same bits).
 * PC_ERR_UNSUPPORTED for ray
 * counts whose slots per lane are not on the kernel menu (12 / 16 / 32 run the table-driven fast mode; 17 and 18 share the
 * slots of 16 and run the generic mode), shapes whose LDS footprint exceeds 160 KB (33 rays with the fp32 or bf16x3 weight
 * image in the large form), and 33 rays in the GENERIC mode with split operands (a mixed-track batch whose workgroups
 * straddle tracks, or the fast mode switched off: those kernels spilled and are not built): callers fall back to the
 * two-kernel loop, which fills the same buffers bit for bit. */
int pc_rollout(pc_env* e, const pc_policy* p, const float* image, int64_t T, double reward_scale, uint64_t seed, uint64_t offset,
               const uint64_t* offset_dev, float* obs_buf, float* act_buf, float* rew_buf, float* val_buf, float* term_buf,
               float* trunc_buf, float* logprob_buf, float* next_obs, float* next_term, float* next_trunc, float* last_value,
               float* reward_sum, void* stream);
/* pc_rollout that also keeps the observation every time-limit truncation replaced (gymnasium's info["final_observation"]; the
 * rollout buffer holds only the reset observation there): final_obs [slots][N][D] float32 (device), the truncation of env n at
 * rollout step t in row [t / PC_TIME_LIMIT][n] (see pc_gae_bootstrap for why the slots never collide).  Only those rows are written;
 * every other entry keeps what it held (the caller zeroes the buffer once, so a value pass never sees garbage).  Every other output
 * is pc_rollout's, bit for bit: pc_rollout is this call with final_obs = NULL.  PC_ERR_INVALID_ARG: final_obs NULL or
 * slots < ceil(T / PC_TIME_LIMIT). */
int pc_rollout_final_obs(pc_env* e, const pc_policy* p, const float* image, int64_t T, double reward_scale, uint64_t seed,
                         uint64_t offset, const uint64_t* offset_dev, float* obs_buf, float* act_buf, float* rew_buf, float* val_buf,
                         float* term_buf, float* trunc_buf, float* logprob_buf, float* next_obs, float* next_term, float* next_trunc,
                         float* last_value, float* reward_sum, float* final_obs, int64_t slots, void* stream);
/* The GREEDY rollout (what evaluate_policy(deterministic=True) steps): T x (pc_policy_act_greedy; pc_env_step) as one persistent launch, bit for
 * bit, in every buffer pc_rollout fills.  final_obs == NULL: pc_rollout's outputs (`slots` is ignored); else pc_rollout_final_obs's, with its
 * `slots` check.  The other argument checks are pc_rollout's.  The launch is the greedy instance of the kernel pc_rollout picks for the same
 * handle and options -- same PC_KERNEL_* id, envs per workgroup, grid, LDS bytes and 1/den-table choice -- where that kernel is on the greedy
 * menu: F32 handles, fp16 x 2 policy arithmetic (precision 2), Discrete(9), 12 / 16 / 32 nominal rays, the table-driven modes (small form, big
 * form, 16-envs-per-wave form).  Everything else -- F64 handles, precision 0 and 1, the generic mode (PC_OPT_ROLLOUT_FAST = 0, ray counts or
 * tracks off the fast menu), tracks interleaved inside a block of 32 envs, A != 9 -- is PC_ERR_UNSUPPORTED before any device call, with
 * pc_env_last_rollout_kernel unchanged: callers then run the two per-step kernels, as for pc_rollout's refusals. */
int pc_rollout_greedy(pc_env* e, const pc_policy* p, const float* image, int64_t T, double reward_scale,
                      float* obs_buf, float* act_buf, float* rew_buf, float* val_buf, float* term_buf,
                      float* trunc_buf, float* logprob_buf, float* next_obs, float* next_term,
                      float* next_trunc, float* last_value, float* reward_sum,
                      float* final_obs, int64_t slots, void* stream);

/* ---- the non-GEMM work of one PPO minibatch step (train.py:230-261), three launches:
 * pc_ppo_gather : traj_*[batch_indices] (train.py:233-238,249): idx [B] int64 into the flattened trajectories
 *                 obs [M][D], act / logprob / adv / ret [M]  ->  o_obs [B][D], o_act / o_logprob / o_adv / o_ret [B].
 * pc_ppo_loss   : the clipped-PPO loss (train.py:235-255: ratio, per-minibatch advantage normalisation with the
 *                 unbiased std, max(-A r, -A clamp(r)), 0.5 (v - ret)^2, entropy) given the network outputs
 *                 logits [B][A], values [B]; writes its gradients dlogits [B][A], dvalues [B] (what autograd would
 *                 hand to the two MLPs) and adds (policy_loss, value_loss, entropy, total) to metrics[4]
 *                 (train.py:263-266).  2 <= B <= 1024.
 * pc_clip_adam  : nn.utils.clip_grad_norm_(max_norm) (train.py:260) + Adam.step() (train.py:261; eps/betas as
 *                 train.py:146 configures) over flat float32 buffers of n elements; lr and the step counter live on
 *                 the device (HIP-graph replay); grad_scale = 1/world_size folds the gradient average in. */
int pc_ppo_gather(int device, const int64_t* idx, int B, int D, const float* obs, const float* act, const float* logprob,
                  const float* adv, const float* ret, float* o_obs, float* o_act, float* o_logprob, float* o_adv, float* o_ret,
                  void* stream);
int pc_ppo_loss(int device, const float* logits, const float* values, const float* act, const float* old_logprob,
                const float* adv, const float* ret, int B, int A, double clip_ratio, double vf_coef, double ent_coef,
                float* dlogits, float* dvalues, float* metrics, void* stream);
int pc_clip_adam(int device, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* step_count, const float* lr_dev,
                 int64_t n, double max_norm, double grad_scale, double beta1, double beta2, double eps, void* stream);
/* The same step for the multi-rank form of pc_ppo_minibatch (apply = 2: the gradient kernels have already advanced the step
 * counter): n / 256 workgroups, each summing the bucket's squares itself in one fixed order (replicas stay bit-identical).
 * `grad` = the all-reduced SUM over ranks, left untouched; grad_scale = 1 / world_size.  (train.py:260-261) */
int pc_clip_adam_advanced(int device, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* step_count,
                          const float* lr_dev, int64_t n, double max_norm, double grad_scale, double beta1, double beta2, double eps,
                          void* stream);

/* ---- one whole PPO minibatch step (train.py:230-261) with no library GEMM: gather, both MLPs forward, the clipped-PPO
 * loss, both MLPs backward, and (apply != 0) clip_grad_norm_ + Adam, as three launches.  `param` / `grad` / `exp_avg` /
 * `exp_avg_sq` are flat float32 buffers in torch's module.parameters() order (actor.0.weight [H][D], actor.0.bias,
 * actor.2.weight [A][H], actor.2.bias, critic.0.weight, critic.0.bias, critic.2.weight [1][H], critic.2.bias); idx [B]
 * indexes the flattened trajectories obs [M][D], act / old_logprob / adv / ret [M].  grad receives the (clipped, when
 * applied) gradient; metrics[4] += (policy_loss, value_loss, entropy, total); step_count [1] float and lr_dev [1] live on
 * the device.  apply == 0 stops after the gradient; apply == 2 stops after the gradient but advances the step counter
 * (multi-rank: all-reduce the gradient, then pc_clip_adam_advanced).  workspace: device
 * buffer of pc_ppo_workspace_floats(B, D, H, A) floats.  Deterministic (fixed summation order, no atomics).
 * Alignment: `param` and `workspace` must be 16-byte aligned (the forward / backward launch loads the first-layer weights and
 * stores the gradient partials as 16-byte vectors): PC_ERR_INVALID_ARG otherwise, checked with the NULL checks before any device
 * call.  No other argument needs more than its element's alignment: idx, obs / act / old_logprob / adv / ret, grad, exp_avg,
 * exp_avg_sq, step_count, lr_dev and metrics are read and written element by element.
 * PC_ERR_UNSUPPORTED unless H == 256, A <= 15, D <= 40, 2 <= B <= 1024. */
int64_t pc_ppo_workspace_floats(int B, int D, int H, int A);
int pc_ppo_minibatch(int device, const int64_t* idx, int B, int D, int H, int A, const float* obs, const float* act,
                     const float* old_logprob, const float* adv, const float* ret, float* param, float* grad, float* exp_avg,
                     float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef, double ent_coef,
                     double max_norm, double beta1, double beta2, double eps, float* metrics, float* workspace, int apply,
                     void* stream);

/* ---- one supervised minibatch step on the same flat buckets (behaviour cloning of a teacher's actions; K27, then the reduction
 * and clip + Adam launches of pc_ppo_minibatch unchanged): gather, both MLPs forward, the loss below, both MLPs backward, and
 * (apply == 1) clip_grad_norm_ + Adam.  No library GEMM, no atomics, a fixed summation order: two calls give the same bits.
 *   obs [M][D]; label [M] float32 (act_buf's layout: a rollout buffer's actions can serve); target [M] float32, the critic's
 *   regression targets, or NULL; idx [B] int64 into them, duplicates allowed.
 *   With labelled_i = (0 <= label_i < A):
 *     ce_i  = labelled_i ? -log_softmax(logits_i)[label_i] : 0      ent_i = labelled_i ? entropy(softmax(logits_i)) : 0
 *     vl_i  = 0.5 (v_i - target_i)^2
 *     loss  = (sum_i ce_i + vf_coef * sum_i vl_i - ent_coef * sum_i ent_i) / B
 *   The divisor is always B.  A label outside 0 .. A-1 means "no label" (the planners' doomed states carry -1): the actor's
 *   gradient of that sample is exactly zero and it adds nothing to the ce and ent sums; its value term still counts.
 *   target == NULL needs vf_coef == 0 (PC_ERR_INVALID_ARG otherwise): the critic's gradient is +0.0f in every element, metrics[1]
 *   gets +0, and a clip + Adam step from zero moments leaves the critic's parameters bit-identical.
 * metrics[4] += (mean ce, mean vl, mean ent, total); grad receives the (clipped, when applied) gradient; apply 0 / 1 / 2,
 * step_count, lr_dev, the workspace (pc_ppo_workspace_floats(B, D, H, A) floats), the alignment (`param` and `workspace` 16-byte
 * aligned: PC_ERR_INVALID_ARG; nothing else), the limits (H == 256, A <= 15, D <= 40, 2 <= B <= 1024: PC_ERR_UNSUPPORTED) and the
 * order of the checks (those that need no device first) are pc_ppo_minibatch's. */
int pc_bc_minibatch(int device, const int64_t* idx, int B, int D, int H, int A, const float* obs, const float* label,
                    const float* target, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* step_count,
                    const float* lr_dev, double vf_coef, double ent_coef, double max_norm, double beta1, double beta2, double eps,
                    float* metrics, float* workspace, int apply, void* stream);

/* pc_bc_minibatch against SOFT targets: soft [M][A] float32 row-major (pc_sequences_action_values' target can serve) in label's place,
 * everything else as above.  With p = row i of soft, w_i = sum_k p_ik (float32, the 16-lane row's reduction tree) and
 * labelled_i = (w_i > 0) -- an all-zero row, or one that holds a NaN, is "no label":
 *     ce_i  = labelled_i ? -sum_k p_ik log_softmax(logits_i)[k] : 0      ent_i, vl_i and the loss as above
 *     d loss / d logit_k = labelled_i ? -(p_ik - w_i softmax_k) / B + the entropy term : +0
 * A one-hot row gives pc_bc_minibatch's bits for that label.  The third compile-time head of the shared forward / backward body; the
 * compiled and the generic shapes; no deferred, prepared, diagnostics or large form. */
int pc_bc_minibatch_soft(int device, const int64_t* idx, int B, int D, int H, int A, const float* obs, const float* soft,
                         const float* target, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* step_count,
                         const float* lr_dev, double vf_coef, double ent_coef, double max_norm, double beta1, double beta2, double eps,
                         float* metrics, float* workspace, int apply, void* stream);

/* The same step on a minibatch gathered beforehand. pc_ppo_prepare gathers n_mb minibatches in ONE launch: minibatch m
 * reads its B indices at idx[m * idx_ld ...] and writes, at prepared + m * pc_ppo_prepared_floats(B, D), the sample rows
 * obs[idx] [B][D], then act / old_logprob / adv / ret [B] each, then (mean, max(unbiased std, 1e-5)) of its advantages and
 * two pad floats -- what every workgroup of pc_ppo_minibatch otherwise fetches (an index load, then the dependent row
 * loads: two cold misses at the head of its critical path) and reduces for itself.  pc_ppo_minibatch_prepared(one such
 * block) == pc_ppo_minibatch on the same samples, bit for bit.  (train.py:225-240) */
int64_t pc_ppo_prepared_floats(int B, int D);
int pc_ppo_prepare(int device, const int64_t* idx, int64_t idx_ld, int n_mb, int B, int D, const float* obs, const float* act,
                   const float* old_logprob, const float* adv, const float* ret, float* prepared, void* stream);
int pc_ppo_minibatch_prepared(int device, const float* prepared_mb, int B, int D, int H, int A, float* param, float* grad, float* exp_avg,
                              float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef,
                              double ent_coef, double max_norm, double beta1, double beta2, double eps, float* metrics,
                              float* workspace, int apply, void* stream);


/* ---- update diagnostics and the target-KL early stop (opt-in: the entry points above are untouched).  Per minibatch of B samples,
 * from the very logratio_i = new_logprob_i - old_logprob_i and ratio_i = exp(logratio_i) the clipped loss is made of (CleanRL's
 * ppo.py):
 *   approx_kl = mean_i((ratio_i - 1) - logratio_i)          clipfrac = mean_i(|ratio_i - 1| > clip_ratio)
 * and per epoch, over the whole rollout, explained_variance = 1 - Var(ret - val) / Var(ret) (population variances; NaN when
 * Var(ret) == 0).  The *_diag forms of the minibatch step keep a device block diag[PC_DIAG_FLOATS]:
 *   [0] sum of approx_kl over the steps evaluated   [1] sum of clipfrac over them   [2] steps evaluated   [3] steps applied
 *   [4] stop flag (0 / 1)                           [5] approx_kl of the last step evaluated               [6..7] pad
 * The stop (Stable-Baselines3's target_kl): a step whose approx_kl > 1.5 * target_kl is evaluated but NOT applied -- grad, param,
 * the moments, the step counter and metrics stay as they are -- and raises the flag; every later *_diag launch sees the flag and
 * writes nothing, until the caller zeroes the block (hipMemsetAsync on the same stream, at the head of every epoch).  The flag
 * is device memory read and written by the launches of one stream: no host round trip, so a captured graph of a whole epoch is
 * replayed unchanged.  target_kl <= 0 or NaN: never stop (diagnostics only).  Without a stop, param / grad / exp_avg / exp_avg_sq /
 * step_count / metrics get the bits of the plain entry points.
 * pc_ppo_minibatch_diag / _prepared_diag: workspace of pc_ppo_diag_workspace_floats(B, D, H, A) floats (the plain layout plus a
 * second per-workgroup partial); apply == 2 (the multi-rank form: the ranks would have to agree on the stop) is
 * PC_ERR_UNSUPPORTED.  pc_ppo_loss_diag books the step as above (a stopping step still writes dlogits / dvalues);
 * pc_clip_adam_diag is pc_clip_adam that returns at once when diag[4] != 0.  diag == NULL: PC_ERR_INVALID_ARG.
 * pc_explained_variance: val / ret [M] float32, float64 accumulation about a shift with pairwise (Chan) merges, not
 * E[x^2] - E[x]^2; two launches in a fixed order (deterministic); workspace: pc_explained_variance_workspace_doubles(device)
 * doubles; out[5] = (mean(ret), M2(ret), mean(ret - val), M2(ret - val), explained_variance), M2 = the sum of squared deviations
 * = M * Var.  NULL arrays or M < 1: PC_ERR_INVALID_ARG, checked before any device call. */
#define PC_DIAG_FLOATS 8
int64_t pc_ppo_diag_workspace_floats(int B, int D, int H, int A);
int pc_ppo_minibatch_diag(int device, const int64_t* idx, int B, int D, int H, int A, const float* obs, const float* act,
                          const float* old_logprob, const float* adv, const float* ret, float* param, float* grad, float* exp_avg,
                          float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef, double ent_coef,
                          double max_norm, double beta1, double beta2, double eps, float* metrics, float* workspace, int apply,
                          float* diag, double target_kl, void* stream);
int pc_ppo_minibatch_prepared_diag(int device, const float* prepared_mb, int B, int D, int H, int A, float* param, float* grad, float* exp_avg,
                                   float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef,
                                   double ent_coef, double max_norm, double beta1, double beta2, double eps, float* metrics,
                                   float* workspace, int apply, float* diag, double target_kl, void* stream);
int pc_ppo_loss_diag(int device, const float* logits, const float* values, const float* act, const float* old_logprob,
                     const float* adv, const float* ret, int B, int A, double clip_ratio, double vf_coef, double ent_coef,
                     float* dlogits, float* dvalues, float* metrics, float* diag, double target_kl, void* stream);
int pc_clip_adam_diag(int device, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* step_count, const float* lr_dev,
                      int64_t n, double max_norm, double grad_scale, double beta1, double beta2, double eps, const float* diag,
                      void* stream);
int64_t pc_explained_variance_workspace_doubles(int device);
int pc_explained_variance(int device, const float* val, const float* ret, int64_t M, double* workspace, double* out, void* stream);

/* ---- the same minibatch step for LARGE minibatches, 1024 < B <= PC_PPO_LARGE_MAX_B (opt-in: the entry points above are untouched
 * and keep their limit).  No library GEMM, no atomics, float32 arithmetic throughout (the advantage statistics accumulate in
 * float64 and are rounded once), every index -> row address in 64 bits.
 * pc_ppo_adv_stats: for each of n_mb minibatches (minibatch m reads its B indices at idx[m * idx_ld ...]) the pair
 *   stats[m][0..1] = (mean, max(unbiased std, 1e-5)) of adv[idx] (train.py:238-240): float64 sums about a shift taken from the
 *   data, several workgroups per minibatch and a merge in a fixed order, two launches.  It depends on idx and adv only, so one call at
 *   the head of an epoch covers every minibatch of it.  workspace: pc_ppo_adv_stats_workspace_doubles(n_mb, B) doubles.
 *   NULL arrays, n_mb < 1 or > 65535, idx_ld < B: PC_ERR_INVALID_ARG, checked before any device call.
 * pc_ppo_minibatch_large: pc_ppo_minibatch's arguments, contract (apply 0 / 1 / 2, metrics, step_count, lr_dev), status codes and
 *   order of checks, plus adv_stats = this minibatch's pair from pc_ppo_adv_stats (device memory).  The forward / backward launch
 *   is a FIXED grid of pc_ppo_large_parts(device, B) = min(ceil(B / 8), compute units of the device) workgroups: workgroup g loads the
 *   parameters once and walks the groups of 8 samples g, g + G, g + 2 G, ... with its gradient accumulators in registers, then
 *   writes one partial; the partials are summed in index order by the gradient-reduction launch of pc_ppo_minibatch, and the clip +
 *   Adam launch is the same one.  The summation order is fixed for a given (device, B): two calls give the same bits; it is NOT the
 *   order of pc_ppo_minibatch, and it differs between devices with different compute-unit counts.
 *   workspace: pc_ppo_large_workspace_floats(device, B, D, H, A) floats, laid out as pc_ppo_minibatch's with `parts` partials:
 *   [parts][n_pad] gradient partials (n_pad = the parameter count rounded up to 4), [parts][4] metric partials, then the
 *   per-block squared-norm partials.  Nothing is read that the step has not written: the buffer needs no initialisation.
 *   Alignment: as pc_ppo_minibatch, `param` and `workspace` must be 16-byte aligned (PC_ERR_INVALID_ARG, with the NULL checks);
 *   idx, the five sample arrays, adv_stats, grad, the moments, step_count, lr_dev and metrics need their element's alignment only.
 *   Never synchronises; every launch goes to `stream`.
 * PC_ERR_UNSUPPORTED unless H == 256, 1 <= A <= 15, 1 <= D <= 40, 1024 < B <= PC_PPO_LARGE_MAX_B; PC_ERR_NO_DEVICE for device < 0
 * or a device the runtime does not know (the grid depends on the device). */
#define PC_PPO_LARGE_MAX_B (1 << 20)
int64_t pc_ppo_large_workspace_floats(int device, int B, int D, int H, int A);
int pc_ppo_large_parts(int device, int B);
int64_t pc_ppo_adv_stats_workspace_doubles(int n_mb, int B);
int pc_ppo_adv_stats(int device, const int64_t* idx, int64_t idx_ld, int n_mb, int B, const float* adv, float* stats, double* workspace,
                     void* stream);
int pc_ppo_minibatch_large(int device, const int64_t* idx, int B, int D, int H, int A, const float* obs, const float* act,
                           const float* old_logprob, const float* adv, const float* ret, const float* adv_stats, float* param, float* grad,
                           float* exp_avg, float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef,
                           double ent_coef, double max_norm, double beta1, double beta2, double eps, float* metrics, float* workspace,
                           int apply, void* stream);

/* The whole minibatch loop of one epoch (train.py:223-261) over n_mb prepared minibatches (consecutive blocks of
 * pc_ppo_prepared_floats(B, D) floats at `prepared`), with the clip + Adam step of minibatch i taken by the forward / backward
 * launch of minibatch i + 1 as it loads the parameters (every workgroup needs all of them anyway; workgroup 0 writes the new
 * generation into the other of two state buffers): TWO launches per minibatch instead of three, plus one clip + Adam launch for
 * the last gradient, which also brings the state home.  Bit-identical to n_mb x pc_ppo_minibatch_prepared(apply = 1): param,
 * exp_avg, exp_avg_sq, step_count and metrics; `grad` ends as the LAST minibatch's clipped gradient.  state2: device scratch of
 * pc_ppo_epoch_state_floats(D, H, A) floats; param / grad / exp_avg / exp_avg_sq / state2 16-byte aligned.  Single-rank only
 * (the multi-rank step has the gradient exchange between the backward pass and the clip). */
int64_t pc_ppo_epoch_state_floats(int D, int H, int A);
int pc_ppo_epoch_prepared(int device, const float* prepared, int n_mb, int B, int D, int H, int A, float* param, float* grad, float* exp_avg,
                          float* exp_avg_sq, float* step_count, const float* lr_dev, double clip_ratio, double vf_coef, double ent_coef,
                          double max_norm, double beta1, double beta2, double eps, float* metrics, float* workspace, float* state2,
                          void* stream);

/* ---- the per-minibatch gradient exchange (one all-reduce(SUM) of the flat gradient bucket between
 * loss.backward() and clip_grad_norm_, train.py:259-260) as a ONE-SHOT all-reduce over peer-mapped buffers -- the
 * latency-proof alternative to an RCCL all_reduce for a 49 - 92 KB message: every rank writes its bucket straight into a
 * slot of every peer's staging buffer (hipIpc-mapped device memory: W - 1 independent xGMI writes), raises an arrival flag,
 * waits for its own W flags and sums the W slots locally in rank order, so the reduced buckets are bit-identical on all
 * ranks.  One process per rank (ranks of one node; up to 8):
 *   pc_xchg_create(device, rank, world, n_floats)   allocates this rank's staging buffer (uncached device memory);
 *   pc_xchg_local_handle(x, out)                    PC_XCHG_HANDLE_BYTES bytes for the other ranks: the hipIpcMemHandle_t of the
 *                                                   staging buffer, then the PCI bus id of its device (text) -- the caller carries
 *                                                   them across (e.g. torch.distributed.all_gather_object);
 *   pc_xchg_connect(x, all)                         `all` = world x PC_XCHG_HANDLE_BYTES bytes in rank order: resolves every peer's
 *                                                   PCI bus id to this process's device ordinal, verifies / enables peer access
 *                                                   to it (PC_ERR_UNSUPPORTED with a message in pc_last_hip_error when the device
 *                                                   is not visible to this process or not reachable), THEN maps the peers'
 *                                                   buffers; a failed connect closes what it opened and leaves the handle as it was;
 *   pc_xchg_connect_local(x, ranks)                 the in-process form: `ranks` = the world's pc_xchg handles in rank order, all created
 *                                                   in THIS process (one process driving several devices -- peer access is verified /
 *                                                   enabled -- or several ranks on one device, each launching on its own stream);
 *   pc_xchg_allreduce_group(ranks, buckets, stream) the exchanges of ALL ranks of such an in-process group on ONE device as one launch
 *                                                   (bucket[r] := the rank-ordered sum, for every r): the ranks' workgroups are then
 *                                                   co-resident by construction -- separate launches on separate streams are not (HIP
 *                                                   multiplexes streams onto a few hardware queues) and must not be used with more
 *                                                   ranks per device than hardware queues; PC_ERR_UNSUPPORTED when world x
 *                                                   ceil(n_floats / 1024) workgroups exceed what the device holds at once;
 *   pc_xchg_set_timeout(x, seconds)                 patience of a wait inside the exchange kernel (default 20 s);
 *   pc_xchg_allreduce(x, bucket, stream)            in place, asynchronous on `stream`, capturable into a HIP graph: bucket[0..n)
 *                                                   := sum over ranks (rank order) of their buckets.  Every rank must make the
 *                                                   same sequence of calls;
 *   pc_xchg_status(x)                               synchronises the device; PC_ERR_TIMEOUT if a wait inside any call gave up
 *                                                   (the timeout passed without a peer's flag: the kernel then finishes with a
 *                                                   WRONG sum rather than hang the GPU, and later calls on the handle do not wait
 *                                                   again): the caller must check it wherever it synchronises and abort the job;
 *   pc_xchg_destroy(x)                              after every rank has finished using it (the caller synchronises the ranks). */
#define PC_XCHG_HANDLE_BYTES 128
int pc_xchg_create(int device, int rank, int world, int64_t n_floats, pc_xchg** out);
int pc_xchg_local_handle(pc_xchg* x, void* handle_out);
int pc_xchg_connect(pc_xchg* x, const void* all_handles);
int pc_xchg_connect_local(pc_xchg* x, pc_xchg* const* ranks);
int pc_xchg_allreduce_group(pc_xchg* const* ranks, float* const* buckets, void* stream);
int pc_xchg_set_timeout(pc_xchg* x, double seconds);
int pc_xchg_allreduce(pc_xchg* x, float* bucket, void* stream);
int pc_xchg_status(pc_xchg* x);
void pc_xchg_destroy(pc_xchg* x);

const char* pc_strerror(int code);
/* Detail of the last error on this thread: the HIP error string behind a PC_ERR_HIP, or what made pc_env_create answer
 * PC_ERR_UNSUPPORTED (e.g. an F32 handle for a track that does not fit 2000 px).  Empty when there is none. */
const char* pc_last_hip_error(void);
/* 0 in every shipped build.  Non-zero only in the separate developer library `make ablate` builds
 * (libppocar_ablate.so, -DPC_ABLATE=n: timing ablations that skip parts of the rollout kernel); bench.py and the
 * tests refuse to run on such a build.  There is no run-time switch that makes a kernel do less work. */
int pc_build_ablate(void);
/* Kernel-launch geometry of the last pc_env_step on this handle (lanes per env, rays per lane,
 * blocks, threads) -- for bench.py / DESIGN.md; any pointer may be NULL. */
int pc_env_launch_info(const pc_env* e, int* lanes_per_env, int* rays_per_lane, int* blocks, int* threads);
/* What pc_env_create made of track `track` of this handle: its wall count (car_env.py:653-670), the vertices of its wall chains,
 * and -- F32 handles -- how many wall segments carry the "resolve by the float64 chain scan" mark (walls that cross or touch
 * without being chain neighbours, spikes, walls shorter than the corner margin: exact, but every ray that selects one of them
 * costs an O(n_walls) float64 scan).  A track where that is a large share of the walls runs correctly and SLOWLY in dtype f32: the
 * Python host layer warns above 25 %.  F64 handles: the same count where the persistent kernel's selector form can run on the track
 * (PC_KERNEL_K9_LITERAL), else 0.  Any pointer may be NULL. */
int pc_env_track_info(const pc_env* e, int track, int* n_walls, int* n_chain_vertices, int* n_scan_segments);
/* Which persistent kernel the last successful pc_rollout on this handle launched (0 before the first; for bench.py, the tests and
 * DESIGN.md -- every kernel fills the same buffers bit for bit, this only says which one did):
 *   PC_KERNEL_K9          big form, float32-selector env step with float64 refinement (F32 handles)
 *   PC_KERNEL_K9M / _LITERAL  K9 with 16 envs per wave (4 lanes per env): 8193 .. 32768 envs at 16 rays (F32 / F64 handles)
 *   PC_KERNEL_K9S         small form (F32 handles, small batches)
 *   PC_KERNEL_K9_LITERAL  big form on an F64 handle: the float32 sweep selects each ray's wall, the reference's literal float64
 *                         arithmetic measures it (12 / 16 / 32 nominal rays, tracks inside the selector's limits, every env's rotation
 *                         on the track's rotation table: what reset and stepping produce)
 *   PC_KERNEL_K9S_LITERAL the same literal form inside the small form (F64 handles, 12 / 16 nominal rays, up to 8192 envs)
 *   PC_KERNEL_K9D_SELECTOR F64 handle, the generic kernel with the per-step kernel's selector step (sweep over the wall chain in
 *                         global memory + literal cast): tracks of more than 64 chain vertices, bf16 x 3, rotations off the table
 *   PC_KERNEL_K9D_FILTER  F64 handle, the filter form: every (ray, wall) pair in float64 (any track; 12 / 16 nominal rays) */
#define PC_KERNEL_NONE 0
#define PC_KERNEL_K9 1
#define PC_KERNEL_K9S 2
#define PC_KERNEL_K9_LITERAL 3
#define PC_KERNEL_K9D_FILTER 4
#define PC_KERNEL_K9S_LITERAL 5
#define PC_KERNEL_K9D_SELECTOR 6
#define PC_KERNEL_K9M 7
#define PC_KERNEL_K9M_LITERAL 8
int pc_env_last_rollout_kernel(const pc_env* e);
/* Override the lanes-per-env choice (power of two 1..64; 0 = automatic).  Tuning knob for bench.py. */
int pc_env_set_lanes_per_env(pc_env* e, int lanes_per_env);

#ifdef __cplusplus
}
#endif
#endif /* PPOCAR_H */
