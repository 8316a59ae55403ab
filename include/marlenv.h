/*
 * marlenv.h — C ABI of libmarlenv_hip.so, the MI355X (gfx950) batched
 * intersection environment.
 *
 * This is the drop-in boundary that replaces the reference's pybind11 module
 * `MARLEnv` (reference cpp/bindings.cpp:11-95) as reached through
 * cpp_backend.py (reference cpp_backend.py:30-66) and env.py (reference
 * env.py:80-221).  One handle holds E independent environment instances
 * ("envs") of the reference's IntersectionEnv (reference
 * cpp/IntersectionEnv.h:23-105), each with N ego agents and (traffic mode) up
 * to max_npcs NPC cars, resident on ONE GPU in structure-of-arrays layout.
 *
 * Conventions
 *  - Every function returns 0 on success or a negative MEV_E* code; the
 *    message is available from mev_last_error() (thread-local).  No C++
 *    exception crosses this boundary.
 *  - Buffers are caller-owned.  Host pointers unless MEV_DEVICE_PTRS is set in
 *    the call's flags, in which case every pointer in that call is a device
 *    pointer on the handle's device and the call does not synchronise.
 *  - All work of a handle is ordered on one HIP stream (mev_set_stream).
 *  - Lane points are numbered 0..8L-1: "IN_k" -> k-1, "OUT_k" -> 4L+k-1
 *    (reference cpp/RouteGen.cpp:7-53).  A route is a (start point, end point)
 *    pair (reference IntersectionEnv::add_car_with_route,
 *    cpp/IntersectionEnv.cpp:78-131).
 *  - Status codes: 0 ALIVE, 1 DEAD, 2 SUCCESS, 3 CRASH_WALL, 4 CRASH_LINE,
 *    5 CRASH_CAR (the strings of reference cpp/Reward.h:16-29 / env.py:193).
 */
#ifndef MARLENV_H
#define MARLENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MEV_ABI_VERSION 3  /* 2: MEV_GATHER_STATE, MEV_PK_STATE (MEV_PK_FIELDS 7 -> 8), mev_unpack_gathered;
                              3: mev_set_car_dims / mev_get_car_dims, mev_set_beam_angles / mev_get_beam_angles,
                              mev_decode_errors, snapshot format 2 (car sizes, route table check) */

enum {
    MEV_OK = 0,
    MEV_E_INVALID = -1,  /* bad argument / configuration          */
    MEV_E_HIP = -2,      /* HIP runtime error                      */
    MEV_E_NOMEM = -3,    /* device or host allocation failed       */
    MEV_E_RANGE = -4     /* index out of range (std::out_of_range) */
};

enum { MEV_ALIVE = 0, MEV_DEAD = 1, MEV_SUCCESS = 2, MEV_CRASH_WALL = 3, MEV_CRASH_LINE = 4, MEV_CRASH_CAR = 5 };

/* flags for mev_step / mev_reset / mev_get_outputs */
#define MEV_DEVICE_PTRS 0x1u /* all pointers in this call are device pointers; no host sync */
#define MEV_AUTO_RESET 0x2u  /* an env whose previous step ended (terminated|truncated) is reset
                                before this step (gym-style vector auto-reset) */
/* MEV_GATHER_TO_ROOT (0x4) is declared with the multi-GPU entry points below */

typedef struct mev_handle mev_handle;

/* Configuration: fields mirror reference env.py:81-131 config keys and
 * IntersectionEnv::configure* (cpp/IntersectionEnv.cpp:50-64). */
typedef struct {
    int32_t num_envs;        /* E >= 1                                                     */
    int32_t num_agents;      /* N, 1..64 ego cars per env                                   */
    int32_t num_lanes;       /* lanes per direction (reference default 3)                  */
    int32_t lidar_rays;      /* R in [1, 1024] (reference hard-codes 96, IntersectionEnv.cpp:113) */
    float lidar_fov_deg;     /* 360                                                        */
    float lidar_max_dist;    /* 250 px                                                     */
    float lidar_step;        /* 4 px                                                       */
    int32_t obs_dim;         /* 0 => 31 + R; 127 reproduces the reference layout exactly   */
    int32_t traffic_flow;    /* NPC traffic mode (TrafficFlow.cpp)                          */
    float traffic_density;   /* arrival rate (1/s), clamped >= 0                            */
    int32_t use_team_reward;
    int32_t respawn_enabled;
    int32_t max_steps;       /* truncation; <= 0 disables                                   */
    float reward[8];         /* k_prog, v_min_ms, k_stuck, k_cv, k_co, k_succ, k_sm, alpha  */
    int32_t max_npcs;        /* NPC slots per env, 0..64 (overflowing spawns are dropped)    */
    uint64_t seed;           /* on-device Philox stream for NPC spawns                      */
    int32_t device;          /* HIP device ordinal                                          */
} mev_config;

/* Per-step arguments (reference IntersectionEnv::step, cpp/IntersectionEnv.cpp:133-392,
 * + get_observations :418-520). */
typedef struct {
    const float* actions;       /* [E][N][2] (throttle, steer); never clipped (Car.cpp:9-40) */
    float dt;                   /* seconds (reference default 1/60)                          */
    const int32_t* spawn_route; /* optional [E]: traffic-route index the NPC spawner uses this
                                   step (-1 = no spawn attempt); NULL = on-device Philox draw.
                                   Replays the reference's RNG decisions (TrafficFlow.cpp:275-329). */
    float* obs;                 /* optional [E][N][obs_dim]                                  */
    float* reward;              /* optional [E][N]                                           */
    uint8_t* done;              /* optional [E][N]                                           */
    uint8_t* status;            /* optional [E][N]                                           */
    uint8_t* terminated;        /* optional [E]                                              */
    uint8_t* truncated;         /* optional [E]                                              */
    int32_t* agents_alive;      /* optional [E]                                              */
    int32_t* step;              /* optional [E] step counter after this step                 */
    uint32_t flags;             /* MEV_DEVICE_PTRS | MEV_AUTO_RESET                           */
} mev_step_args;

/* Full simulator state, SoA.  Ego arrays are [E][N], NPC arrays [E][max_npcs].
 * Any NULL pointer is skipped.  Replaces EnvState/get_state/set_state
 * (reference cpp/EnvState.h:9-15, cpp/IntersectionEnv.cpp:394-416) and exposes
 * the Car fields the pybind layer hides (acc, steering_angle, spawn_state,
 * prev_dist_to_goal, prev_action; cpp/Car.h:16-46). */
typedef struct {
    float *x, *y, *v, *heading, *acc, *steering, *prev_dist, *prev_a0, *prev_a1;
    float *spawn_x, *spawn_y, *spawn_v, *spawn_heading;
    int32_t *path_index, *route, *intention;
    uint8_t* alive;
    float *npc_x, *npc_y, *npc_v, *npc_heading, *npc_acc, *npc_steering;
    int32_t *npc_path_index, *npc_route, *npc_intention;
    uint8_t* npc_alive;
    int32_t* npc_count;  /* [E] */
    int32_t* step_count; /* [E] */
} mev_state;

const char* mev_last_error(void);
int mev_abi_version(void);
int mev_device_count(int32_t* count);

int mev_config_default(mev_config* cfg);
int mev_create(const mev_config* cfg, mev_handle** out);
int mev_destroy(mev_handle* h);
int mev_get_config(const mev_handle* h, mev_config* cfg);
int mev_obs_dim(const mev_handle* h, int32_t* obs_dim);
/* A handle starts on its own non-blocking stream.  mev_set_stream orders all
 * later work on `stream` (a hipStream_t; NULL = the legacy default stream),
 * e.g. torch.cuda.current_stream().cuda_stream; mev_use_own_stream reverts. */
int mev_set_stream(mev_handle* h, void* stream);
int mev_use_own_stream(mev_handle* h);
int mev_sync(mev_handle* h);

/* Runtime reconfiguration, effective from the next step: reference
 * IntersectionEnv::configure / configure_traffic (cpp/IntersectionEnv.cpp:50-60)
 * and writes to its reward_config (env.py:57-77, cpp/Reward.h:5-14). */
int mev_configure(mev_handle* h, int32_t use_team, int32_t respawn, int32_t max_steps);
int mev_configure_traffic(mev_handle* h, int32_t enabled, float density);
int mev_set_reward(mev_handle* h, const float* reward8);

/* Host-side single-car helpers with the reference's exact arithmetic, for API
 * parity with the bound MARLEnv.Car methods (cpp/bindings.cpp:24-25); they do
 * not touch any device.  kin = {x, y, v, heading, acc, steering_angle}
 * (Car::update, cpp/Car.cpp:9-40); box = {x, y, heading, length, width}
 * (Car::check_collision, cpp/Car.cpp:86-141). */
int mev_car_update(float* kin, float throttle, float steer_input, float dt);
/* y[i] = tanh_c(x[i]) for i < n: the tanh of the rollout policies' activations (mev_policy_create, "THE
 * ARITHMETIC IS PART OF THE CONTRACT"), the very function the kernels run.  A host helper: no handle, no device.
 * x == y is allowed.  n < 0, or a null array with n > 0: MEV_E_INVALID. */
int mev_tanh(const float* x, float* y, int64_t n);
int mev_car_check_collision(const float* box_a, const float* box_b, int32_t* collide);

/* Lane points / routes (reference cpp/RouteGen.cpp). */
int mev_num_points(const mev_handle* h, int32_t* n);
int mev_point_xy(const mev_handle* h, int32_t point, float* xy);
int mev_route_id(const mev_handle* h, int32_t start_point, int32_t end_point, int32_t* route);
/* path [max(n, 160)][2], intent, spawn (x, y, heading) of a route of n points
 * (mev_route_len; a route of n < 160 points reads back padded with its last point) */
int mev_route_info(const mev_handle* h, int32_t route, float* path, int32_t* intent, float* spawn);
int mev_route_len(const mev_handle* h, int32_t route, int32_t* npoints);
int mev_path_len(void);
/* A route of the caller's own: path [npoints][2], 2 <= npoints <= 4096 (every
 * path the reference generates has 160, RouteGen.cpp:111-205), and intent (0
 * straight, 1 left, 2 right) appended to the handle's route table; *route
 * receives its id (>= P*P, the lane-layout routes).  Cars and NPCs then take it
 * like any route (mev_set_ego_routes, mev_set_state); a reset spawns at path[0]
 * heading to path[1].  Replaces assigning Car.path in the reference
 * (cpp/bindings.cpp:29, a read-write std::vector member): every reader clamps
 * to path.size() (Car.cpp:56, IntersectionEnv.cpp:177-179,446,
 * TrafficFlow.cpp:55,89,263), as the device does, also for a car whose
 * path_index lies past its path's end (set through mev_set_state: the index
 * search keeps it, the look-ahead clamps to path.back(), an NPC's ghost scan is
 * empty).  A path longer than the table's rows re-lays the table out at that
 * length rounded up to 16 points (one re-upload; every route keeps its ids).
 * mev_add_route(h, path, intent, route) = mev_add_route_n(h, path, 160, ...). */
int mev_add_route(mev_handle* h, const float* path, int32_t intent, int32_t* route);
int mev_add_route_n(mev_handle* h, const float* path, int32_t npoints, int32_t intent, int32_t* route);
/* Per-car size: reference Car::length / Car::width (cpp/Car.h:19-20), read-write through
 * cpp/bindings.cpp:24-25 and used by Car::corners (status tests and the SAT car-car
 * collision, Car.cpp:86-141) and by the LiDAR's box of each car (Lidar.cpp:65-75).
 * ego_dims [E][N][2] and npc_dims [E][max_npcs][2] hold (length, width) in px; NULL leaves
 * that array unchanged.  Every car starts at the reference's 54 x 24 px; a reset (and the
 * MEV_AUTO_RESET of mev_step) gives its egos that size again (new Cars, reference
 * IntersectionEnv::reset + add_car_with_route), a spawned NPC has it, a respawned ego keeps
 * its own (Car::respawn, Car.cpp:76-84); NPC sizes move with their NPCs.  Values must be
 * finite with |value| <= 1e4.  While any car differs from 54 x 24 the steps run the
 * runtime-layout kernels (k_cars + k_lidar or k_step without the compile-time layouts; no
 * step server) -- mev_car_dims_active says whether that is the case. */
int mev_set_car_dims(mev_handle* h, const float* ego_dims, const float* npc_dims);
int mev_get_car_dims(mev_handle* h, float* ego_dims, float* npc_dims);
int mev_car_dims_active(const mev_handle* h, int32_t* active);
/* LiDAR beam offsets (radians, [lidar_rays]): reference Lidar::rel_angles (cpp/Lidar.h:17,
 * read-write through cpp/bindings.cpp:92), by default the cfg's fov formula
 * (Lidar.cpp:4-14).  Lidar::update casts beam i along heading + rel_angles[i] for i < rays
 * (Lidar.cpp:24-25), so a reference Lidar whose rays was lowered casts the first rays
 * angles of its list: a handle of that many rays with those angles reproduces it.  Any
 * finite list with |angle| <= 1000 is taken; one the car-pair culling cannot model
 * linearly (uneven beyond 1e-5 rad, descending, constant, wider than a revolution) is
 * simulated without that culling (exact, slower). */
int mev_set_beam_angles(mev_handle* h, const float* rel);
int mev_get_beam_angles(mev_handle* h, float* rel);
/* Ego routes for every (env, agent): route ids [E][N] (reference env.py:104-106,148-151). */
int mev_set_ego_routes(mev_handle* h, const int32_t* routes);
/* NPC route list (reference configure_routes / init_traffic_routes, TrafficFlow.cpp:198-238). */
int mev_set_traffic_routes(mev_handle* h, const int32_t* routes, int32_t count);
int mev_default_traffic_routes(const mev_handle* h, int32_t* routes, int32_t* count);

/* Reset the envs selected by env_mask ([E], NULL = all): reference
 * IntersectionEnv::reset + add_car_with_route per agent (cpp/IntersectionEnv.cpp:66-131).
 * Writes the reset observation (LiDAR block = 1.0: no cast at reset). */
int mev_reset(mev_handle* h, const uint8_t* env_mask, float* obs, uint32_t flags);

/* One step of every env. */
int mev_step(mev_handle* h, const mev_step_args* args);

/* Frame skip / action repeat: hold one action for up to `repeat` steps of every env in
 * one call, as the reference's driver does (test.py:144-155: the reward summed over the
 * sub-steps, stopping at terminated or truncated).  Per env, with n = repeat:
 *
 *   if MEV_AUTO_RESET and the env's previous call ended: reset it, exactly as mev_step does
 *   for s = 1..n:
 *       r = IntersectionEnv::step(actions, dt)     (cpp/IntersectionEnv.cpp:133-392)
 *       acc[i] = s == 1 ? r.rew[i] : acc[i] + r.rew[i]             (f32, in this order)
 *       if r.done[i]: any_done[i] = 1, latched[i] = r.status[i]
 *       k = s;  if r.terminated or r.truncated: break
 *
 * obs is the observation after sub-step k (the LiDAR block cast once, from the state the
 * env stopped at, respawns included: Lidar::update feeds only get_observations,
 * cpp/IntersectionEnv.cpp:374-390, :418-520, and no step reads a LiDAR distance); reward
 * = acc; done = any_done; status = latched[i] where any_done[i], else sub-step k's;
 * terminated, truncated, agents_alive and step are sub-step k's; substeps[e] = k.  An env
 * that stops early keeps the state of sub-step k and is pending for the next auto-reset
 * as after a single step.  step.spawn_route, if given, is [repeat][E] (row s - 1: sub-step
 * s); with the Philox spawner sub-step s uses the handle's counter + (s - 1), the route draw
 * of an auto-reset the first sub-step's, and the counter advances by n per call whatever
 * the envs did -- so for envs that do not end inside the window one call leaves the handle
 * (state, outputs, later random draws) exactly where n mev_step calls with these actions
 * would.  repeat = 1 equals mev_step on every output bit.
 * step.flags: MEV_DEVICE_PTRS | MEV_AUTO_RESET (MEV_GATHER_TO_ROOT and a repeat outside
 * 1..MEV_MAX_REPEAT: MEV_E_INVALID, the handle untouched).  The call runs launched (a
 * resident step server is stopped first) on the runtime-layout kernels, whatever
 * mev_set_step_kernel says, and is not counted by mev_kernel_timing.  The outputs are
 * the handle's last outputs for mev_get_outputs, mev_device_outputs, mev_output_dlpack
 * and snapshots, as after mev_step.
 * Measured (profiles/repeat_sweep.json): at 4096 envs x 8 agents x 64 beams one
 * call takes 71.5 us against 114.7 us for four mev_step calls (1.60x; 2.15x at repeat 8, level
 * at 2, slower than mev_step at 1); one-ego traffic does not gain (0.60x at repeat 4). */
#define MEV_MAX_REPEAT 64
typedef struct {
    mev_step_args step;   /* as mev_step; spawn_route, if given, is [repeat][E]          */
    int32_t repeat;       /* 1..MEV_MAX_REPEAT                                           */
    int32_t* substeps;    /* optional [E]: sub-steps executed                            */
} mev_repeat_args;
int mev_step_repeat(mev_handle* h, const mev_repeat_args* args);

/* Open-loop plan rollout: mev_step_repeat's loop with an action row and a dt of its own per
 * sub-step -- what a planner (CEM, MPPI, tree search) evaluates: T different actions, every
 * sub-step's reward and done to discount, the observation only at the leaf.  Per env, with
 * T = length, actions[s] = row s - 1 of step.actions ([T][E][N][2]), dt_s = dt_seq ?
 * dt_seq[s - 1] : step.dt:
 *
 *   if MEV_AUTO_RESET and the env's previous call ended: reset it, exactly as mev_step does
 *   for s = 1..T:
 *       r = IntersectionEnv::step(actions[s], dt_s)       (cpp/IntersectionEnv.cpp:133-392)
 *       reward_seq[s-1][i] = r.rew[i];  done_seq[s-1][i] = r.done[i];  status_seq[s-1][i] = r.status[i]
 *       acc[i] = s == 1 ? r.rew[i] : acc[i] + r.rew[i]             (f32, in this order)
 *       if r.done[i]: any_done[i] = 1, latched[i] = r.status[i]
 *       k = s;  if r.terminated or r.truncated: break
 *   rows s >= k of reward_seq / done_seq / status_seq = 0.0f / 0 / 0
 *
 * obs, reward (= acc), done (= any_done), status (latched), terminated, truncated, agents_alive,
 * step and substeps[e] = k are defined exactly as for mev_step_repeat; the LiDAR is cast once,
 * from the state the env stopped at.  The *_seq rows before k hold that sub-step's outputs exactly
 * as mev_step would write them (team mix included); the rows from k on are zero, so a
 * discounted sum over all T rows needs no mask (the stopping wave writes them itself: no
 * preparation of the arrays is needed).  The *_seq arrays are the caller's only: they are not
 * part of mev_get_outputs, snapshots or DLPack.  Between sub-steps the actions differ, so the
 * reward's smoothness term sees each sub-step's own previous action, as in single steps.
 * step.spawn_route, if given, is [T][E]; with the Philox spawner sub-step s uses the handle's
 * counter + (s - 1) and the counter advances by T per call; sub-step s spawns with probability
 * 1 - expf(-density * dt_s), computed on the host as mev_step does.  dt_seq is therefore ALWAYS a
 * host pointer, read before the call returns -- a by-value parameter like step.dt, also with
 * MEV_DEVICE_PTRS.  So for envs that do not end inside the window one call leaves the handle
 * (state, outputs, later random draws) exactly where T mev_step calls with actions[s], dt_s
 * would; with every row equal and dt_seq NULL every shared output equals mev_step_repeat(repeat
 * = T) bit for bit.
 * step.flags: MEV_DEVICE_PTRS | MEV_AUTO_RESET (MEV_GATHER_TO_ROOT, a length outside
 * 1..MEV_MAX_REPEAT or null actions: MEV_E_INVALID, the handle untouched).  Launch path as
 * mev_step_repeat: a resident step server is stopped first, the runtime-layout kernels run
 * (any N <= 64, <= 64 NPC slots, per-car sizes, any beam list), not counted by
 * mev_kernel_timing.  Host mode stages actions, spawn_route, substeps and the *_seq arrays in the
 * handle's staging block, which every host-mode call shares and which grows to the largest call
 * seen (no more than the call's own rows), and is synchronous.
 * Measured (python tools/bench_sequence.py -> profiles/sequence_sweep.json): at 4096 envs x
 * 8 agents x 64 beams one call with all three *_seq arrays takes 73.9 us at T = 4 against 102.1 us for four
 * mev_step calls with the same actions (1.38x), 109.7 against 205.5 us at T = 8 (1.87x), 180.9 against 412.9 us
 * at T = 16 (2.28x); at T = 2 it loses (56.3 against 51.1 us, 0.91x).  A further sub-step costs 8.9 us (8.4 us in
 * mev_step_repeat: the difference is the sub-step's action load).  One-ego traffic (4096 x 1 x 64, density 0.5)
 * loses to single steps at every length, as frame skip does: 174.3 against 103.5 us at T = 4 (0.59x), 0.67x at
 * T = 16. */
typedef struct {
    mev_step_args step;     /* as mev_step, except: step.actions is [length][E][N][2] (row s: sub-step s+1),
                               step.spawn_route, if given, is [length][E]; step.dt is used when dt_seq is NULL */
    int32_t length;         /* T, 1..MEV_MAX_REPEAT */
    const float* dt_seq;    /* optional [length]; ALWAYS a host pointer, read before the call returns
                               (it is a by-value parameter like step.dt, also with MEV_DEVICE_PTRS) */
    float*   reward_seq;    /* optional [length][E][N]: sub-step s's reward exactly as mev_step would output it */
    uint8_t* done_seq;      /* optional [length][E][N] */
    uint8_t* status_seq;    /* optional [length][E][N] */
    int32_t* substeps;      /* optional [E] */
} mev_sequence_args;
int mev_step_sequence(mev_handle* h, const mev_sequence_args* args);

/* Plan evaluation: score C candidate plans from the LIVE batch and leave the handle untouched -- what
 * a sampling planner (CEM, MPPI, tree search) does every iteration.  Candidate c starts from a private
 * copy of live env r = roots[c] (ego state, NPC slots and count, step counter, car sizes) and runs
 * exactly mev_step_sequence's loop without MEV_AUTO_RESET (a root whose last step ended is stepped on
 * from its stored state, as mev_step does without the flag), with actions[s] = row s - 1 of actions
 * ([T][C][N][2]) and dt_s = dt_seq ? dt_seq[s - 1] : dt.  C is independent of num_envs; any number of
 * candidates may share a root.  Everything read of the starting state is env r's, everything written is
 * indexed by c:
 *
 *   g = 1.0f; ret[i] = 0.0f
 *   for s = 1..T:
 *       r = IntersectionEnv::step(actions[s], dt_s)          on the copy
 *       reward_seq[s-1][c][i] = r.rew[i];  done_seq[s-1][c][i] = r.done[i];  status_seq[s-1][c][i] = r.status[i]
 *       ret[i] = ret[i] + g * r.rew[i];  g = g * gamma       (f32, in this order, no FMA)
 *       k = s;  if r.terminated or r.truncated: break
 *   returns[c][i] = ret[i];  substeps[c] = k;  terminated[c], truncated[c] = sub-step k's flags
 *   rows s >= k of reward_seq / done_seq / status_seq = 0.0f / 0 / 0  (written by the call itself)
 *
 * The *_seq rows are defined exactly as for mev_step_sequence (team mix and bonuses included).
 * spawn_route, if given, is [T][C]: sub-step s takes spawn_route[s-1][c].  Without it the Philox spawner
 * is keyed by the candidate index c in the env's place, with the handle's counter + (s - 1) and the
 * probability 1 - expf(-density * dt_s) computed on the host; the handle's counter is NOT advanced.  So
 * with C == num_envs the call equals mev_restore_map(roots) followed by mev_step_sequence on a handle
 * with the same counter, bit for bit.  dt_seq is ALWAYS a host pointer, read before the call returns.
 * The handle is untouched: state and car sizes, last outputs (mev_get_outputs, DLPack), the Philox
 * counter, the NPC diagnostics and a snapshot's bytes are what they were; the one side effect is that
 * a resident step server is stopped first, as by every non-step call.
 * No leaf observation is returned and no LiDAR is cast, on purpose: the LiDAR hand-off tables are
 * per-env scratch sized by num_envs, and a cast per candidate is the cost this call exists to avoid.  A
 * planner that wants the leaf observation of the winning plan runs that one plan through
 * mev_step_sequence; one that wants every candidate's (a value at the leaf) calls mev_evaluate_leaves below.
 * Errors (MEV_E_INVALID, the handle untouched): null actions or roots, no output pointer at all,
 * candidates outside 1..MEV_MAX_CANDIDATES, length outside 1..MEV_MAX_REPEAT, any flag other than
 * MEV_DEVICE_PTRS.  Host pointers: a root outside [0, E) -> MEV_E_RANGE; the arrays are staged in a
 * per-handle device buffer that grows to the largest call seen, and the call is synchronous.  Device
 * pointers: such a root makes its candidate a no-op with defined outputs -- all its rows, returns,
 * substeps and flags zero (the kernel never reads outside the state arrays) -- and the call does not
 * synchronise.  Launched on the runtime-layout path (any N <= 64, <= 64 NPC slots, per-car sizes, any
 * beam list); not counted by mev_kernel_timing.
 * Measured (python tools/bench_evaluate.py -> profiles/evaluate_sweep.json): at 4096 envs x 8 agents
 * x 64 beams, device pointers, C = 4096 candidates (64 per root), every output: 35.4 us per call at T = 4 against
 * 154.7 us for mev_restore_map + mev_step_sequence (4.37x), 20.7 against 137.6 us at T = 2 (6.66x), 64.1 against
 * 189.1 us at T = 8 (2.95x), 124.1 against 260.1 us at T = 16 (2.10x); the pair's closing mev_restore is another
 * 117.4-118.5 us.  A further sub-step costs 7.4 us (the pair: 8.7).  C = 16384 from the same handle: 122.1 us at
 * T = 4, 0.0075 us per candidate (0.0086 at C = 4096).  One-ego traffic (4096 x 1 x 64, density 0.5) gains too:
 * 91.0 against 220.1 us at T = 4 (2.42x), 388.1 against 595.3 us at T = 16 (1.53x).  No measured shape loses. */
#define MEV_MAX_CANDIDATES (1 << 20)
typedef struct {
    const float*   actions;     /* [length][candidates][N][2]: row s = action of sub-step s+1        */
    const int32_t* roots;       /* [candidates]: the LIVE env each candidate starts from, 0..E-1     */
    const int32_t* spawn_route; /* optional [length][candidates], as mev_step_sequence's             */
    int32_t candidates;         /* C, 1..MEV_MAX_CANDIDATES; independent of num_envs                 */
    int32_t length;             /* T, 1..MEV_MAX_REPEAT                                              */
    float   dt;                 /* used when dt_seq is NULL                                          */
    const float* dt_seq;        /* optional [length]; ALWAYS host, read before the call returns      */
    float   gamma;              /* discount of `returns`                                             */
    float*   returns;           /* optional [C][N]                                                   */
    float*   reward_seq;        /* optional [length][C][N]                                           */
    uint8_t* done_seq;          /* optional [length][C][N]                                           */
    uint8_t* status_seq;        /* optional [length][C][N]                                           */
    int32_t* substeps;          /* optional [C]                                                      */
    uint8_t* terminated;        /* optional [C]: flags of the sub-step the candidate stopped at      */
    uint8_t* truncated;         /* optional [C]                                                      */
    uint32_t flags;             /* MEV_DEVICE_PTRS only                                              */
} mev_evaluate_args;
int mev_evaluate_plans(mev_handle* h, const mev_evaluate_args* args);

/* Plan evaluation with leaf observations: mev_evaluate_plans, and for EVERY candidate the observation
 * of the state it stopped at -- what a planner that adds a learned value at the leaf needs
 * (returns + gamma^k * V(obs_leaf): TD-MPC-style MPPI, AlphaZero / MuZero-style search, n-step
 * bootstrapped critic targets).  Everything mev_evaluate_plans defines holds unchanged and bit for
 * bit: the *_seq rows, returns, substeps, the flags, the Philox spawner keyed by c, the handle's
 * counter not advanced, dt_seq ALWAYS a host pointer.  Every output of `eval` is optional here.
 *
 *   leaf_obs[c][i][0 .. obs_dim) = the row mev_step_sequence would return in obs for agent i of an env
 *   holding a copy of live env roots[c], given candidate c's plan without MEV_AUTO_RESET
 *
 * i.e. the observation after sub-step k = substeps[c]; the head and the LiDAR block are cast once, from
 * the state the candidate stopped at, respawns included.  Every float of every row is written by the
 * call, padding columns beyond 31 + R included: the caller prepares nothing.  With C == num_envs,
 * leaf_obs equals the obs of mev_restore_map(roots) + mev_step_sequence bit for bit.
 * The handle is untouched exactly as for mev_evaluate_plans -- state, car sizes, last outputs
 * (mev_get_outputs, DLPack), Philox counter, NPC diagnostics and a snapshot's bytes -- and its own
 * LiDAR hand-off tables and output buffers are neither read nor written: the candidates hand their
 * poses, candidate masks and obstacle boxes to the cast through a per-handle scratch indexed by
 * candidate.  That scratch only grows, to 64 MiB at the most (33 bytes per agent + 16 per agent and NPC
 * slot: 904 per candidate at 8 agents and the default 32 slots, 4160 at 64 agents + 64 slots); a call
 * with more candidates than it holds runs in chunks -- rollout, then cast, per chunk, in stream order --
 * with the same results.
 * MEV_LEAF_CHUNK=n in the environment at mev_create fixes the chunk at n candidates (tests).
 * Errors (MEV_E_INVALID, the handle untouched): null leaf_obs, and everything mev_evaluate_plans
 * refuses except "no output pointer at all" (leaf_obs is one).  Host pointers: a root outside [0, E) ->
 * MEV_E_RANGE; leaf_obs is staged through the same per-handle staging block as the other arrays, and
 * the call is synchronous.  Device pointers: such a root makes its candidate a no-op whose leaf_obs
 * rows are all zero bits, like its other outputs; other candidates are unaffected; the call does not
 * synchronise.  Launched on the runtime-layout path, as mev_evaluate_plans (any N <= 64, <= 64 NPC
 * slots, per-car sizes, any beam list including lists that run without culling); not counted by
 * mev_kernel_timing.
 * Measured (python tools/bench_evaluate_leaves.py -> profiles/evaluate_leaves_sweep.json; the method of
 * mev_evaluate_plans' figures): at 4096 envs x 8 agents x 64 beams, device pointers, C = 4096 candidates (64 per
 * root), every output: 74.2 us per call at T = 4 against 154.1 us for mev_restore_map + mev_step_sequence in the same
 * session (2.08x), 55.1 against 135.8 us at T = 2 (2.46x), 110.1 against 189.1 us at T = 8 (1.72x), 183.6 against
 * 271.4 us at T = 16 (1.48x); the pair's closing mev_restore is another 117.8-141.9 us.  Over mev_evaluate_plans on
 * the same inputs the leaves cost 34.4 us at T = 2 to 52.8 us at T = 16 (the cast is one k_lidar, about 31 us); a
 * further sub-step costs 9.2 us against 7.9 us for mev_evaluate_plans (it builds the obstacle table) and 9.7 us for the
 * pair.  C = 16384 from the same handle: 247.1 us at T = 4, 0.0151 us per candidate (0.0181 at C = 4096).  One-ego
 * traffic (4096 x 1 x 64, density 0.5): 132.0 against 227.2 us at T = 4 (1.72x), 483.3 against 592.5 us at T = 16
 * (1.23x).  Every measured shape is below the pair by far more than the blocks' spreads. */
typedef struct {
    mev_evaluate_args eval;  /* exactly as mev_evaluate_plans; every output in it is optional here */
    float* leaf_obs;         /* required, [C][N][obs_dim] */
} mev_leaf_args;
int mev_evaluate_leaves(mev_handle* h, const mev_leaf_args* args);

/* State pools: complete env states kept on the device OUTSIDE the live batch, so that a search can
 * expand nodes that are not the root (mev_expand_plans below).  A pool has 1..MEV_MAX_POOL_SLOTS
 * slots and belongs to the handle it was created from; mev_destroy releases the handle's remaining
 * pools (their pointers are dead afterwards).  A slot holds one env's whole simulator state as
 * structure-of-arrays over slots in the handle's own field layout: every ego field of mev_state, the
 * NPC slots and count, the step counter and the car sizes of egos and NPCs -- no outputs, no LiDAR
 * hand-off, no pending-reset flag.  Each slot has a valid byte that starts at 0; storing into the
 * slot sets it to 1.  mev_set_car_dims clears the valid bytes of all the handle's pools, on the
 * handle's stream (whether the per-car-size regime applies is a property of the whole handle, and a
 * slot stored before must not be read under another); nothing else invalidates a slot.  Pools are
 * not part of snapshots, mev_get_outputs or DLPack.  mev_pool_create: MEV_E_INVALID for a slot count
 * out of range, MEV_E_NOMEM when the allocation fails (about 76 N + 48 max_npcs + 9 bytes per slot).
 *
 * mev_pool_capture copies live env envs[i] into slot slots[i], i < count, without stepping: a tree's
 * root node.  flags: MEV_DEVICE_PTRS only.  Host pointers: an env outside [0, E) or a slot outside
 * [0, slots) -> MEV_E_RANGE, nothing changed; synchronous.  Device pointers: such a pair is skipped,
 * and the call does not synchronise.  A slot named twice holds one of the two envs.
 *
 * mev_pool_get_state is a host read-back for tests and debugging: the arrays of `out` (each
 * optional) are [count][N] / [count][max_npcs] / [count] in mev_state's field meaning, row i = slot
 * slots[i]; ego_dims [count][N][2] and npc_dims [count][max_npcs][2] in mev_get_car_dims' layout;
 * valid [count].  slots is a host pointer (an entry out of range -> MEV_E_RANGE).  It synchronises
 * the handle's stream.  NPC slots at or beyond a slot's npc_count hold unspecified values. */
typedef struct mev_pool mev_pool;
#define MEV_MAX_POOL_SLOTS (1 << 20)
int mev_pool_create(mev_handle* h, int32_t slots, mev_pool** out);
int mev_pool_destroy(mev_pool* pool);
int mev_pool_slots(const mev_pool* pool, int32_t* slots);
int mev_pool_capture(mev_handle* h, mev_pool* pool, const int32_t* envs, const int32_t* slots, int32_t count,
                     uint32_t flags);
int mev_pool_get_state(mev_pool* pool, const int32_t* slots, int32_t count, const mev_state* out, float* ego_dims,
                       float* npc_dims, uint8_t* valid);

/* Plan expansion: mev_evaluate_plans (with leaf_obs: mev_evaluate_leaves) whose candidates may START
 * from a slot of a pool and whose STOP STATE is kept in one -- the node expansion of a tree search
 * below depth one (AlphaZero / MuZero-style search, beam search, multi-level MPPI).  Everything the
 * two calls define holds bit for bit, with two additions.
 *
 * Where a candidate starts.  src == NULL: live env roots[c], as before.  Otherwise a private copy of
 * slot roots[c] of src.  A root outside [0, slots of src), or a slot whose valid byte is 0, is
 * handled exactly like an out-of-range root of mev_evaluate_plans: MEV_E_RANGE with host pointers; with
 * device pointers the candidate is a no-op whose every output is zero.  Nothing is stored for it.
 *
 * What is kept.  For a candidate that ran, with d = dst_slots[c] in [0, slots of dst): at the sub-step
 * it stops at (terminated, truncated or the last) slot d of dst receives the state mev_step_sequence
 * would leave in an env that held a copy of the root and ran this plan without MEV_AUTO_RESET -- every
 * field mev_get_state and mev_get_car_dims report, the respawns of that sub-step included -- and the
 * slot's valid byte becomes 1.  dst_slots[c] == -1 (with device pointers: any value out of range)
 * stores nothing and leaves every slot as it was.
 *
 * Philox: sub-step s uses the handle's counter + counter_offset + (s - 1), keyed by c.  Composition:
 * expanding T1 sub-steps into slot d, then T2 from slot d with counter_offset raised by T1 and the same
 * candidate index, gives a candidate that did not end in the first part the same rows, flags, stop
 * state and leaf_obs as one call with the concatenated plan (returns restart at g = 1 per call).
 *
 * The live batch, last outputs, Philox counter, NPC diagnostics and a snapshot's bytes are untouched,
 * exactly as for mev_evaluate_plans.  src == dst is allowed (one tree in one pool); the dst_slots of
 * the call must then be disjoint from its roots, and dst_slots must never name a slot twice.  Host
 * pointers: both are checked before anything is launched (MEV_E_INVALID, nothing changed).  Device
 * pointers: the caller's contract -- the offending slots' contents are unspecified, every access
 * stays inside the pool.
 * Errors as mev_evaluate_plans, plus a null dst or dst_slots and a pool of another handle
 * (MEV_E_INVALID); "no output pointer at all" is not an error here, the pool is an output.  Host
 * pointers: a dst_slots entry outside [-1, slots of dst) -> MEV_E_RANGE.  Launch path as the two
 * calls: runtime-layout kernels (any N <= 64, <= 64 NPC slots, per-car sizes, any beam list), a
 * resident step server stopped first, not counted by mev_kernel_timing, host pointers staged and
 * synchronous, device pointers unsynchronised; with leaf_obs the same scratch and chunks
 * (MEV_LEAF_CHUNK honoured).
 * Measured (python tools/bench_expand.py -> profiles/expand_sweep.json; mev_evaluate_plans' method):
 * at 4096 envs x 8 agents x 64 beams, device pointers, C = 4096, every output, medians of five blocks -- the second
 * level of a tree from a pool, one slot per candidate, costs 21.5 / 36.4 / 66.7 us at T = 2 / 4 / 8 (min-max
 * 21.5-23.1, 36.2-36.6, 66.7-66.9) against 34.7 / 64.1 / 124.3 us (34.2-36.1, 63.9-64.3, 124.1-124.5) for
 * mev_evaluate_plans at 2T from the live batch, the only other way there that leaves the batch alone; with leaf_obs
 * 57.0 / 73.9 / 110.1 us against 74.3 / 109.9 / 183.2 us for mev_evaluate_leaves at 2T.  One-ego traffic (4096 x 1 x
 * 64, density 0.5): 45.2 / 82.7 / 158.0 us against 81.7 / 157.9 / 311.7 us, with leaf_obs 76.2 / 130.6 / 235.1 us
 * against 125.6 / 229.8 / 437.0 us.  Every measured shape is below the replay by more than the blocks' spreads (at
 * the least 13.2 us against 1.9 us); no shape loses.  Keeping the stop states costs -1.1 to 3.9 us per call over
 * the evaluation call on the same inputs (at most 1.4 us without leaf_obs). */
typedef struct {
    mev_evaluate_args eval;    /* exactly as mev_evaluate_plans; every output in it optional        */
    float* leaf_obs;           /* optional [C][N][obs_dim], defined exactly as mev_evaluate_leaves' */
    const mev_pool* src;       /* NULL: eval.roots are live envs; else slots of src                 */
    mev_pool* dst;             /* required                                                          */
    const int32_t* dst_slots;  /* [C]: slot that receives candidate c's stop state; -1: not stored  */
    uint64_t counter_offset;   /* Philox: sub-step s uses the handle's counter + counter_offset + (s - 1) */
} mev_expand_args;
int mev_expand_plans(mev_handle* h, const mev_expand_args* args);

/* Sampled plan evaluation: mev_evaluate_plans (with leaf_obs: mev_evaluate_leaves) whose action rows
 * are not read from memory -- the sampling half of a CEM / MPPI iteration.  There are `groups` groups
 * of `samples` candidates; candidate c = g * samples + j starts from live env eval.roots[g] and, for
 * agent i and sub-step row s (0-based), draws
 *
 *   (w0, w1, w2, w3) = Philox4x32-10(key = (lo32(noise_seed), hi32(noise_seed)),
 *                                    counter = (lo32(noise_counter), hi32(noise_counter), c * 64 + i, s))
 *   B(w)   = the sum of the four bytes of w                                 (integer, 0..1020)
 *   eps[0] = ((float)(B(w0) + B(w1)) - 1020.0f) * 0x1.39897ep-8f            (throttle)
 *   eps[1] = ((float)(B(w2) + B(w3)) - 1020.0f) * 0x1.39897ep-8f            (steer)
 *   x      = mean[s][g][i][k] + sigma[s][g][i][k] * eps[k]                  (f32: multiply, then add, no FMA)
 *   action[k] = fminf(fmaxf(x, lo[k]), hi[k])
 *
 * The constant is (float)(1 / sqrt(43690)), bits 0x3b9cc4bf: eight uniform bytes have mean 1020 and
 * variance 43690.  The conversion and the subtraction are exact, so there is one rounded multiply and
 * the noise is the same bits on the host and the device.  eps is an IRWIN-HALL APPROXIMATION of a unit
 * Gaussian, not a Gaussian: mean 0, variance 1, kurtosis 2.85, support +-4.88 in 2041 levels.  A caller
 * who needs another distribution draws the actions itself and calls mev_evaluate_plans.  With
 * MEV_SAMPLE_MEAN_FIRST candidate j == 0 of every group takes eps = 0.0f in the formula: the (clamped)
 * mean plan is always among the candidates.
 * Every output in `eval`, and leaf_obs, is bit for bit what mev_evaluate_plans / mev_evaluate_leaves
 * return for actions = actions_out and roots[c] = eval.roots[c / samples]; the Philox spawner is keyed
 * by c with the handle's counter + (s - 1), as before, and the handle is untouched exactly as for
 * mev_evaluate_plans.  Every element of actions_out is written -- the rows after the sub-step a
 * candidate stopped at and the rows of a candidate without a root too, still the formula's values -- so
 * the caller prepares nothing and mev_update_plans reads only defined data.  With leaf_obs the same
 * scratch and chunks apply (MEV_LEAF_CHUNK honoured; a chunk may cut through a group).
 * Errors (MEV_E_INVALID, the handle untouched): everything the two evaluation calls refuse, non-NULL
 * eval.actions, null mean or sigma, candidates != groups * samples, lo[k] > hi[k] or a non-finite
 * bound, an unknown sample_flags bit; "no output pointer at all" counts leaf_obs and actions_out as
 * outputs.  Host pointers: a root outside [0, E) -> MEV_E_RANGE; mean, sigma and actions_out go through
 * the same staging block, and the call is synchronous.  Device pointers: such a root makes all `samples`
 * candidates of its group the usual all-zero no-ops (their actions_out rows are still the formula's);
 * no synchronisation.  State pools as source or destination: mev_sample_expand_plans below.
 * Measured (python tools/bench_plan_iteration.py -> profiles/plan_iteration_sweep.json; mev_evaluate_plans'
 * method): at 4096 envs x 8 agents x 64 beams, device pointers, 64 groups x 64 candidates, every output, medians of
 * five blocks -- mev_sample_plans + mev_update_plans (softmax) 65.0 us per iteration at T = 4 against 95.1 us for the
 * same iteration in eager torch around mev_evaluate_plans (98.8 against 123.7 us at T = 8; 4096 groups x 4: 163.3
 * against 178.5 us at T = 4; one-ego traffic 118.2 against 140.3 us), below it by more than the blocks' spreads at all
 * five measured shapes.  The call alone costs 3.6 us (T = 4) to 6.8 us (T = 8) more than mev_evaluate_plans on
 * ready-made actions: drawing is about 0.9 us per sub-step at 4096 candidates, not free. */
#define MEV_SAMPLE_MEAN_FIRST 0x1u
typedef struct {
    mev_evaluate_args eval;   /* as mev_evaluate_plans, except: eval.actions must be NULL; eval.roots is [groups]
                                 (the live env of group g); eval.candidates must equal groups * samples; every
                                 output, spawn_route [T][C], dt / dt_seq, gamma and flags as before */
    float* leaf_obs;          /* optional [C][N][obs_dim], defined exactly as mev_evaluate_leaves' */
    const float* mean;        /* [length][groups][N][2] */
    const float* sigma;       /* [length][groups][N][2] */
    float lo[2], hi[2];       /* clamp per component; lo[k] <= hi[k], finite */
    int32_t groups, samples;  /* G >= 1, K >= 1, G * K <= MEV_MAX_CANDIDATES */
    uint64_t noise_seed, noise_counter;
    float* actions_out;       /* optional [length][C][N][2]: the actions the candidates ran */
    uint32_t sample_flags;    /* MEV_SAMPLE_MEAN_FIRST */
} mev_sample_args;
int mev_sample_plans(mev_handle* h, const mev_sample_args* args);

/* Sampled plan expansion: mev_sample_plans whose groups may START from a slot of a pool and whose
 * candidates' STOP STATES are kept in one -- sampled continuations below the root of a tree (beam
 * search over sampled plans, multi-level MPPI, sampled MuZero-style expansion).  It is the two calls
 * at once and defines nothing of its own.  With A = actions_out:
 *   - every output in sample.eval, leaf_obs, and every field of every slot written in dst (the valid
 *     bytes included) is bit for bit what mev_expand_plans returns and stores for actions = A,
 *     roots[c] = sample.eval.roots[c / samples] and the same src, dst, dst_slots and counter_offset;
 *   - A is bit for bit mev_sample_plans' formula, noise at (noise_seed; noise_counter, c * 64 + i, s),
 *     MEV_SAMPLE_MEAN_FIRST honoured: a function of mean, sigma, lo, hi, groups, samples and the noise
 *     stream only, not of src, dst or counter_offset.  Every element of A is written, also for
 *     candidates that stop early or have no root.
 * The live batch, last outputs, Philox counter, NPC diagnostics and a snapshot's bytes are untouched.
 * A root without a state -- roots[g] outside the source, or a src slot whose valid byte is 0 -- is
 * handled per group as mev_sample_plans handles an out-of-range root: MEV_E_RANGE with host pointers,
 * nothing changed; with device pointers all `samples` candidates of the group are the all-zero no-ops,
 * their actions_out rows still the formula's, and nothing is stored for them.
 * Composition: mev_update_plans(MEV_UPDATE_ELITES) writes order[G][M], the elites' candidate indices; with
 * dst_slots[c] = c these are the slots of the next level's roots, so a beam search over sampled plans
 * is sample_expand -> update -> sample_expand -> update ... per level with device pointers throughout:
 * no host round trip and no framework kernel for the noise.  (Raise counter_offset by the sub-steps
 * already run and change noise_counter per level.)
 * Errors: everything mev_sample_plans refuses, plus a null dst or dst_slots and a pool of another handle
 * (MEV_E_INVALID); "no output pointer at all" is not an error, the pool is an output.  Host pointers:
 * mev_expand_plans' checks over the C dst_slots entries, each before anything is launched -- an entry
 * outside [-1, slots of dst) -> MEV_E_RANGE; a slot named twice, or with src == dst an entry that is
 * one of the G roots -> MEV_E_INVALID -- with the handle and the pools unchanged.  Launch path, staging,
 * synchronisation and, with leaf_obs, scratch and chunks (MEV_LEAF_CHUNK honoured; a chunk may cut
 * through a group) as the two calls.
 * Measured (python tools/bench_sample_expand.py -> profiles/sample_expand_sweep.json; mev_evaluate_plans'
 * method): at 4096 envs x 8 agents x 64 beams, device pointers, 64 groups x 64 candidates, every output, medians of
 * five blocks -- the second level of a tree from a pool, one slot per candidate, costs 39.0 us at T = 4 against 54.1 us
 * for the draw in eager torch followed by mev_expand_plans (72.2 against 87.3 us at T = 8; with leaf_obs 79.8 / 119.1
 * against 93.8 / 131.3 us; 4096 groups x 4: 130.6 against 147.1 and 248.4 against 261.9 us, with leaf_obs 259.7 against
 * 271.5 us at T = 4; one-ego traffic 88.8 against 99.1 us, with leaf_obs 124.7 against 137.2 us): below it by more than
 * the blocks' spreads at nine of the ten measured shapes, by 10.3-16.4 us.  At 4096 groups x 4, T = 8 with leaf_obs it
 * is 403.8 against 406.4 us, 2.6 us inside a block spread of 10.7 us: no gain shown there.  Over mev_sample_plans from the
 * live batch the call costs 1.1-4.5 us at 4096 candidates and 4.0-14.3 us at 16384. */
typedef struct {
    mev_sample_args sample;    /* exactly as mev_sample_plans, except: sample.eval.roots[g] is a slot of src when src != NULL */
    const mev_pool* src;       /* NULL: the groups' roots are live envs; else slots of src */
    mev_pool* dst;             /* required */
    const int32_t* dst_slots;  /* [C], C = groups * samples: slot that receives candidate c's stop state; -1: not stored */
    uint64_t counter_offset;   /* NPC spawner: sub-step s uses the handle's counter + counter_offset + (s - 1), keyed by c */
} mev_sample_expand_args;
int mev_sample_expand_plans(mev_handle* h, const mev_sample_expand_args* args);

/* The reduction over each group's candidates: the refit half of a CEM / MPPI iteration.  Candidates
 * c = g * samples + j; score[c] = scores[c], or with scores NULL the f32 sum of returns[c][i] over
 * i = 0..N-1 in that order.  Rank within a group: a ranks before b if score_a > score_b; on equal
 * scores (-0.0f equals +0.0f) the lower j ranks first.  A non-finite score is replaced by -FLT_MAX
 * before anything else (device pointers); with host pointers it is refused with MEV_E_INVALID.
 *
 * MEV_UPDATE_ELITES, exact: with c_0 .. c_{M-1} the first M = elites candidates in rank order, for every
 * (s, g, i, k), in f32, multiply then add:
 *   sum = 0;  for r: sum = sum + a[s][c_r][i][k];              mean = sum / (float)M
 *   q   = 0;  for r: d = a[s][c_r][i][k] - mean;  q = q + d * d
 *   sigma = sqrtf(q / (float)M)
 * MEV_UPDATE_SOFTMAX: m = the best score, x_j = (score_j - m) * inv_temperature, w_j = expf(x_j) (the
 * device's expf, within 1 ulp: the one operation that is not bit-exact against a host), W = the sum of
 * w_j in j order, mean = (sum_j w_j * a) / W, q = (sum_j w_j * d * d) / W with d = a - mean, sigma =
 * sqrtf(q), sums in j order.
 * Both: new_mean = mean, new_sigma = fmaxf(sigma, sigma_min); best[g] = the candidate index c of the
 * group's first-ranked candidate, best_score[g] its score; order (ELITES) = the elites' c in rank
 * order; weights (SOFTMAX) = w / W.  new_mean / new_sigma have mev_sample_plans' layout, ready to be its
 * next input; row 0 of the best candidate (or of new_mean) is an action for mev_step.
 * The call reads and writes only its arguments: the handle supplies N, the device and the stream; its
 * state, outputs and counters are untouched (a resident step server is stopped first).  Host pointers
 * are staged and the call is synchronous; device pointers are not synchronised.
 * Errors (MEV_E_INVALID): null actions, scores and returns both NULL, no output pointer at all, groups
 * < 1, samples outside 1..MEV_MAX_SAMPLES, groups * samples > MEV_MAX_CANDIDATES, length outside
 * 1..MEV_MAX_REPEAT, an unknown mode, elites outside 1..samples (ELITES), inv_temperature negative or
 * non-finite (SOFTMAX), a NaN sigma_min, any flag other than MEV_DEVICE_PTRS. */
enum { MEV_UPDATE_ELITES = 0, MEV_UPDATE_SOFTMAX = 1 };
#define MEV_MAX_SAMPLES 4096
typedef struct {
    const float* actions;    /* [length][C][N][2], C = groups * samples (mev_sample_plans' actions_out, or the caller's own) */
    const float* scores;     /* optional [C]; e.g. returns + gamma^k * V(leaf) computed by the caller */
    const float* returns;    /* [C][N], used when scores is NULL: score[c] = sum over i = 0..N-1, f32, in that order */
    int32_t groups, samples, length;   /* samples <= MEV_MAX_SAMPLES, length 1..MEV_MAX_REPEAT */
    int32_t mode, elites;    /* ELITES: M = elites in 1..samples */
    float inv_temperature;   /* SOFTMAX: 1 / lambda, finite, >= 0 */
    float sigma_min;         /* new_sigma = fmaxf(sigma, sigma_min) */
    float* new_mean;         /* optional [length][groups][N][2] */
    float* new_sigma;        /* optional [length][groups][N][2] */
    int32_t* best;           /* optional [groups]: candidate index c of the group's first-ranked candidate */
    float* best_score;       /* optional [groups] */
    int32_t* order;          /* optional [groups][M] (ELITES): the elites' c in rank order */
    float* weights;          /* optional [C] (SOFTMAX): w / W */
    uint32_t flags;          /* MEV_DEVICE_PTRS */
} mev_update_args;
int mev_update_plans(mev_handle* h, const mev_update_args* args);

/* Closed-loop rollouts: a small MLP policy held by the library, evaluated inside the step kernel's
 * loop on each env's own observation rows -- observe -> act -> step, T times, in ONE launch.
 *
 * A policy has one or two hidden layers of 1..MEV_POLICY_MAX_WIDTH units (hidden[1] == 0: one) and an
 * output layer of 2 units (throttle, steer); in_dim must equal the handle's obs_dim.  Layer l's weights
 * are row-major [out][in] (torch.nn.Linear.weight's layout), its biases [out]; with one hidden layer
 * w[2] / b[2] are not read.  flags: MEV_DEVICE_PTRS, and on mev_policy_create the activation bits below.  Host pointers: every weight and bias must be
 * finite (else MEV_E_INVALID) and the call is synchronous.  Device pointers: no validation, no
 * synchronisation -- the library repacks the weights into its own layout with a small kernel on the
 * handle's stream, so a training loop pushes new weights every iteration without a host copy, and a
 * rollout issued before an update on that stream runs the old weights.  mev_policy_update takes a spec of
 * the same shape.  A policy belongs to its handle: mev_destroy releases the handle's policies.
 *
 * ACTIVATIONS are a property of the policy, fixed by mev_policy_create's flags: MEV_POLICY_HIDDEN_TANH -- every
 * hidden layer applies tanh_c (below) in the ReLU's place -- and MEV_POLICY_OUT_TANH -- mu[k] = tanh_c(layer(W_last,
 * b_last, h)[k]), the squashed mean of DDPG / TD3-style actors.  Without them (flags 0 or MEV_DEVICE_PTRS) the
 * policy is the ReLU policy with a raw mu, and every call gives it the bits it always gave.  mev_policy_update keeps
 * the activations: it accepts MEV_DEVICE_PTRS only, an activation bit there is MEV_E_INVALID and the policy is
 * untouched; any other unknown bit on either call is MEV_E_INVALID.  mev_policy_get_activations reads the two bits
 * back.  In mev_rollout_policies the activations are each listed policy's own.
 *
 * THE ARITHMETIC IS PART OF THE CONTRACT.  For an observation row x[0..D), D = obs_dim, padding columns
 * included as they stand:
 *
 *   layer(W, b, x)[j]: y = b[j]; for k = 0 .. in-1 (ascending): y = fmaf(W[j][k], x[k], y)   (f32, one rounding per k)
 *   relu(y) = y > 0.0f ? y : 0.0f                                                            (NaN and -0.0f give +0.0f)
 *   h1 = relu(layer(W0, b0, x)); h2 = relu(layer(W1, b1, h1)) (skipped with one hidden layer); mu = layer(W_last, b_last, h)
 *   MEV_POLICY_HIDDEN_TANH: tanh_c in relu's place in h1 and h2.  MEV_POLICY_OUT_TANH: then mu[k] = tanh_c(mu[k]).
 *   mean_seq holds that mu (the squashed mean), the noise and the clamp below follow unchanged (TD3's exploration
 *   rule), and the value head (mev_policy_set_value_head) reads h_last after the hidden activation and is never squashed.
 *   action[k] = fminf(fmaxf(sigma ? mu[k] + sigma[k] * eps[k] : mu[k], lo[k]), hi[k])        (multiply, then add: no FMA here)
 *
 * tanh_c(y) is a tanh DEFINED AS ARITHMETIC -- no libm or device tanhf / expf, whose last bits differ between
 * machines -- every operation f32 with one rounding, `/` the correctly rounded divide, fmaf a fused multiply-add
 * (csrc/mev_act.h is this text as code; mev_tanh runs it on the host):
 *
 *   a  = |y|;  ac = a < 10.0f ? a : 10.0f                       (NaN gives 10)
 *   s  = ac * ac
 *   q  = fmaf(s, fmaf(s, fmaf(s, fmaf(s, Q4, Q3), Q2), Q1), Q0)
 *   p  = fmaf(ac * s, q, ac)
 *   x  = ac + ac;  n = rintf(x * LOG2E)                          (to nearest, ties to even)
 *   r  = fmaf(-n, LN2_LO, fmaf(-n, LN2_HI, x))
 *   g  = fmaf(r, fmaf(r, fmaf(r, fmaf(r, G4, G3), G2), G1), G0)
 *   E  = fmaf(r, fmaf(r, g, 1.0f), 1.0f) * 2^n                   (2^n the float with the bits (n + 127) << 23)
 *   t  = 1.0f - 2.0f / (E + 1.0f)
 *   m  = a < 0x1p-12f ? a : a < 0.5625f ? p : t
 *   tanh_c(y) = y != y ? +0.0f : m with y's sign bit
 *
 *   Q0..Q4 = -0x1.555554p-2f, 0x1.110fbap-3f, -0x1.b9915ep-5f, 0x1.5c6c6p-6f, -0x1.abecbp-8f
 *   LOG2E = 0x1.715476p+0f, LN2_HI = 0x1.62e4p-1f, LN2_LO = 0x1.7f7d1cp-20f
 *   G0..G4 = 0x1p-1f, 0x1.5554dcp-3f, 0x1.5554e8p-5f, 0x1.120c74p-7f, 0x1.6d445ep-10f
 *
 * So tanh_c(-y) has the bits of -tanh_c(y); +-0 and subnormals come back as they are; |tanh_c| <= 1, exactly 1 from
 * |y| = 9.02 on, +-inf included; NaN gives +0.0f, as the ReLU does; and tanh_c does not decrease across any pair of
 * adjacent floats.  Measured over EVERY finite float against tanh in double, in ulp of the result: at most 0.333
 * below 2^-12, 0.814 in the polynomial region, 1.537 in the exponential region (just above 0.5625), 0.500 from 8
 * on (tests/native/tanh_check.cpp exhaustive; the test suite asserts 1, 1, 2, 1 on a strided sweep).
 * Measured (python tools/bench_rollout_act.py -> profiles/rollout_act_sweep.json; the method above): 4096
 * envs x 8 agents x 64 beams, 95-64-64-2, T = 16: the tanh-hidden policy 0.975 ms (0.975-0.977) against 1.413 ms
 * (1.412-1.419) for an eager torch forward of the Tanh module, a clamp and mev_step per sub-step, and 0.933 ms for the
 * ReLU policy: 2.6 us per sub-step for 16 tanh_c per lane (47 VALU instructions each; estimated 1.3-5 us); the
 * output tanh is not measurable.  T = 64: 3.799 against 5.687 ms; 64 envs: 0.582 against 1.407 ms.  All gains beyond
 * the blocks' spreads.  ReLU policies run their own instantiations: against the parent commit in the same session the
 * flagship mev_rollout_policy_repeat row ties (0.7835 / 0.7834 ms); the plain call is +0.14 % at T = 16 (beyond the
 * spreads), a tie at T = 64 and -0.36 % at 64 envs.
 *
 * eps is mev_sample_plans' noise word for word: Philox4x32-10 with key noise_seed and counter
 * (lo32(noise_counter), hi32(noise_counter), e * 64 + i, t) -- the env index e in the candidate's place,
 * t the 0-based sub-step -- eps[0] from words 0, 1 and eps[1] from words 2, 3.  With sigma == NULL no
 * noise word is drawn.  The FMA chain is this library's one exception to its no-FMA rule (that rule
 * matches the reference's SSE build; the policy has no reference counterpart); gfx950 keeps f32
 * subnormals, so the chain is the same bits as a host loop over fmaf.  The action is computed for every
 * agent slot, alive or not, from the row as it stands.
 *
 * mev_rollout_policy is defined, per env and bit for bit, as this loop, obs_0 being the rows
 * mev_get_outputs would return before the call:
 *
 *   for t = 0 .. T-1:
 *       a_t = policy(obs_t)                                            (every agent of the env)
 *       r   = mev_step(actions = a_t, dt, spawn_route[t], flags)       (exactly mev_step, MEV_AUTO_RESET included)
 *       obs_{t+1} = r.obs;  row t of every *_seq array = r's outputs / a_t / mu_t
 *
 * All T sub-steps run for every env: nothing stops at an episode's end.  With MEV_AUTO_RESET an env that
 * ended is reset before its next sub-step, as mev_step does, so its first action after the reset is
 * computed from the terminal observation, as in the host loop.  The Philox spawner and the reset route
 * draw use the handle's counter + t, and the counter advances by T.  Afterwards the handle is exactly
 * where the T mev_step calls would have left it: state and car sizes, pending-reset flags, the last
 * outputs (mev_get_outputs, mev_device_outputs, DLPack, snapshots), the Philox counter and the NPC
 * diagnostics.  With device pointers the last outputs are row T-1 of the caller's *_seq arrays where
 * given (keep them allocated, as after mev_step).  Every element of every given *_seq array is written.
 * A resident step server is stopped first; the NPC-aware deal restarts afterwards (inside the call the
 * envs run in the identity order); mev_kernel_timing does not count the call.  Host pointers are staged
 * and the call is synchronous; device pointers do not synchronise.
 *
 * Supported shapes: every shape the fused kernel can hold (what mev_set_step_kernel(2) accepts) with
 * obs_dim <= 31 + 128; handles with a written beam list or per-car sizes included (the latter run the
 * runtime layout; mev_get_rollout_row).  Anything else is MEV_E_INVALID: there is no slower fallback.
 * Errors (MEV_E_INVALID, the handle untouched): a null policy or one of another handle, in_dim !=
 * obs_dim, length outside 1..MEV_MAX_ROLLOUT, MEV_GATHER_TO_ROOT or an unknown flag, a non-finite bound
 * or sigma, lo[k] > hi[k], an unsupported shape.
 * Measured (python tools/bench_rollout.py -> profiles/rollout_sweep.json; mev_evaluate_plans' method):
 * device pointers, auto-reset, every *_seq output, medians of five blocks (min-max), against (b) the loop a user
 * runs without the call -- an eager torch nn.Sequential forward, a clamp and mev_step per sub-step into the same
 * tensors -- and (c) T x mev_step alone on ready-made actions.  4096 envs x 8 agents x 64 beams, policy 95-64-64-2:
 * a rollout of T = 16 takes 0.943 ms (0.942-0.944), 58.9 us per sub-step, against (b) 1.528 ms (1.525-1.557) and
 * (c) 0.422 ms; T = 64: 3.670 (3.666-3.676) against 6.115 (6.057-6.218) and 1.683 ms -- below (b) by more than the
 * blocks' spreads, 1.6x, with the policy costing 31-33 us per sub-step inside the kernel where the step itself is
 * 26 us (the estimate was a third of the step; supposed, not profiled: its LDS broadcasts and spilled registers,
 * not its FMAs, set the pace).  64 envs: 0.547 against 1.527 ms, 2.8x.  The runtime-layout row at 4096 x 8 x 64 (per-car sizes): 1.120
 * against 1.526 ms; the compile-time row is 11 us per sub-step faster than it.  It LOSES with the wider policy
 * 95-128-128-2 -- 2.315 ms (2.307-2.320) against (b) 1.559 at T = 16, 9.233 against 6.197 ms at T = 64: the framework's
 * GEMM wins there -- and at 4096 envs x 1 agent with traffic, 1.745 (1.708-1.763) against 1.526 ms: the call runs
 * one wave per env where mev_step runs the early split, and a wave's policy pass costs the same for 1 agent as for 8. */
#define MEV_POLICY_MAX_WIDTH 128
typedef struct mev_policy mev_policy;
typedef struct {
    int32_t in_dim;          /* must equal the handle's obs_dim */
    int32_t hidden[2];       /* widths 1..MEV_POLICY_MAX_WIDTH; hidden[1] == 0: one hidden layer */
    const float* w[3];       /* layer l: row-major [out][in] */
    const float* b[3];       /* [out]; the last used layer has out = 2 (throttle, steer) */
} mev_policy_spec;
#define MEV_POLICY_HIDDEN_TANH 0x10u /* mev_policy_create: every hidden layer applies tanh_c, not the ReLU */
#define MEV_POLICY_OUT_TANH    0x20u /* mev_policy_create: mu[k] = tanh_c(mu[k]) before noise and clamp  */
int mev_policy_create(mev_handle* h, const mev_policy_spec* spec, uint32_t flags, mev_policy** out);
int mev_policy_update(mev_policy* p, const mev_policy_spec* spec, uint32_t flags);
/* *flags = the policy's MEV_POLICY_HIDDEN_TANH | MEV_POLICY_OUT_TANH bits (0: the ReLU policy with a raw mu) */
int mev_policy_get_activations(const mev_policy* p, uint32_t* flags);
int mev_policy_destroy(mev_policy* p);

#define MEV_MAX_ROLLOUT 1024
typedef struct {
    const mev_policy* policy;
    int32_t length;                 /* T, 1..MEV_MAX_ROLLOUT */
    float dt;
    const int32_t* spawn_route;     /* optional [T][E], as mev_step_sequence's */
    const float* sigma;             /* optional [2], host, read by value like dt; NULL: deterministic */
    float lo[2], hi[2];             /* finite, lo <= hi */
    uint64_t noise_seed, noise_counter;
    float* obs_seq;                 /* optional [T][E][N][obs_dim]: the observation AFTER sub-step t */
    float* actions_seq;             /* optional [T][E][N][2]: the actions sub-step t ran */
    float* mean_seq;                /* optional [T][E][N][2]: mu before noise and clamp */
    float* reward_seq;              /* optional [T][E][N] */
    uint8_t *done_seq, *status_seq; /* optional [T][E][N] */
    uint8_t *terminated_seq, *truncated_seq; /* optional [T][E] */
    uint32_t flags;                 /* MEV_DEVICE_PTRS | MEV_AUTO_RESET */
} mev_rollout_args;
int mev_rollout_policy(mev_handle* h, const mev_rollout_args* args);
/* The row of k_rollout's instantiation table (MEV_ROLLOUT_KERNELS, csrc/mev_plan.h) that
 * mev_rollout_policy runs for this handle: 0 the runtime layout without traffic, 1 / 2 the traffic
 * layouts of <= 32 / 64 NPC slots, 3 the compile-time row of 8 agents x 64 beams; -1 where the call is
 * not supported. */
int mev_get_rollout_row(const mev_handle* h, int32_t* row);

/* Actor-critic rollouts: a value head on the policy's trunk, and the advantages on the device.
 *
 * value head of a policy: v = layer(wv, bv, h_last)[0], the same FMA chain as every other layer
 * (y = bv[0]; for k ascending: y = fmaf(wv[k], h_last[k], y)); wv [H_last], bv [1], h_last the last hidden
 * layer's activations after the ReLU.  wv == NULL detaches the head.  flags / validation / stream order
 * exactly as mev_policy_update: host pointers are checked finite and the call is synchronous, device
 * pointers are read by a small kernel on the handle's stream.  mev_policy_update leaves an attached head
 * as it is; a new policy has none.
 *
 * mev_rollout_policy_values is mev_rollout_policy -- every output of `rollout`, the handle's state, last
 * outputs, Philox counter and NPC diagnostics bit for bit the same for the same arguments -- that also
 * writes value_seq [T+1][E][N]: row t = V(obs_t), obs_0 being the rows mev_get_outputs returns before the
 * call and obs_{t+1} the observation after sub-step t.  The value is computed for every agent slot, alive
 * or not, from the row as it stands, like the action.  Row t + 1 of an env that ended at t is the value of
 * the TERMINAL observation (the next action is computed from that same row; with MEV_AUTO_RESET the reset
 * happens inside sub-step t + 1).  Row T costs one more pass of the hidden layers after the last sub-step,
 * with no step and no noise word.  With obs_seq NULL the rows are read from the handle's buffer in place.
 * Every element of value_seq is written.  Host pointers are staged and the call is synchronous; device
 * pointers do not synchronise.  Errors (MEV_E_INVALID, the handle untouched): a null value_seq, a policy
 * without a value head, and everything mev_rollout_policy refuses. */
int mev_policy_set_value_head(mev_policy* p, const float* wv, const float* bv, uint32_t flags);
int mev_policy_has_value_head(const mev_policy* p, int32_t* has);

typedef struct {
    mev_rollout_args rollout;   /* exactly as mev_rollout_policy */
    float* value_seq;           /* required, [T+1][E][N]: row t = V(obs_t); obs_0 = the rows mev_get_outputs
                                   returns before the call, obs_{t+1} = the observation after sub-step t */
} mev_rollout_values_args;
int mev_rollout_policy_values(mev_handle* h, const mev_rollout_values_args* args);

/* mev_rollout_policy_repeat: closed-loop rollouts with frame skip -- T DECISIONS in one launch, each one policy
 * pass and then mev_step_repeat with that action held for up to n = repeat sub-steps.  It is defined, per env and
 * bit for bit, as this loop, obs_0 being the rows mev_get_outputs would return before the call:
 *
 *   for t = 0 .. T-1:
 *       a_t = policy(obs_t)                    (the stated FMA chains; noise word index t = the DECISION index,
 *                                               counter (lo32, hi32, e * 64 + i, t); value_seq[t] = V(obs_t) if asked)
 *       r   = mev_step_repeat(actions = a_t, repeat = n, dt, spawn_route rows [t][0..n), flags)
 *                                              (exactly mev_step_repeat: reward summed in f32 in sub-step order, done
 *                                               latched, status latched at the latest done else sub-step k's,
 *                                               terminated / truncated of sub-step k, the env stopping at its first
 *                                               ended sub-step, MEV_AUTO_RESET only at the decision's first sub-step)
 *       obs_{t+1} = r.obs                      (head and ONE LiDAR cast, from the state the env stopped at)
 *       row t of obs_seq / reward_seq / done_seq / status_seq / terminated_seq / truncated_seq = r's outputs
 *       row t of actions_seq / mean_seq = a_t / mu_t;   substeps_seq[t][e] = r.substeps[e]
 *   value_seq[T] = V(obs_T)                    (if asked: one more trunk pass, no noise word, no step)
 *
 * Every *_seq row is one decision; rollout.spawn_route, if given, is [T][repeat][E].  Sub-step s of decision t
 * uses the handle's Philox counter + t * n + s (the NPC spawner), an auto-reset's route draw its decision's first
 * sub-step's counter, and the counter advances by T * n whatever the envs did: mev_step_repeat's rule, T times.
 * Afterwards the handle is exactly where the T mev_step_repeat calls would have left it: state and car sizes,
 * pending-reset flags, the last outputs (with device pointers: row T-1 of the caller's arrays where given), the
 * Philox counter and the NPC diagnostics.  Every element of every given *_seq array is written; a null array
 * leaves that output in the handle's own buffers.  value_seq is optional here (NULL: no value row is computed)
 * and needs a value head.  With repeat = 1 every output equals mev_rollout_policy's bit for bit, and with
 * value_seq mev_rollout_policy_values'.  The actor-critic calls work at the decision level unchanged: value_seq
 * rows are V of the observation each decision was made from, and mev_gae on the summed rewards applies gamma and
 * lambda per decision.
 * Supported shapes, the step-server stop, the identity env order, staging, synchronisation and "not counted by
 * mev_kernel_timing" are all as mev_rollout_policy: every row for which mev_get_rollout_row is >= 0 runs, with no
 * slower fallback.  Errors (MEV_E_INVALID, the handle untouched): everything mev_rollout_policy refuses, repeat
 * outside 1..MEV_MAX_REPEAT, T * repeat above MEV_MAX_ROLLOUT_SUBSTEPS, a non-null value_seq on a policy without a
 * value head.
 * How it runs: the kernel of mev_rollout_policy with the repeat as a flag of the instantiation;
 * inside a decision each sub-step is a whole fused step without the LiDAR (the state goes through L2 between
 * sub-steps, as in the plain call), and the sub-step the env stops at casts the LiDAR from its own LDS.
 * Estimated beforehand, from other calls' numbers: the policy pass (31-33 us) and the LiDAR once per decision, and
 * 8.4 us for each further sub-step's car part.  Measured (python tools/bench_rollout_repeat.py ->
 * profiles/rollout_repeat_sweep.json; tools/bench_rollout.py's method: device pointers, auto-reset, every
 * *_seq output plus value_seq and substeps_seq, medians of five alternated blocks (min-max)), 4096 envs x 8 agents x 64
 * beams, policy 95-64-64-2 with a value head, T = 16 decisions, (a) the call against (b) what a user runs today for the
 * same semantics -- an eager torch forward, a clamp and mev_step_repeat per decision into the same tensors -- and (c)
 * mev_rollout_policy_values over T * n sub-steps (other semantics, orientation only), ms per call:
 *   n = 1: (a) 0.776 (0.775-0.802)  (b) 1.952 (1.948-1.955)  (c) 0.843      n = 2: (a) 0.992 (0.991-0.993)  (b) 2.044 (2.033-2.114)  (c) 1.649
 *   n = 4: (a) 1.431 (1.430-1.436)  (b) 2.145 (2.140-2.148)  (c) 3.235      n = 8: (a) 2.328 (2.326-2.332)  (b) 2.705 (2.699-2.714)  (c) 6.422
 * -- below (b) by more than both blocks' spreads at every n, 2.5x to 1.16x: a decision costs 48.5 us plus 13.5-13.9 us per
 * further sub-step, where (b) is launch-bound at 122-134 us per decision up to n = 4.  The estimate of the further
 * sub-step was low by 5 us: each one is a whole fused step without the LiDAR -- the state's round trip through L2 and an
 * observation head that the next sub-step overwrites included -- not k_cars_repeat's looped car part.  64 envs, n = 4:
 * 0.911 against 2.054 ms.  The runtime-layout row (one car 55 x 24), n = 4: 1.591 against 2.096 ms.  It LOSES at 4096 envs
 * x 1 agent with traffic 0.5, n = 4: 4.220 (3.993-4.387) against 3.221 ms (3.140-3.329) -- as mev_rollout_policy loses there
 * (above): one wave per env, and a wave's policy pass costs the same for 1 agent as for 8.
 * A first version with the sub-steps as a loop INSIDE the loop of decisions was
 * bit-exact and slower throughout (n = 1: 1.187 ms, n = 4: 1.994 ms, a tie with (b), n = 8: 3.120 ms, a loss): its kernels
 * spilt 236 VGPRs where the flat loop's spill 105 (profiles/rollout_repeat_sweep_nested.json).  The existing calls are
 * unchanged: their kernels keep the parent's register figures to the byte, and mev_rollout_policy's first row took
 * 0.944 / 0.941 ms on this build against 0.941 / 0.942 ms on the commit before it in one session (two alternated pairs of
 * processes; each block's spread is 0.001 ms, so the processes differ by more than the blocks, in both directions);
 * bench.py's config 3 1.2747 / 1.2750 against 1.2743 / 1.2728 G agent-steps/s. */
#define MEV_MAX_ROLLOUT_SUBSTEPS 4096   /* T * repeat of one launch: at the measured <= 60 us per sub-step about 0.25 s */
typedef struct {
    mev_rollout_args rollout;  /* as mev_rollout_policy, except: every *_seq row is one DECISION (above);
                                  rollout.spawn_route, if given, is [T][repeat][E] */
    float*   value_seq;        /* optional [T+1][E][N], as mev_rollout_policy_values'; needs a value head */
    int32_t  repeat;           /* n, 1..MEV_MAX_REPEAT; T * n <= MEV_MAX_ROLLOUT_SUBSTEPS */
    int32_t* substeps_seq;     /* optional [T][E]: sub-steps decision t ran in env e */
} mev_rollout_repeat_args;
int mev_rollout_policy_repeat(mev_handle* h, const mev_rollout_repeat_args* args);

/* mev_rollout_policies: a policy per agent slot in one rollout -- self-play against frozen copies, a population
 * with a policy per env, cross-play of two checkpoints, independent learners.  It is mev_rollout_policy_repeat's
 * defining loop (above) with one line changed: agent slot (e, i) is driven by policies[assign[e][i]],
 *
 *   a_t[e][i], mu_t[e][i] = policy_p(obs_t[e][i]),  p = assign[e][i]       (the stated FMA chains, that policy's own layers)
 *   action[k] = fminf(fmaxf(sigma ? mu[k] + sigma[p][k] * eps[k] : mu[k], lo[k]), hi[k])    (multiply, then add)
 *   value_seq[t][e][i] = V_p(obs_t[e][i])                                   (if asked; row T included)
 *
 * The noise word is unchanged -- counter (lo32, hi32, e * 64 + i, t), t the decision -- and does not depend on p.
 * Everything else is mev_rollout_policy_repeat's, word for word: `repeat` with its summed, latched rows and
 * substeps_seq, spawn_route as [T][repeat][E], the Philox counter advancing by T * n, auto-reset at a decision's first
 * sub-step, every element of every given *_seq array written, the handle left exactly where T mev_step_repeat calls
 * would leave it.  The assignment belongs to the SLOT (e, i): it holds for the whole call, across respawns and
 * auto-resets.  The policies may differ in depth and widths (one or two hidden layers, 1..128 units each).  With
 * count == 1 and assign all zero every output equals mev_rollout_policy_repeat's bit for bit; with repeat == 1 also
 * the plain calls'.
 * `policies` and `sigma` are ALWAYS host arrays, read before the call returns (sigma by value, like dt; NULL: no
 * noise word is drawn); `assign` is a host or a device array as base.rollout.flags says and is staged like every
 * host-mode array.  Host pointers: an assign entry >= count -> MEV_E_RANGE, nothing changed; synchronous.  Device
 * pointers: such an entry is read as count - 1; not synchronous.  Supported shapes, the step-server stop and "not
 * counted by mev_kernel_timing" as mev_rollout_policy; the LDS scratch is sized by the largest sum of hidden widths
 * among the listed policies.
 * Errors (MEV_E_INVALID, the handle untouched): everything mev_rollout_policy_repeat refuses; a non-NULL
 * base.rollout.policy or base.rollout.sigma; null policies or assign; count outside 1..MEV_MAX_ROLLOUT_POLICIES; a
 * null entry, an entry of another handle or one whose in_dim != obs_dim; a non-finite sigma value; value_seq given
 * while a listed policy has no value head; a shape for which mev_get_rollout_row is negative.
 * How it runs: k_rollout's flat frame-skip loop with one more flag of the instantiation.  Per group
 * of up to 8 agents the observation rows are staged in LDS once; then, for each policy that at least one agent of
 * the group has (a wave-uniform test), the single-policy chains run for the whole group with that policy's layers
 * and only its own agents' lanes store.  The cost is one policy pass per DISTINCT policy present in a group: a
 * per-env assignment costs what one policy costs.
 * Estimated beforehand (supposed, not measured): one policy pass of 31-33 us per distinct policy present in an env on
 * top of the step, so that eight policies in one env might lose.  Measured (python tools/bench_rollout_multi.py ->
 * profiles/rollout_multi_sweep.json; tools/bench_rollout_repeat.py's method: device pointers,
 * auto-reset, every *_seq output plus value_seq and substeps_seq, medians of five alternated blocks (min-max)), 4096
 * envs x 8 agents x 64 beams, policies 95-64-64-2 with value heads, T = 16 decisions, (a) the call against (b) what a
 * user runs today for the same semantics -- an eager torch forward of each of the P policies over all rows, a gather
 * by assign, a clamp and mev_step_repeat per decision into the same tensors -- and (c) mev_rollout_policy_repeat with
 * one policy (orientation only), ms per call at n = 1 / n = 4:
 *   P = 1:                      (a) 0.819 / 1.506  (b) 2.272 / 2.333   (c) 0.795 / 1.437
 *   P = 2, 4 / 4 in every env:  (a) 1.083 / 1.749  (b) 3.798 / 3.823   (c) 0.808 / 1.443
 *   P = 2 by env parity:        (a) 0.819 / 1.509  (b) 4.088 / 4.027   (c) 0.807 / 1.447
 *   P = 8, one per agent:       (a) 2.738 / 3.356  (b) 13.102 / 13.166 (c) 0.807 / 1.461
 * and 64 envs, 4 / 4, n = 4: (a) 1.135 (b) 3.814 -- (a) below (b) by more than both blocks' spreads at all nine
 * points, no loss.  A further distinct policy in an env costs 17-19 us per decision, not 31-33: the rows are staged
 * once per group (supposed from the structure, not profiled).  The existing calls are unchanged: their kernels keep
 * the parent's register figures to the byte, and mev_rollout_policy_repeat's first row took 0.781 / 0.781 ms on this
 * build against 0.780 / 0.780 ms on the commit before it in one session (a block's spread is 0.002-0.003 ms). */
#define MEV_MAX_ROLLOUT_POLICIES 8
typedef struct {
    mev_rollout_repeat_args base;       /* exactly as mev_rollout_policy_repeat, except:
                                           base.rollout.policy and base.rollout.sigma must be NULL */
    const mev_policy* const* policies;  /* [count]; ALWAYS a host array, read before the call returns */
    int32_t count;                      /* P, 1..MEV_MAX_ROLLOUT_POLICIES */
    const uint8_t* assign;              /* [E][N]: agent slot (e, i) is driven by policies[assign[e][i]];
                                           host or device as base.rollout.flags says */
    const float* sigma;                 /* optional [P][2]; ALWAYS host, by value like dt; NULL: no noise word drawn */
} mev_rollout_multi_args;
int mev_rollout_policies(mev_handle* h, const mev_rollout_multi_args* args);

/* mev_gae: generalised advantage estimation over a rollout's arrays, one reverse scan on the device.
 * THE ARITHMETIC IS THE CONTRACT: f32, multiply, then add, no FMA, per (e, i) and for t descending, with
 * c the f32 product gamma * lambda, computed once:
 *
 *   stop  = done[t][e][i] | terminated[t][e]                       (absent arrays read as 0)
 *   cut   = stop | truncated[t][e]
 *   nv    = stop ? 0.0f : V[t+1]
 *   delta = (r[t] + gamma * nv) - V[t]
 *   adv   = cut ? delta : delta + c * adv_next                     (adv_next of t = T-1 is 0.0f)
 *   masked (MEV_GAE_MASK_RESET_STEPS, and (t > 0 ? terminated[t-1][e] | truncated[t-1][e]
 *                                                : ended_before ? ended_before[e] : 0)):
 *           adv = 0.0f, valid = 0      (its predecessor is cut anyway, so nothing flows through it)
 *   ret   = adv + V[t];  adv_next = adv
 *
 * Truncation bootstraps from V[t+1] -- the value of the terminal observation, which is what
 * mev_rollout_policy_values writes there -- and cuts the trace; termination and an agent's own done (a
 * per-agent end inside a running env, a respawn in the same step included) do neither.  The masked rows
 * are this library's auto-reset steps: the env ended at t - 1, so the action of t was computed from the
 * terminal observation and the step ran on the reset env; such a transition belongs to no episode, and
 * `valid` tells a loss which rows to leave out.  ended_before says the same of row 0: the env's
 * terminated | truncated of the step before the window.
 * Like mev_update_plans the call reads and writes only its arguments; the handle supplies E, N, the device
 * and the stream, and a resident step server is stopped first.  Host pointers are staged and the call is
 * synchronous; device pointers do not synchronise.  Errors (MEV_E_INVALID): null rewards or values, no
 * output pointer at all, length outside 1..MEV_MAX_ROLLOUT, a non-finite gamma or lambda, an unknown flag.
 * Measured (python tools/bench_actor_critic.py -> profiles/actor_critic_sweep.json; tools/bench_rollout.py's
 * method: device pointers, auto-reset, medians of five blocks (min-max)), 4096 envs x 8 agents x 64 beams, policy
 * 95-64-64-2 with a value head: (a) mev_rollout_policy_values, T = 16, 0.890 ms (0.883-0.891) against (b)
 * mev_rollout_policy on the same build 0.945 ms (0.944-0.945): the value instantiation is FASTER than the plain one, by
 * 3.4 us per sub-step (T = 64: 3.404 against 3.688 ms) -- not because a third chain is free but because its kernel spills
 * 132 VGPRs where the plain one spills 185 (the code object; why the allocator does better is supposed, not profiled) --
 * where (c) an eager torch forward of trunk + head over the (T + 1) E N observation rows takes 0.357 ms (0.357-0.367;
 * T = 64: 1.324 ms).  64 envs: (a) 0.537, (b) 0.553, (c) 0.164 ms.  (d) mev_gae takes 0.011 ms (0.011-0.011) at T = 16
 * and 0.027 ms at T = 64 against (e) the eager torch GAE loop's 1.384 ms (1.379-1.393) and 5.344 ms: 128x and 197x; 64
 * envs 0.007 against 1.257 ms.  All beyond the blocks' spreads.  mev_rollout_policy itself is unchanged: its kernels are a
 * template instantiation of their own with the parent's register figures, 0.937 ms (0.936-0.937) on this build against
 * 0.937 ms (0.937-0.938) on the commit before it, same session. */
#define MEV_GAE_MASK_RESET_STEPS 0x100u
typedef struct {
    const float* reward_seq;        /* [T][E][N] */
    const float* value_seq;         /* [T+1][E][N] */
    const uint8_t* done_seq;        /* optional [T][E][N] */
    const uint8_t* terminated_seq;  /* optional [T][E] */
    const uint8_t* truncated_seq;   /* optional [T][E] */
    const uint8_t* ended_before;    /* optional [E]: the env's last step BEFORE the window ended (MASK flag) */
    int32_t length;                 /* T, 1..MEV_MAX_ROLLOUT */
    float gamma, lambda;            /* finite */
    float* advantages;              /* optional [T][E][N] */
    float* returns;                 /* optional [T][E][N]: advantages + value_seq[t] */
    uint8_t* valid;                 /* optional [T][E][N]: 0 for a masked transition, else 1 */
    uint32_t flags;                 /* MEV_DEVICE_PTRS | MEV_GAE_MASK_RESET_STEPS */
} mev_gae_args;
int mev_gae(mev_handle* h, const mev_gae_args* args);

/* Outputs of the last step / reset, from the handle's own device buffers.
 * Lifetime: after a step that wrote caller-owned output buffers (device
 * pointers in mev_step_args), this call, mev_device_outputs and
 * mev_output_dlpack read those buffers -- keep them allocated and unmodified
 * until the next mev_step / mev_reset of the handle (or read the outputs from
 * them directly). */
int mev_get_outputs(mev_handle* h, float* obs, float* reward, uint8_t* done, uint8_t* status,
                    uint8_t* terminated, uint8_t* truncated, int32_t* agents_alive, int32_t* step,
                    uint32_t flags);

/* State snapshot / restore (host pointers).  mev_set_state recomputes the
 * observation with LiDAR = 1.0, as after a reset. */
int mev_get_state(mev_handle* h, const mev_state* out);
int mev_set_state(mev_handle* h, const mev_state* in);

/* Device pointers of the handle's internal output buffers (zero-copy consumers),
 * holding the last step's / reset's outputs: a step that wrote elsewhere (caller
 * buffers, the pinned block of a small host-mode step, a packed gather row) is
 * first copied into them on the handle's stream (caller buffers must still be
 * valid then: see mev_get_outputs).  Device-mode steps without output pointers
 * write them in place. */
int mev_device_outputs(mev_handle* h, float** obs, float** reward, uint8_t** done, uint8_t** status,
                       uint8_t** terminated, uint8_t** truncated);

/* Route randomisation at reset (the reference's test.py draws
 * a random route from the mapping on every reset, test.py:36-39,118-119): with
 * count > 0, every reset -- mev_reset and the MEV_AUTO_RESET of mev_step --
 * draws each agent's route uniformly from routes[0..count) (Philox keyed by the
 * handle seed, the reset counter, env and agent).  count = 0 restores fixed
 * routes (mev_set_ego_routes), the reference env.py behaviour. */
int mev_set_reset_routes(mev_handle* h, const int32_t* routes, int32_t count);

/* Device snapshots for batched rollbacks (EnvState +
 * get_state/set_state, reference cpp/EnvState.h:9-15, IntersectionEnv.cpp:394-416):
 * the whole state of every env plus the last step's outputs, in one
 * self-describing buffer of mev_snapshot_size bytes.  With MEV_DEVICE_PTRS the
 * buffer (and env_mask) live on the handle's device and the copies are
 * device-to-device.  mev_restore restores every env (env_mask NULL; also the
 * handle's Philox counter) or only the envs with env_mask[e] != 0; afterwards
 * mev_get_outputs returns the snapshot's outputs.  The car sizes (mev_set_car_dims)
 * are part of the state.  A snapshot restores only into a handle of the same shape
 * whose route table begins with the snapshot handle's routes (mev_add_route, same
 * paths in the same order); otherwise MEV_E_INVALID and the handle is unchanged. */
int mev_snapshot_size(mev_handle* h, uint64_t* bytes);
int mev_snapshot(mev_handle* h, void* dst, uint32_t flags);
int mev_restore(mev_handle* h, const void* src, const uint8_t* env_mask, uint32_t flags);
/* Branching from a snapshot (a planner fans one root env out into E candidates):
 * env e takes the state, car sizes and last outputs of the SNAPSHOT's env env_map[e]; env_map[e] == -1 leaves
 * env e as it is.  [E] int32, host or (MEV_DEVICE_PTRS) device, like src.  Same validation as mev_restore.
 * Host pointers: an entry outside [-1, E) -> MEV_E_RANGE, the handle unchanged.  Device pointers: such an
 * entry is treated as -1 (the kernel never reads outside the snapshot).  The handle's Philox counter is not
 * restored (as with env_mask).  The reset route pool (mev_set_reset_routes) is configuration, not state, and
 * stays the handle's; a car's fixed route (mev_set_ego_routes) is its `route` state field, which a later reset
 * reuses, so a copy keeps its source's routes (as after a masked mev_restore or mev_set_state).
 * The on-device spawner is keyed by env index, so two copies of one env
 * draw different NPC spawns unless the caller replays spawn_route.  The source is the snapshot buffer, never
 * the live state: any map, a permutation included, is safe.
 * Measured (profiles/sequence_sweep.json): 59.1 us per call at 4096 envs x 8 agents with device pointers,
 * level with a masked mev_restore (58.9 us; both include reading the snapshot header back to the host). */
int mev_restore_map(mev_handle* h, const void* src, const int32_t* env_map, uint32_t flags);

/* Diagnostics (cumulative): route ids in state-format gather messages this handle's route
 * table does not have (mev_unpack_gathered; their rows' look-ahead terms are NaN).
 * mev_comm_init already refuses ranks whose route tables differ. */
int mev_decode_errors(mev_handle* h, int64_t* count);
/* Diagnostics: spawns dropped because max_npcs was full (cumulative). */
int mev_npc_overflow(mev_handle* h, int64_t* count);
/* Diagnostics (cumulative): the spawn overflow above, and the NPC turns the
 * controller ran one after another because its parallel rounds disagreed
 * (mev_kernels.hip npc_phase: round B changed a throttle; results are the
 * sequential ones either way). */
int mev_npc_stats(mev_handle* h, int64_t* overflow, int64_t* sequential_turns);
/* Diagnostics: per-env phase timestamps [E][8] of the last step; all zero
 * unless the library was built with -DMEV_STAMPS (tools/phase_profile.py). */
int mev_debug_stamps(mev_handle* h, uint64_t* out);
/* Measurement: with timing enabled (every = n > 0), every n-th mev_step
 * records HIP events on the handle's stream before k_cars, between k_cars and
 * k_lidar, and after k_lidar (every = 0 disables).  mev_kernel_times returns
 * the summed device durations (ms) of the two kernels over the timed steps
 * and their count since the previous call (or since enabling), then clears
 * them; it waits for the recorded steps to finish.  With the fused step kernel
 * (mev_set_step_kernel) cars_ms holds k_step's duration and lidar_ms is 0. */
int mev_kernel_timing(mev_handle* h, int32_t every);
int mev_kernel_times(mev_handle* h, double* cars_ms, double* lidar_ms, int64_t* steps);
/* Scheduling (results are identical either way): which kernels run a step.
 * 1 = k_cars (one wave per env) then k_lidar (one wave per group of agents),
 * with the obstacle table handed over through HBM; 2 = the fused k_step, one
 * wave per env running both parts back to back from its LDS; 0 = automatic
 * (fused when its LDS -- car tables, NPC slots in traffic mode, one LiDAR pool
 * -- fits a wave's 10 KB share at 4 waves per SIMD, and E >= 1024 or an env's
 * beams fit one LiDAR group (N * R <= 256) or, without traffic, N <= 8 agents
 * and R <= 128 beams).  Asked for
 * explicitly, the fused kernel runs whenever that LDS fits one workgroup
 * (64 KB); otherwise the call fails with MEV_E_INVALID.  mev_get_step_kernel returns the kernel
 * the next step will use (1 or 2).  Replaces nothing in the reference (its
 * step is one sequential loop, cpp/IntersectionEnv.cpp:133-392). */
int mev_set_step_kernel(mev_handle* h, int32_t kernel);
int mev_get_step_kernel(const mev_handle* h, int32_t* kernel);
/* Scheduling (results are identical either way): envs per fused k_step wave.
 * With few agents per env (N <= 4, no traffic) 2, 4 or 8 envs share a wave's
 * 64 lanes (8 agent slots), so one wave's latency chain steps them all.
 * 0 = automatic; a request is reduced to fit N * envs <= 8.  mev_get_step_pack
 * returns what the next step uses (1 on the two-kernel path).  Replaces
 * nothing in the reference (one env per IntersectionEnv object). */
int mev_set_step_pack(mev_handle* h, int32_t envs_per_wave);
int mev_get_step_pack(const mev_handle* h, int32_t* envs_per_wave);
/* Scheduling (results are identical either way): two waves per fused k_step
 * workgroup -- the car part, then the LiDAR in one wave beside the rest of the
 * car part (rewards, flags, observation head) in the other.  0 = automatic (on
 * when the batch needs <= 2048 workgroups, i.e. <= 4 waves per SIMD, no traffic),
 * 1 = off, 2 = on (no traffic), 3 = early split (no traffic, one env per
 * workgroup, N * R <= 512: the LiDAR wave marches the road from the poses after
 * the kinematics while the car wave resolves collisions).  With traffic, one ego
 * per env, <= 32 NPC slots, R <= 128 and E a multiple of 16, the early split is
 * two envs per workgroup: one wave per env runs the NPC controller and the car
 * logic, one wave runs the two egos' kinematics, status and LiDAR beside them;
 * automatic (mode 0) and by 3.  mev_get_step_split
 * returns 1 (split) or 2 (early split) when the next step uses it.  Replaces
 * nothing in the reference. */
int mev_set_step_split(mev_handle* h, int32_t mode);
int mev_get_step_split(const mev_handle* h, int32_t* split);
/* Which compiled kernel the handle runs (for tests; each pointer may be NULL).
 * step_row: the row of the k_step instantiation table (kStepKeys, csrc/mev_plan.h)
 * that the next launched mev_step into the handle's own output buffers runs, -1
 * on the two-kernel path.  serve_row: the row of k_serve's table (kServeKeys)
 * that the persistent step server runs for this handle, -1 where it does not
 * apply.  tab: 1 when the kernels read the LiDAR's probe distances from a table
 * (lidar_step values whose multiples are not exact), else 0.  A step into a
 * caller's device rows of the same width runs the same row.  Replaces nothing in
 * the reference. */
int mev_get_step_row(const mev_handle* h, int32_t* step_row, int32_t* serve_row, int32_t* tab);
/* Scheduling (results are identical either way): the NPC-aware env deal of the
 * fused traffic k_step -- workgroups take envs heaviest NPC count first, from
 * orders the previous step built.  on: 1 (default; MEV_NO_DEAL=1 in the
 * environment makes 0 the default), 0 = the XCD-aware identity order.  Replaces
 * nothing in the reference. */
int mev_set_env_deal(mev_handle* h, int32_t on);
/* Host-mode steps as a persistent step server (results are identical either
 * way).  A step with host buffers (no MEV_DEVICE_PTRS) of a small handle (<= 64
 * envs, outputs <= 256 KB, the fused kernel, no traffic above one ego / 32 NPC
 * slots) is answered by a kernel that stays resident between steps (k_serve):
 * the host posts the step in a mailbox of pinned memory and the kernel answers
 * once its outputs are there -- a PCIe round trip instead of a kernel launch and
 * a stream synchronisation.  The kernel leaves when no step is posted for its
 * idle limit and is launched again by the next one; every other call on the
 * handle stops it first.  Only on the handle's own stream (not after
 * mev_set_stream); the kernel itself runs on a non-blocking highest-priority
 * stream of its own; at most 2 servers are resident per process (other handles
 * step launched).  A server slot belongs to the handle that took it -- across its
 * server's idle exits and paused stretches -- until the handle is closed, turns
 * serving off, moves to another stream, or has made no host-mode step for 50 ms
 * (and none since the previous step, or the creation, of the asking handle) when
 * another handle asks for a slot; so a round-robin over more small handles than
 * slots serves the first two to step, whatever the timing of idle exits or of
 * pauses of the host between steps.
 * While it is resident, every device-wide wait of the process
 * (hipDeviceSynchronize, torch.cuda.synchronize(), frees that wait for the
 * device) waits for its idle exit, so the idle limit is adaptive: 8 x the
 * moving average of the host's time between an answer and the next post,
 * within [0.2, 2] ms; after 4 consecutive posts that found the server already
 * gone (a device-wide wait or a slow host between steps) the next 1024 host
 * steps are launched instead.  MEV_SERVE_IDLE_MS=n (1..1000) fixes the limit.
 * mode: 0 = off, 1 = automatic (default; MEV_NO_SERVE=1 in the environment
 * turns it off).  mev_serve_stats: steps served, server launches, whether one
 * is running.  Replaces nothing in the reference (its env.py steps one
 * IntersectionEnv per call on the CPU, cpp/bindings.cpp:53-55). */
int mev_set_serve(mev_handle* h, int32_t mode);
int mev_serve_stats(const mev_handle* h, uint64_t* steps, uint64_t* launches, int32_t* running);

/* ---- Multi-GPU: the per-step RCCL gather of the stacked outputs ----------
 * envs are sharded over the GPUs of a node, one process and
 * one handle per GPU, with no communication inside a step; the one collective
 * is a gather of every rank's step outputs to a root rank over xGMI.  The
 * reference has no counterpart (each IntersectionEnv is a single instance,
 * cpp/IntersectionEnv.h:23-105).
 *
 * Packed layout of one rank's outputs (slots = envs per rank, the largest
 * shard; a smaller shard leaves the tail of its slots unused), one contiguous
 * message per rank:
 *   obs f32 [slots][N][D] | reward f32 [slots][N] | done u8 [slots][N] |
 *   status u8 [slots][N] | terminated u8 [slots] | truncated u8 [slots]
 * each field 256-B aligned, the total padded to 256 B.  Host-only (no device). */
#define MEV_GATHER_TO_ROOT 0x4u /* mev_step: write the outputs packed and gather them to the root rank */
#define MEV_COMM_ID_BYTES 128   /* == NCCL_UNIQUE_ID_BYTES */
enum { MEV_PK_OBS = 0, MEV_PK_REWARD, MEV_PK_DONE, MEV_PK_STATUS, MEV_PK_TERMINATED, MEV_PK_TRUNCATED, MEV_PK_COUNT,
       MEV_PK_LIDAR = MEV_PK_COUNT /* compact formats only */, MEV_PK_STATE /* state format only */, MEV_PK_FIELDS };
int mev_packed_layout(int32_t slots, int32_t num_agents, int32_t obs_dim, uint64_t* offsets /*[MEV_PK_COUNT]*/,
                      uint64_t* bytes);
/* Gather formats (mev_set_gather_format, before mev_comm_init):
 *   MEV_GATHER_F32 (default): the layout above, obs rows as the plain step writes them;
 *   MEV_GATHER_LIDAR_U8: obs holds only each row's 31-float head, [slots][N][31], and a
 *     field MEV_PK_LIDAR, u8 [slots][N][lidar_slots], holds one code per beam: 0 no hit
 *     (max_dist), k + 1 a hit at march probe k, 255 a dead agent.  Lossless: the floats
 *     are table[code] (mev_lidar_decode_table, 256 entries), bit-identical to the plain
 *     step's; padding columns beyond 31 + lidar_slots are zero.  At R = 64, N = 8 a row
 *     shrinks from 380 B to 194 B (the message from 12.66 MB to 6.37 MB at 4096 envs).
 *   MEV_GATHER_STATE (no traffic): no observation field at all; the LiDAR codes as in
 *     MEV_GATHER_LIDAR_U8, and a field MEV_PK_STATE with each agent's post-step state
 *     as arrays of n = slots * N: x, y, v, heading f32 | route, path index i16 |
 *     intention, alive u8 (22 B per agent).  get_observations (cpp/IntersectionEnv.cpp:
 *     418-520) is a pure function of that state, so the root rebuilds the 31-float
 *     head with the step's own device code (mev_unpack_gathered), bit-identical to
 *     the plain step's rows.  At R = 64, N = 8 a row is 92 B instead of 380 B (the
 *     message 3.03 MB instead of 12.66 MB at 4096 envs); the ranks also skip the head.
 * mev_packed_layout2: offsets of all MEV_PK_FIELDS fields for any format (fields a
 * format does not use are empty).  Host-only. */
#define MEV_GATHER_F32 0
#define MEV_GATHER_LIDAR_U8 1
#define MEV_GATHER_STATE 2
int mev_packed_layout2(int32_t slots, int32_t num_agents, int32_t obs_dim, int32_t lidar_slots, int32_t format,
                       uint64_t* offsets /*[MEV_PK_FIELDS]*/, uint64_t* bytes);
int mev_set_gather_format(mev_handle* h, int32_t format);
int mev_lidar_decode_table(const mev_handle* h, float* table /*[256]*/);
/* ncclGetUniqueId: called by ONE process (any), then shared with every rank
 * out of band (e.g. a TCP store); id is MEV_COMM_ID_BYTES bytes. */
int mev_comm_unique_id(uint8_t* id);
/* Join the communicator of `world` ranks (ncclCommInitRank on the handle's
 * device; collective: every rank calls it) and allocate the double-buffered
 * packed buffers: two send buffers on a non-root rank, two [world][bytes]
 * gather buffers on the root.  slots = envs per rank of the largest shard
 * (0 = num_envs). */
int mev_comm_init(mev_handle* h, const uint8_t* id, int32_t world, int32_t rank, int32_t root, int32_t slots);
int mev_comm_destroy(mev_handle* h);
/* mev_step with MEV_GATHER_TO_ROOT (the args' obs/reward/done/status/
 * terminated/truncated pointers must be NULL): the step kernel writes this
 * rank's outputs straight into its packed slot (on the root: its row of the
 * gather buffer, no copy), then one grouped ncclSend (non-root) / ncclRecv
 * from every peer (root) runs on the handle's communication stream, ordered
 * after the step by an event, so it overlaps the next step.  Step t and t+2
 * share a buffer: step t+2 waits for gather t.  agents_alive / step still go
 * to the args' pointers (or the handle's own buffers).
 *
 * mev_gather_result (root): the gather buffer of the last gathered step,
 * [world][bytes] in rank order, and makes the handle's stream wait for that
 * gather (stream-ordered consumers on that stream then see every rank's rows).
 * mev_gather_wait: host wait for every gather issued so far, at most
 * timeout_ms (<= 0: no limit); on timeout the communicator is aborted and
 * MEV_E_HIP returned, so a lost peer cannot hang the caller forever. */
int mev_gather_result(mev_handle* h, void** stacked, uint64_t* bytes_per_rank, int32_t* world);
int mev_gather_wait(mev_handle* h, int32_t timeout_ms);
/* Root (any gather format): the float observation rows of a gathered buffer
 * `stacked` (device, [world][bytes] as mev_gather_result returns it, in the
 * handle's gather format and slots) into obs (device, [world][slots][N][D]), on
 * the handle's stream -- the rows each rank's plain step would have written, bit
 * for bit (F32: copied; LIDAR_U8: heads + decoded codes; STATE: heads rebuilt from
 * the shipped state).  Slots beyond a rank's envs hold whatever their (zeroed)
 * message decodes to.  Reward, done, status, terminated and truncated are read
 * from the buffer directly (mev_packed_layout2). */
int mev_unpack_gathered(mev_handle* h, const void* stacked, int32_t world, float* obs);

/* ---- Zero-copy export (DLPack) -----------------------------------------
 * the handle's device output buffers as DLPack tensors for
 * torch-free consumers (and torch.from_dlpack).  The structs below are the
 * DLPack v0.8 ABI (dlpack.h: DLDevice, DLDataType, DLTensor, DLManagedTensor),
 * restated so this header stays self-contained.  The tensor views memory the
 * handle owns: it is valid until mev_destroy; call its deleter when done (it
 * frees only the descriptor). */
typedef struct { int32_t device_type; int32_t device_id; } mev_dl_device; /* kDLROCM = 10 */
typedef struct { uint8_t code; uint8_t bits; uint16_t lanes; } mev_dl_dtype; /* kDLInt 0, kDLUInt 1, kDLFloat 2 */
typedef struct {
    void* data;
    mev_dl_device device;
    int32_t ndim;
    mev_dl_dtype dtype;
    int64_t* shape;
    int64_t* strides; /* NULL = compact row-major */
    uint64_t byte_offset;
} mev_dl_tensor;
typedef struct mev_dl_managed {
    mev_dl_tensor dl_tensor;
    void* manager_ctx;
    void (*deleter)(struct mev_dl_managed* self);
} mev_dl_managed;
enum { MEV_OUT_OBS = 0, MEV_OUT_REWARD, MEV_OUT_DONE, MEV_OUT_STATUS, MEV_OUT_TERMINATED, MEV_OUT_TRUNCATED,
       MEV_OUT_AGENTS_ALIVE, MEV_OUT_STEP, MEV_OUT_GATHERED /* root: [world][bytes] u8 of the last gather */,
       MEV_OUT_COUNT };
/* The handle's internal output buffer `which` (what mev_device_outputs returns,
 * brought up to the last outputs the same way) as a DLPack tensor:
 * obs [E][N][D] f32, reward [E][N] f32, done/status [E][N] u8,
 * terminated/truncated [E] u8, agents_alive/step [E] i32.  MEV_OUT_GATHERED
 * (root): the last gather's buffer; the handle's stream is made to wait for its
 * RCCL receives, as mev_gather_result does. */
int mev_output_dlpack(mev_handle* h, int32_t which, mev_dl_managed** out);

#ifdef __cplusplus
}
#endif

#endif /* MARLENV_H */
