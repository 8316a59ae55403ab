// mev_kernels.h — device-side data layout and kernel launchers of the
// batched intersection environment (gfx950).
//
// HBM layout (structure of arrays; env e, agent i, NPC slot k):
//   ego field f      : f[e*N + i]            (x, y, v, heading, acc, steering, prev_dist,
//                                             prev_a0, prev_a1, spawn_x/y/v/heading: f32;
//                                             path_index, route, intention: i32; alive: u8)
//   npc field f      : f[e*K + k]  K = max_npcs, live slots are a prefix of length npc_count[e]
//   per-env          : step_count, npc_count (i32), pending_reset (u8)
//   outputs          : obs[(e*N + i)*D + c] f32 (D = obs_dim), reward/done/status [e*N+i],
//                      terminated/truncated/agents_alive/step [e]
//   constant tables  : route paths [P*P][160][2] f32 (P = 8L lane points), route intent /
//                      spawn (x, y, heading) / success axis, LiDAR beam offsets [R] f32,
//                      NPC route list [M] i32
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mev_beams.h"
#include "mev_plan.h"
#include "mev_refworld.h"

namespace mev {

// The 4-byte fields of each SoA live in ONE allocation, field k at base +
// k * stride (x first): kernels address them from the x pointer and the stride
// so they hold one base address in SGPRs instead of one pointer per field.
struct EgoSoA {
    float *x, *y, *v, *h, *acc, *steer, *prev_dist, *pa0, *pa1, *sx, *sy, *sv, *sh;
    int32_t *pidx, *route, *intent;
    uint8_t* alive;
    int64_t stride;  // elements between consecutive fields (>= E*N)
};
enum EgoField { EF_X, EF_Y, EF_V, EF_H, EF_ACC, EF_STEER, EF_PREV_DIST, EF_PA0, EF_PA1, EF_SX, EF_SY, EF_SV, EF_SH,
                EF_PIDX, EF_ROUTE, EF_INTENT, EF_COUNT };

struct NpcSoA {
    float *x, *y, *v, *h, *acc, *steer;
    int32_t *pidx, *route, *intent;
    uint8_t* alive;
    int32_t* count;
    int64_t stride;  // elements between consecutive fields (>= E*K)
};
enum NpcField { NF_X, NF_Y, NF_V, NF_H, NF_ACC, NF_STEER, NF_PIDX, NF_ROUTE, NF_INTENT, NF_COUNT };

struct RouteTab {
    const float* path;      // [nroutes][row][2]: plen points, the last segment, zeros (mev_world.h)
    const int32_t* intent;  // [nroutes]
    const float* spawn;     // [nroutes][3]  x, y, heading
    // [nroutes][3] bounding boxes (min x, max x, min y, max y) of each route's three
    // pieces -- points [0, 50), [50, 110), [110, plen) (RouteGen.cpp:160-237) -- for
    // the NPC ghost scan's prefilter
    const float4* pbox;
    const int32_t* len;     // [nroutes] each path's own length (Car.path.size())
    int32_t nroutes;
    int32_t plen;           // points per path in the rows (PATH_LEN, or the longest path rounded up to 16)
    int32_t row;            // points per row (plen + 16; ROUTE_PTS for plen = PATH_LEN)
    int32_t min_len;        // the shortest path's length (an index below it is inside every path)
};

struct Outputs {
    float* obs;
    float* rew;
    uint8_t* done;
    uint8_t* status;
    uint8_t* term;
    uint8_t* trunc;
    int32_t* alive_cnt;
    int32_t* step;
    // floats per observation row in `obs`: D, or OBS_HEAD when lidar_u8 is set (the
    // compact gather format: the LiDAR block goes to lidar_u8 as one code per beam,
    // [E*N][lidar_slots]: 0 = no hit (max_dist), k + 1 = hit at march probe k, 255 =
    // dead agent (0.0); decoded through mev_lidar_decode_table; padding columns
    // beyond 31 + lidar_slots are not written)
    int32_t obs_ld;
    uint8_t* lidar_u8;
    // The state gather format (MEV_GATHER_STATE; obs == nullptr, lidar_u8 set): no
    // observation head is written; instead every agent's post-step state, from which
    // the root rebuilds the head (launch_decode_state), as SoA arrays of state_n
    // elements at `state` (layout: kStateBytesPerAgent).  Agent a = e * N + i.
    uint8_t* state;
    int64_t state_n;
};
// the LiDAR code of a dead agent's beam in the compact gather formats
constexpr int kLidarCodeDead = 255;
// decode the compact format's rows: obs [n][D] from heads [n][31] and codes [n][slots]
hipError_t launch_unpack_lidar_u8(const float* head, const uint8_t* codes, const float* table, float* obs, int n,
                                  int D, int slots, hipStream_t s);
// The state format's per-agent arrays, n elements each: x, y, v, heading f32 at
// byte offsets 0, 4n, 8n, 12n; route, path index i16 at 16n, 18n; intention,
// alive u8 at 20n, 21n -- 22 bytes per agent.
constexpr int kStateBytesPerAgent = 22;
struct SimParams;
// Rebuild the float observation rows of state-format messages (no traffic): n_env
// envs, env g in message g / C (messages `stride` bytes apart), slot g % C; each
// message's state arrays (C * N elements) at state0 and LiDAR codes [C*N][lidar_slots]
// at codes0 (+ the message offset); obs [n_env][N][D] -- the rows the plain step
// writes, bit for bit (write_obs_head_tg + the decode table).
hipError_t launch_decode_state(const SimParams& p, const uint8_t* state0, const uint8_t* codes0, size_t stride, int C,
                               int n_env, const float* table, float* obs, hipStream_t s);

struct SimParams {
    int32_t E, N, R, K, D;   // envs, agents, beams, npc slots, obs_dim
    int32_t lidar_slots;     // min(R, D - 31)
    int32_t num_lanes;
    int32_t irw;             // road half width in px (L*42)
    int32_t line_stop;       // LineMask stop offset int(L*42) + 84
    float rw;                // road half width (float)
    int32_t use_team, respawn, traffic, max_steps;
    float k_prog, v_min, k_stuck, k_cv, k_co, k_succ, k_sm, alpha;
    float max_progress;      // hypot(750, 750)
    float lidar_max, lidar_step, lidar_inv;
    int32_t lidar_steps;      // S = number of march probes (dist < max_dist)
    // host side: never choose the kernels that hold the reference's world at compile time
    // (MEV_NO_WORLD_CONST=1 at mev_create).  (In the four bytes that pad dist_tab to its
    // alignment: every other field keeps its offset.)
    int32_t no_world_const;
    const float* dist_tab;    // [S] accumulated probe distances, or null when dist_k == k*step exactly
    uint64_t seed;
    EgoSoA ego;
    NpcSoA npc;
    RouteTab rt;
    const float* rel_angles;  // [R]
    const int32_t* traffic_routes;  // [M] route ids
    int32_t n_traffic_routes;
    int32_t* step_count;      // [E]
    uint8_t* pending_reset;   // [E]
    unsigned long long* overflow;  // [3]: dropped spawns, sequential NPC turns (npc_phase), undecodable route ids (k_decode_state)
    unsigned long long* debug;     // diagnostic builds only (MEV_STAMPS): [E*8]
    // LiDAR hand-off k_cars -> k_lidar (L2-resident, rewritten every step)
    int4* ob_box;                  // [E][ob_stride] integer pixel AABB (x0, x1, y0, y1)
    unsigned long long* ob_cand;   // [E*N][2] candidate obstacle bits per agent
    int32_t ob_stride;             // N + max_npcs
    // route pool drawn per agent at every reset (n_reset_routes == 0: routes stay fixed)
    const int32_t* reset_routes;
    int32_t n_reset_routes;
    // step kernel choice (host side): 0 auto, 1 k_cars + k_lidar, 2 fused k_step
    int32_t step_kernel;
    // envs per fused k_step wave (host side): 0 auto, 1, 2 or 4 (reduced to fit 8 agent slots)
    int32_t step_pack;
    // two waves per fused workgroup (host side): 0 auto (<= 2048 workgroups), 1 off, 2 on
    int32_t step_split;
    // NPC-aware env deal of the fused traffic kernel (see kDealLists): per (ring, list,
    // class) counters, each on its own 128-B line, and per (ring, list, class) env orders
    int32_t* deal_cnt;    // [3][kDealLists][kDealClasses][kDealPad]
    int32_t* deal_order;  // [3][kDealLists][kDealClasses][E]: rings like the counters
    // Car sizes (Car::length / Car::width, cpp/Car.h:19-20), (length, width) per car: ego
    // [E*N][2], NPC [E*K][2] (moved with the NPCs).  Always valid: every entry is 54, 24 until
    // mev_set_car_dims.  The kernels that can run a handle with other sizes (k_cars, k_reset,
    // k_step<NM = 0>) read and keep them; dims: some car differs from 54 x 24, so the steps
    // run those kernels (the compile-time layouts assume the reference's size).  Last in the
    // struct: the other fields keep their offsets.
    float* ego_dim;
    float* npc_dim;
    int32_t dims;
    // LiDAR phase 3b culls each obstacle box to the beams its angular span covers with a
    // linear model of the offsets: rel[b] = rel[0] + b*d, d > 0, (R-1)*d <= 2*pi (every list
    // Lidar() / add_car_with_route makes with fov > 0).  0 for any other list (descending,
    // constant, uneven or wider than a revolution; a written Lidar.rel_angles): every beam
    // is then resolved against every candidate box -- the same probes, no culling.
    int32_t beam_cull;
    // What the LiDAR derives from the beam offsets alone (mev_beams.h), refreshed with rel_angles.
    BeamModel beams;
};

// The fused traffic k_step deals envs to workgroups by their NPC count: every env
// stays in logical list x (the workgroups b with b % 8 == x, i.e. one XCD), and
// within a list the workgroups take its envs heaviest first (the i-th workgroup of
// list x, b = 8 i + x, the i-th env in descending NPC class), so that the first
// workgroups the dispatcher places -- one per SIMD -- hold the heaviest envs and
// every SIMD's four wave slots get one env from each quarter of the NPC-count
// order.  At the end of its step each env appends itself to the class list of
// step t+1 (a counter atomic per (list, class)); rings of three counter sets and
// three order sets: step t reads ring t % 3, fills ring (t+1) % 3 and clears the
// counters of ring (t+2) % 3.  (With one order set, step t's early envs would
// overwrite entries that workgroups starting later still have to read.)
constexpr int kDealLists = 8;
constexpr int kDealClasses = 8;  // NPC counts 0..6, 7 and more
constexpr int kDealPad = 32;     // ints per counter (128 B)
constexpr int kDealRingInts = kDealLists * kDealClasses * kDealPad;

struct StepInputs {
    const float* actions;      // [E*N*2]
    const int32_t* spawn_route;  // [E] or null
    float dt;
    float spawn_prob;          // 1 - expf(-density * dt) computed on host with glibc
    int32_t auto_reset;
    uint64_t rng_counter;      // handle-wide step counter (Philox counter for NPC spawns)
    // NPC-aware deal (fused traffic k_step): bit 0 take envs from ring deal_ring's
    // lists (else the XCD-aware identity order), bit 1 build ring deal_ring + 1
    int32_t deal;
    int32_t deal_ring;
};

// The kernels launch_step and launch_serve use for p, their launches and what the
// getters report: plan_step (mev_plan.h) of p's shape.
// whether p's world is kRefWorld, field by field (what StepWorld<true> replaces with constants)
inline bool reference_world(const SimParams& p) {
    constexpr WorldConsts w = kRefWorld;
    return p.num_lanes == w.num_lanes && p.irw == w.irw && p.line_stop == w.line_stop && p.rw == w.rw &&
           p.lidar_max == w.lidar_max && p.lidar_step == w.lidar_step && p.lidar_inv == w.lidar_inv &&
           p.lidar_steps == w.lidar_steps && p.dist_tab == nullptr && p.max_progress == world_max_progress() &&
           p.beam_cull == 1;
}
inline StepShape step_shape(const SimParams& p) {
    return {p.E, p.N, p.R, p.K, p.lidar_slots, p.traffic, p.dims, p.step_kernel, p.step_pack, p.step_split,
            !p.no_world_const && !p.dims && reference_world(p)};
}
inline StepPlan plan_step(const SimParams& p) { return plan_step(step_shape(p)); }
// whether a step of p into out writes plain rows: 31 + R floats, every column written by the
// step, neither compact gather format (what a kernel with the rows at compile time, StepKey::wc,
// assumes; step_row in mev_plan.h)
inline bool plain_rows(const SimParams& p, const Outputs& out) {
    return out.obs_ld == OBS_HEAD + p.R && p.D == out.obs_ld && !out.lidar_u8 && !out.state;
}
// ev (nullable): three events recorded before k_cars, between k_cars and k_lidar, after k_lidar
// (with k_step: before it, and twice after it)
// dp: a device copy of p (k_step reads its parameters through it)
hipError_t launch_step(const SimParams& p, const SimParams* dp, const StepInputs& in, const Outputs& out,
                       hipStream_t s, const hipEvent_t* ev = nullptr);
// A window (mev_step_repeat, mev_step_sequence): up to n sub-steps of the car part per env in one
// launch (k_cars_repeat: the state stays on the CU in between), then one k_lidar cast from the
// state each env stopped at.  in.spawn_route, if given, is [n][E]; sub-step s uses
// in.rng_counter + s.  substeps (nullable): [E] sub-steps executed.  Every shape k_cars runs.
// rows == nullptr (frame skip): the action in.actions [E][N][2] is held, with in.dt and
// in.spawn_prob, for every sub-step.
// rows (a plan rollout, n <= kMaxSeq): an action row, a dt and a spawn probability of its own
// per sub-step (k_cars_repeat<TRAFFIC, SEQ = true>).  in.actions is [n][E][N][2]; in.dt and
// in.spawn_prob are not read: sub-step s takes dt[s] and spawn_prob[s], which travel by value
// in the kernel's argument segment.  reward / done / status (each nullable) are [n][E][N]: row
// s holds sub-step s's own outputs for the envs that ran it, zero after an env stopped (the
// wave that stops writes its remaining rows itself).
constexpr int kMaxSeq = 64;  // == MEV_MAX_REPEAT
struct SeqRows {
    float* reward;
    uint8_t* done;
    uint8_t* status;
    float dt[kMaxSeq];
    float spawn_prob[kMaxSeq];
};
hipError_t launch_step_window(const SimParams& p, const StepInputs& in, const Outputs& out, int n,
                              const SeqRows* rows, int32_t* substeps, hipStream_t s);
// The five plan evaluations (mev_evaluate_plans, mev_evaluate_leaves, mev_expand_plans,
// mev_sample_plans, mev_sample_expand_plans) are one call, launch_plans, described by a PlanCall
// below: the paragraphs up to it say what each part of the descriptor adds.
// Plan evaluation (mev_evaluate_plans; leaf_obs, dst and sample null): C candidates, candidate c
// rolled through a plan of n sub-steps from a private copy of the live env roots[c] (k_cars_repeat<TRAFFIC, true, EVAL =
// true>), and nothing of p's state, outputs or diagnostics written: one launch of C single-wave
// workgroups, no k_lidar.  in.actions is [n][C][N][2], in.spawn_route, if given, [n][C]; the
// Philox spawner is keyed by c with in.rng_counter + s; in.auto_reset is not read (never a
// reset).  rows as for launch_step_window with [n][C][N] arrays.  A root outside [0, p.E) makes
// its candidate's outputs zero.  Every shape k_cars runs.
struct EvalOutputs {
    float gamma;          // discount of returns
    float* returns;       // [C][N] (each nullable)
    int32_t* substeps;    // [C]
    uint8_t* terminated;  // [C] flags of the sub-step the candidate stopped at
    uint8_t* truncated;   // [C]
};
// Plan evaluation with leaf observations (mev_evaluate_leaves; leaf_obs set): the same rollout, and
// leaf_obs [C][N][p.D] = the observation of the state each candidate stopped at
// (k_cars_repeat<TRAFFIC, true, true, LEAF = true>, then k_lidar).  The sub-step a candidate stops
// at writes its observation head into leaf_obs row c and publishes a LiDAR hand-off indexed by
// the candidate -- poses, alive, candidate masks, boxes -- into `hand`, a scratch of the caller's
// for `chunk` candidates (leaf_hand_bytes); k_lidar then casts the chunk's agents from a SimParams
// copy whose ego block, alive, ob_box, ob_cand and E describe that scratch and whose rows are
// leaf_obs.  The candidates go through in chunks of `chunk`, car kernel then cast per chunk, in
// stream order; roots, actions, rows and outputs stay indexed by the global c.  p's own hand-off
// tables, state and outputs are neither read (beyond the roots' state) nor written.
struct LeafHand {
    float* pose;                  // [4][stride]: x, y, (unused), heading -- the ego block's field order
    int64_t stride;               // >= chunk * N
    uint8_t* alive;               // [chunk * N]
    int4* box;                    // [chunk][ob_stride]
    unsigned long long* cand;     // [chunk * N][2]
    int32_t c0;                   // the chunk's first candidate
};
size_t leaf_hand_bytes(const SimParams& p, int chunk);
// A state pool (mev_pool_create): `slots` complete env states outside the live batch, structure of
// arrays over slots in the handle's own field layout -- slot d's agent i at d * N + i, its NPC
// slot k at d * K + k -- so a SimParams copy whose state block points here (pool_view) lets every
// kernel that loads an env's state load a slot's.  No outputs, LiDAR hand-off or pending-reset
// flag; per slot a valid byte (0 until a state was stored; cleared by mev_set_car_dims).
struct PoolState {
    float* ego;           // [EF_COUNT][ego_stride]: the 4-byte ego fields, EgoField order
    int64_t ego_stride;   // >= slots * N
    float* npc;           // [NF_COUNT][npc_stride]: the 4-byte NPC fields, NpcField order
    int64_t npc_stride;   // >= slots * K
    uint8_t* ego_alive;   // [slots * N]
    uint8_t* npc_alive;   // [slots * K]
    int32_t* npc_count;   // [slots]
    int32_t* step_count;  // [slots]
    float* ego_dim;       // [slots * N][2]
    float* npc_dim;       // [slots * K][2]
    uint8_t* valid;       // [slots]
    int32_t slots;
};
// the live batch of p as a PoolState of p.E slots without valid bytes (every env counts as valid)
PoolState pool_of_live(const SimParams& p);
// p with its state block replaced by the pool's (E = slots; pending_reset, which the plan
// evaluation reads and ignores, points at the valid bytes): what k_cars_repeat<EVAL> loads from
SimParams pool_view(const SimParams& p, const PoolState& pool);
// Gather copy between two state blocks of one shape (mev_pool_capture, mev_pool_get_state): entry
// i copies slot from[i] of src into slot to[i] of dst (from / to null: i itself), every field of
// all K NPC slots included; dst's valid byte becomes src's, or 1 when src has none.  A pair with
// either index out of range is skipped: nothing is accessed outside the blocks.
hipError_t launch_pool_copy(const SimParams& p, const PoolState& src, const PoolState& dst, const int32_t* from,
                            const int32_t* to, int count, hipStream_t s);
// Plan expansion (mev_expand_plans; dst set): the plan evaluation, without or with leaf observations,
// bit for bit, with two additions (k_cars_repeat<..., KEEP = true>).  src (nullable): candidate c
// starts from slot roots[c] of that pool instead of live env roots[c]; a root out of range or a
// slot whose valid byte is 0 is a candidate without a root.  dst: the sub-step a candidate that
// ran stops at stores its whole post-step state -- what the plan rollout would write back to an
// env -- into slot dst_slots[c] of dst and sets the slot's valid byte; an index outside [0,
// dst.slots) stores nothing.  src and dst may be one pool when no dst slot of the call is a root.
// Together with sample (mev_sample_expand_plans): roots is [groups] and names slots of src.
// Sampled plan evaluation (mev_sample_plans; sample set): the plan evaluation, without or with leaf
// observations, bit for bit, whose candidates draw their own actions
// (k_cars_repeat<..., SAMPLE = true>).  in.actions is not read; candidate c = g * samples + j
// starts from live env roots[g] (roots is [groups], C = groups * samples; with dst: from slot
// roots[g] of src when that is set, and its stop state is kept as above) and takes, per sub-step
// row s, agent i, component k, clamp(mean[s][g][i][k] + sigma[s][g][i][k] * eps[k], lo[k], hi[k])
// with eps from Philox4x32-10 keyed by the noise seed at counter (noise counter, c * 64 + i, s).
// Every element of actions_out (nullable) is written, for candidates that stop early or have no
// root as well.
struct SampleIn {
    const float* mean;   // [n][groups][N][2]
    const float* sigma;  // [n][groups][N][2]
    float* actions_out;  // [n][C][N][2] (nullable)
    float lo[2], hi[2];
    int32_t groups, samples;
    uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;  // the noise stream: Philox key and counter words 0, 1
    uint32_t mean_first;                        // candidate j == 0 of every group takes eps = 0
};
struct PlanCall {
    int C, n;                  // candidates (with sample: groups * samples), sub-steps (1..kMaxSeq)
    const int32_t* roots;      // [C], or [groups] with sample
    const SeqRows* rows;       // the [n][C][N] arrays, dt and spawn probability per sub-step
    EvalOutputs outs;
    float* leaf_obs;           // [C][N][p.D] (null: no leaf observations, no k_lidar)
    uint8_t* hand;             // with leaf_obs: the hand-off scratch, leaf_hand_bytes(p, chunk)
    int chunk;                 // with leaf_obs: candidates per car-kernel launch and cast (>= 1)
    const PoolState* src;      // with dst: the pool the roots are slots of (null: live envs)
    const PoolState* dst;      // the pool that receives the stop states (null: none kept)
    const int32_t* dst_slots;  // with dst: [C]
    const SampleIn* sample;    // null: the actions are in.actions
};
hipError_t launch_plans(const SimParams& p, const StepInputs& in, const PlanCall& c, hipStream_t s);
// Refit over candidates (mev_update_plans, k_update_plans): one workgroup per group ranks its
// `samples` candidates by score (scores[c], or the in-order f32 sum of returns[c][0..N); a
// non-finite score counts as -FLT_MAX; equal scores: the lower j first) and reduces the action rows
// to a new mean and sigma per (s, i, k): mode 0 over the first `elites` in rank order, mode 1 with
// weights expf((score - best) * inv_temperature) in j order.  Every output is nullable.
struct UpdateArgs {
    const float* actions;  // [n][C][N][2]
    const float* scores;   // [C] (nullable)
    const float* returns;  // [C][N], read when scores is null
    int32_t groups, samples, n, N;
    int32_t mode, elites;
    float inv_temperature, sigma_min;
    float* new_mean;       // [n][groups][N][2]
    float* new_sigma;      // [n][groups][N][2]
    int32_t* best;         // [groups]
    float* best_score;     // [groups]
    int32_t* order;        // [groups][elites] (mode 0)
    float* weights;        // [C] (mode 1)
};
hipError_t launch_update_plans(const UpdateArgs& u, hipStream_t s);
hipError_t launch_reset(const SimParams& p, const uint8_t* env_mask, const Outputs& out, hipStream_t s,
                        uint64_t rng_counter);
// recompute the observation rows from the current state with LiDAR = max (after set_state)
hipError_t launch_observe_reset_lidar(const SimParams& p, const Outputs& out, hipStream_t s);

// Persistent step server (k_serve) of a small host-mode handle: the mailbox in
// host-coherent pinned memory.  A posting writes the command line's fields, then
// seq (release).  STEP carries a step number sid (a re-post after a relaunch keeps
// it); workgroup b answers done[b] = sid once its outputs are in the pinned block,
// and answers a sid it has served before with nothing.  STOP writes only cmd and
// seq.  Every workgroup publishes exited[b] = its instance's epoch when it leaves
// (STOP, or no posting for ServeArgs::idle_ticks).
constexpr int kServeLine = 9;  // words of the command line
constexpr uint32_t kServeStep = 1, kServeStop = 2;
struct ServeBox {
    uint32_t seq, cmd, sid;     // host -> device: posting number, kind, step number
    uint32_t dt, spawn_prob;    // f32 bits
    uint32_t auto_reset, spawn;  // spawn: spawn_route holds this step's routes
    uint32_t rng_lo, rng_hi;    // StepInputs::rng_counter
    uint32_t pad0[23];
    uint32_t done[kServeMaxWG];    // device -> host
    uint32_t exited[kServeMaxWG];  // device -> host
};
struct ServeArgs {
    ServeBox* box;               // device address of the mailbox
    const float* actions;        // device address of the pinned actions
    const int32_t* spawn_route;  // device address of the pinned spawn routes
    uint32_t epoch;
    uint32_t idle_ticks;         // 100 MHz ticks
};
// (only where plan_step(p).serve_fits)
hipError_t launch_serve(const SimParams& p, const SimParams* dp, const ServeArgs& sa, const Outputs& out,
                        hipStream_t s);

// Closed-loop policy rollouts (mev_rollout_policy, k_rollout).  A policy's device block: layer l as
// wt[l][k * ld[l] + j] = W[l][j][k] (transposed: lane j reads one coalesced line per k) followed by
// the bias row wt[l][in[l] * ld[l] + j]; ld = out rounded up to 64, the padding zero.  The last
// used layer has out = 2; column 2 of its block holds the value head (mev_policy_set_value_head: wv[k] in
// row k, bv[0] in the bias row), zero while none is attached.
// act: the policy's activations, fixed at creation -- kPolicyHiddenTanh: every hidden layer applies tanh_c
// (mev_act.h) in the ReLU's place; kPolicyOutTanh: mu = tanh_c(mu) before the noise (never the value head).
// 0: the ReLU policy, which runs the instantiations without ACT.
constexpr int32_t kPolicyHiddenTanh = 0x10;  // == MEV_POLICY_HIDDEN_TANH
constexpr int32_t kPolicyOutTanh = 0x20;     // == MEV_POLICY_OUT_TANH
struct PolicyNet {
    const float* wt[3];
    int32_t in[3], out[3], ld[3];
    int32_t layers;  // 2 or 3
    int32_t act;     // kPolicyHiddenTanh | kPolicyOutTanh
};
// repack a policy's [out][in] weights and [out] biases (device arrays) into dst (PolicyNet's layout)
// keep_head: the value head's column is left as it stands
hipError_t launch_policy_repack(const PolicyNet& dst, const float* const* w, const float* const* b, bool keep_head,
                                hipStream_t s);
// the value head's column from wv [in of the last layer] and bv [1] (device arrays); wv null: zeros
hipError_t launch_value_head_repack(const PolicyNet& dst, const float* wv, const float* bv, hipStream_t s);
// One launch of T sub-steps: per sub-step t the policy on the env's observation rows -- obs0 at t = 0,
// then the rows sub-step t - 1 wrote -- then the fused step's body with the actions the policy wrote,
// in.spawn_route ([T][E], nullable) and in.rng_counter advanced to row t.  Each *_seq array (nullable)
// receives row t of its output; a null one leaves that output in `out` (the handle's own buffers,
// rewritten every sub-step).  act_scratch [E][N][2] holds the action row when actions_seq is null.
struct RolloutArgs {
    StepInputs in;
    PolicyNet net;
    int32_t T, pol_off;
    const float* obs0;  // [E][N][D]
    float *obs_seq, *actions_seq, *mean_seq, *reward_seq;
    uint8_t *done_seq, *status_seq, *term_seq, *trunc_seq;
    float* act_scratch;
    int32_t noisy;  // sigma given
    float sigma[2], lo[2], hi[2];
    uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
    // non-null: the value instantiation (mev_rollout_policy_values).  [T + 1][E][N]: row t = the value head on the
    // rows the policy of sub-step t reads, row T on the rows the last sub-step wrote.
    float* value_seq;
};
// (rp: plan_rollout of p's shape, its row >= 0)
hipError_t launch_rollout(const SimParams& p, const SimParams* dp, const RolloutPlan& rp, const RolloutArgs& ra,
                          const Outputs& out, hipStream_t s);
// mev_rollout_policy_repeat (k_rollout's REPEAT instantiations): T DECISIONS, each one policy phase (noise word
// index t) and then up to `repeat` sub-steps of the fused step's body on the held action row -- sub-step s with
// in.spawn_route row t * repeat + s ([T * repeat][E]), in.rng_counter + t * repeat + s, and in.auto_reset at
// s == 0 only -- the env stopping at its first ended sub-step.  Row t of the *_seq arrays is the decision's:
// the reward summed in sub-step order, done and status latched (RepCarry's rules), the flags and the
// observation of the sub-step it stopped at.  A struct of its own on top of RolloutArgs, so that the kernel
// argument segment of the instantiations without REPEAT is what it was; `value_seq` stays the base's last
// field and chooses the value instantiation as it does there.
struct RolloutRepeatArgs : RolloutArgs {
    int32_t repeat;         // n, 1..MEV_MAX_REPEAT
    int32_t* substeps_seq;  // [T][E] sub-steps decision t ran in env e (nullable)
};
hipError_t launch_rollout_repeat(const SimParams& p, const SimParams* dp, const RolloutPlan& rp,
                                 const RolloutRepeatArgs& ra, const Outputs& out, hipStream_t s);
// mev_rollout_policies (k_rollout's MULTI instantiations, on the REPEAT loop): agent slot (e, i) is driven by
// nets[assign[e][i]] for the whole call -- an entry above P - 1 is read as P - 1 -- with that policy's sigma row
// and value head.  The base's `net` and `sigma` are not read; `noisy` says whether sigma was given.  rp's LDS
// holds the largest sum of hidden widths among the P nets.  A struct of its own on top of RolloutRepeatArgs,
// as that one is on RolloutArgs: the other instantiations' kernel argument segments are what they were.
constexpr int kMaxRolloutPolicies = 8;  // == MEV_MAX_ROLLOUT_POLICIES
struct RolloutMultiArgs : RolloutRepeatArgs {
    PolicyNet nets[kMaxRolloutPolicies];  // [P] used
    int32_t P;                            // 1..kMaxRolloutPolicies
    const uint8_t* assign;                // [E][N]
    float sigmas[kMaxRolloutPolicies][2];
};
hipError_t launch_rollout_multi(const SimParams& p, const SimParams* dp, const RolloutPlan& rp,
                                const RolloutMultiArgs& ra, const Outputs& out, hipStream_t s);

// mev_gae (k_gae): the reverse scan of mev_gae.h's gae_step over T rows per (e, i).  c = gamma * lambda in f32.
struct GaeArgs {
    const float* reward;          // [T][E][N]
    const float* value;           // [T + 1][E][N]
    const uint8_t* done;          // [T][E][N] (nullable)
    const uint8_t* term;          // [T][E] (nullable)
    const uint8_t* trunc;         // [T][E] (nullable)
    const uint8_t* ended_before;  // [E] (nullable), read with mask
    int32_t T, E, N, mask;
    float gamma, c;
    float* adv;      // [T][E][N] (nullable)
    float* ret;      // [T][E][N] (nullable)
    uint8_t* valid;  // [T][E][N] (nullable)
};
hipError_t launch_gae(const GaeArgs& a, hipStream_t s);

// masked per-env copy of snapshot fields (mev_restore)
constexpr int kMaxRestoreFields = 48;
struct RestoreTab {
    int32_t n;
    uint8_t* dst[kMaxRestoreFields];
    unsigned long long src_off[kMaxRestoreFields];
    int32_t bpe[kMaxRestoreFields];  // bytes per env
};
hipError_t launch_restore(const RestoreTab& tab, const uint8_t* src, const uint8_t* env_mask, int E, hipStream_t s);
// mapped per-env copy (mev_restore_map): env e takes the slices of the snapshot's env env_map[e];
// an entry outside [0, E) leaves env e alone
hipError_t launch_restore_map(const RestoreTab& tab, const uint8_t* src, const int32_t* env_map, int E, hipStream_t s);

}  // namespace mev
