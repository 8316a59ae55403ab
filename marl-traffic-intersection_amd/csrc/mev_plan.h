// mev_plan.h — which step kernel a handle runs, and with what launch: one host
// function, plan_step.  Host-only and free of HIP: the launchers (mev_kernels.hip)
// look the plan's key up in their kernel tables, the C API reads its fields, and a
// CPU test pins it (tests/native/step_plan_check.cpp).
#pragma once

#include "mev_layout.h"

namespace mev {

// what the policy reads of a handle (SimParams; step_shape in mev_kernels.h)
struct StepShape {
    int E, N, R, K, lidar_slots;      // envs, agents, beams, NPC slots, beams in the observation
    int traffic, dims;                // traffic mode; some car is not 54 x 24
    int step_kernel, step_pack, step_split;  // mev_set_step_kernel / _pack / _split (0: automatic)
    int world = 0;                    // the reference's world (kRefWorld, mev_refworld.h), every car 54 x 24
};

// k_step's template arguments (k_serve's: PK = 1, no ESPLIT), TAB aside
struct StepKey {
    bool traffic;
    int nm, km, pk;  // compile-time layout of NM agents (0: runtime layout), NPC capacity, envs per workgroup
    bool split, esplit;
    int p1, nc;  // the beams and the agents per env fixed at compile time, 0: neither (p1 1 / 2: only
                 // whether the beams are a multiple of 64 / not)
    int wc = 0;  // the reference's world and plain observation rows at compile time (StepWorld / StepRows, mev_refworld.h)
};
constexpr bool operator==(const StepKey& a, const StepKey& b) {
    return a.traffic == b.traffic && a.nm == b.nm && a.km == b.km && a.pk == b.pk && a.split == b.split &&
           a.esplit == b.esplit && a.p1 == b.p1 && a.nc == b.nc && a.wc == b.wc;
}
struct StepLaunch {
    StepKey key;
    unsigned grid, block, lds;  // workgroups, threads, dynamic LDS bytes
};

struct StepPlan {
    int path;  // 1 = k_cars + k_lidar, 2 = the fused k_step; 0: step_kernel == 2 but k_step cannot hold the shape
    StepLaunch step;  // path 2 only (zero otherwise)
    // the persistent step server (k_serve: fused, one workgroup per env, <= kServeMaxWG envs).
    // (serve.key's p1 / nc are those of k_step at that shape; k_serve has fewer such rows
    // and runs its unspecialised one for the others)
    bool serve_fits;
    StepLaunch serve;  // serve_fits only (zero otherwise)
    int pack, split;  // what mev_get_step_pack / mev_get_step_split report (not the key's pk / split)
};

constexpr int kServeMaxWG = 64;
// two waves per fused workgroup (k_step SPLIT) when that keeps <= 4 waves per SIMD
// (<= 2048 workgroups; 256 CUs x 4 SIMDs)
constexpr int kSplitMaxWg = 2048;

// the compiled kernels: X(TRAFFIC, NM, KM, PK, SPLIT, ESPLIT, P1, NC, WC), each for both TAB (a WC row's
// TAB slot holds the row's kernel without WC: the reference's LiDAR step reads no distance table)
#define MEV_STEP_KERNELS(X)                                                                               \
    /* traffic: the early split (config 4: its 64 beams at compile time), one ego and <= 32 NPC slots,    \
       the runtime layouts */                                                                             \
    X(true, 1, 32, kTsplitEnvs, true, true, 64, 0, 0)                                                     \
    X(true, 1, 32, kTsplitEnvs, true, true, 0, 0, 0)                                                      \
    X(true, 1, 32, 1, false, false, 0, 0, 0)                                                              \
    X(true, 0, 32, 1, false, false, 0, 0, 0)                                                              \
    X(true, 0, 64, 1, false, false, 0, 0, 0)                                                              \
    /* the early split (config 2: 4 envs x 1 agent x 64 beams; the reference's defaults: 1 x 96) */       \
    X(false, 8, MAXK, 8, true, true, 0, 0, 0)                                                             \
    X(false, 8, MAXK, 4, true, true, 64, 1, 0)                                                            \
    X(false, 8, MAXK, 4, true, true, 0, 1, 0)                                                             \
    X(false, 8, MAXK, 4, true, true, 0, 0, 0)                                                             \
    X(false, 8, MAXK, 2, true, true, 96, 1, 0)                                                            \
    X(false, 8, MAXK, 2, true, true, 0, 1, 0)                                                             \
    X(false, 8, MAXK, 2, true, true, 0, 0, 0)                                                             \
    X(false, 8, MAXK, 1, true, true, 0, 0, 0)                                                             \
    /* two waves per workgroup (configs 3 / 5 and 96 beams in smaller batches; config 1: one agent) */    \
    X(false, 8, MAXK, 8, true, false, 0, 0, 0)                                                            \
    X(false, 8, MAXK, 4, true, false, 0, 0, 0)                                                            \
    X(false, 8, MAXK, 2, true, false, 0, 0, 0)                                                            \
    X(false, 8, MAXK, 1, true, false, 64, 8, 0)                                                           \
    X(false, 8, MAXK, 1, true, false, 96, 8, 0)                                                           \
    X(false, 8, MAXK, 1, true, false, 128, 8, 0)                                                          \
    X(false, 8, MAXK, 1, true, false, 0, 1, 0)                                                            \
    X(false, 8, MAXK, 1, true, false, 0, 0, 0)                                                            \
    /* one wave per workgroup */                                                                          \
    X(false, 8, MAXK, 8, false, false, 0, 0, 0)                                                           \
    X(false, 8, MAXK, 4, false, false, 0, 0, 0)                                                           \
    X(false, 8, MAXK, 2, false, false, 0, 0, 0)                                                           \
    X(false, 8, MAXK, 1, false, false, 64, 8, 0)                                                          \
    X(false, 8, MAXK, 1, false, false, 64, 0, 0)                                                          \
    X(false, 8, MAXK, 1, false, false, 96, 8, 0)                                                          \
    X(false, 8, MAXK, 1, false, false, 96, 0, 0)                                                          \
    X(false, 8, MAXK, 1, false, false, 128, 8, 0)                                                         \
    X(false, 8, MAXK, 1, false, false, 128, 0, 0)                                                         \
    X(false, 8, MAXK, 1, false, false, 1, 0, 0)                                                           \
    X(false, 8, MAXK, 1, false, false, 2, 0, 0)                                                           \
    /* the runtime layout */                                                                              \
    X(false, 0, MAXK, 1, false, false, 0, 0, 0)                                                           \
    /* one wave per env with the reference's world and plain rows at compile time (the metric's           \
       config 3, config 5) */                                                                             \
    X(false, 8, MAXK, 1, false, false, 64, 8, 1)                                                          \
    X(false, 8, MAXK, 1, false, false, 128, 8, 1)
// k_serve's (env.py's common shapes with their counts at compile time: one agent, 8 agents x 64 / 96 beams)
#define MEV_SERVE_KERNELS(X)               \
    X(true, 1, 32, 1, false, false, 0, 0, 0)  \
    X(true, 0, 64, 1, false, false, 0, 0, 0)  \
    X(false, 8, MAXK, 1, true, false, 0, 1, 0)  \
    X(false, 8, MAXK, 1, true, false, 64, 8, 0) \
    X(false, 8, MAXK, 1, true, false, 96, 8, 0) \
    X(false, 8, MAXK, 1, true, false, 0, 0, 0)
#define MEV_KEY_ROW(T, NM, KM, PK, S, ES, P1, NC, WC) StepKey{T, NM, KM, PK, S, ES, P1, NC, WC},
constexpr StepKey kStepKeys[] = {MEV_STEP_KERNELS(MEV_KEY_ROW)};
constexpr StepKey kServeKeys[] = {MEV_SERVE_KERNELS(MEV_KEY_ROW)};
#undef MEV_KEY_ROW
// the row of key k in a key list (the kernel tables keep its order), or -1
template <int n>
inline int key_row(const StepKey (&keys)[n], const StepKey& k) {
    for (int i = 0; i < n; ++i)
        if (keys[i] == k) return i;
    return -1;
}
// k_serve's row for the plan's serve key: that key's, else its unspecialised one's
inline int serve_row(StepKey k) {
    k.wc = 0;  // (k_serve has no such rows)
    const int r = key_row(kServeKeys, k);
    if (r >= 0) return r;
    k.p1 = k.nc = 0;
    return key_row(kServeKeys, k);
}

inline StepPlan plan_step(const StepShape& p) {
    StepPlan pl{};
    // ---- the LDS of one k_step wave: the dynamic part (cars + one LiDAR pool of
    // step_pool(p) agents) plus, with traffic, the static NPC arrays (the smallest compiled
    // capacity that holds max_npcs; the runtime-layout traffic kernels hold the NPC sizes too)
    const unsigned dyn_lds = (unsigned)step_layout(p).bytes;
    const int npc_cap = p.K <= 32 ? 32 : 64;
    const size_t fused_lds =
        dyn_lds + (!p.traffic ? 0 : npc_cap == 32 ? sizeof(NpcLDST<32, true>) : sizeof(NpcLDST<64, true>));
    // The compile-time layouts: 8 agent slots without traffic, one ego and <= 32 NPC slots with
    // it (config 4), each within a wave's 10 KB LDS share, the NPC arrays included.  R <= 128
    // puts every pool (step_pool agents) within the layout's beams; a handle with cars of other
    // sizes runs the runtime layout.
    const bool fixed_shape = p.R <= kFixedRays && !p.dims;
    const bool fits8 = fixed_shape && !p.traffic && p.N <= 8 && (size_t)FixedLayout<8, 0>::bytes <= 10 * 1024;
    const bool fits_t = fixed_shape && p.traffic && p.K <= 32 && p.N <= 1 &&
                        (size_t)FixedLayout<1, 32>::bytes + sizeof(NpcLDST<32>) <= 10 * 1024;

    // ---- the path.  k_step applies when its LDS fits one workgroup (64 KB); it is the
    // automatic choice when it also fits a wave's share at 4 waves per SIMD (128 VGPRs): a CU
    // holds 16 waves, so a wave may take 160 KB / 16 = 10 KB -- and either the batch fills
    // the chip with one wave per env (>= 4 per CU), or an env's beams fit one k_lidar
    // group anyway (N * R <= 256: the second launch buys nothing, 1 env x 1 agent 70 ->
    // 82 k steps/s fused), or the env fits the compile-time 8-slot layout: its k_step
    // (two waves per env below 2048 workgroups, counts at compile time) beats the
    // LiDAR's finer per-group waves at every batch size since round 6 (8 agents x 64
    // beams: 64 envs 21.2 -> 16.7 us, 768 envs 27.2 -> 18.3 us; profiles/r6_stepk_small.txt).
    // Larger envs at small batches keep the two-kernel path.
    const bool fusable = fused_lds <= 64 * 1024;
    if (p.step_kernel == 1) pl.path = 1;
    else if (p.step_kernel == 2) pl.path = fusable ? 2 : 0;
    else pl.path = fusable && fused_lds <= 10 * 1024 && (p.E >= 1024 || p.N * p.R <= 256 || fits8) ? 2 : 1;

    // the beam count a kernel fixes at compile time (its P1): 64, 96 or 128 beams, every one
    // in the observation; else 0
    const int fr = (p.R == 64 || p.R == 96 || p.R == 128) && p.lidar_slots == p.R ? p.R : 0;
    const bool set_pack = p.step_pack == 1 || p.step_pack == 2 || p.step_pack == 4 || p.step_pack == 8;
    const bool may_esplit = p.step_split == 0 || p.step_split == 3;

    // ---- the fused launch.  one: one workgroup per env (what k_serve runs)
    StepLaunch st{}, one{};
    int pack = 1;  // envs per workgroup as mev_get_step_pack reports them: 1 with traffic
    bool esplit = false, split = false;
    if (p.traffic) {
        // (+ the static NpcLDST)
        if (fits_t) one = {{true, 1, 32, 1, false, false, 0, 0}, (unsigned)p.E, WAVE, FixedLayout<1, 32>::bytes};
        else one = {{true, 0, npc_cap, 1, false, false, 0, 0}, (unsigned)p.E, WAVE, dyn_lds};
        st = one;
        // The traffic early split: kTsplitEnvs one-ego envs per workgroup, their car waves and
        // a LiDAR wave (every workgroup full, and the NPC-aware deal's lists of E / 8 envs split
        // into whole workgroups).  Automatic at every such E: with two envs per workgroup it
        // beats one wave per env from 16 to 16384 envs -- 16-512 envs 25-35 %, 8192 envs 145 ->
        // 165 M, 16384 160 -> 190 M agent-steps/s (profiles/r6_ts2_auto_*.txt).  (Round 5's four
        // envs per workgroup lost at 8192 envs, 55.9 -> 59.0 us, profiles/r5_ab_ts6_cfg4.txt.)
        constexpr int P = kTsplitEnvs;
        esplit = fits_t && p.R <= kTsplitRays && p.E % (8 * P) == 0 && may_esplit && (P >= 2 || p.step_split == 3);
        if (esplit) {
            const unsigned lds =
                (unsigned)(P * FixedLayout<1, 32>::lidar + lidar_layout_beams(P, P * kTsplitRays, 32, false).bytes);
            // (config 4: the beam count at compile time)
            st = {{true, 1, 32, P, true, true, fr == 64 ? 64 : 0, 0}, (unsigned)(p.E / P), (P + 1) * WAVE, lds};
        }
    } else if (fits8) {
        // Envs per workgroup of the early split (0: it does not apply).  An explicit
        // mev_set_step_pack is kept (reduced to <= 8 agent slots) when the slots' beams fit one
        // 512-beam LiDAR pool.  Automatic: 4 envs while their beams stay <= 256 and >= 1024
        // workgroups remain, else 2 envs within one pool and >= 1024 workgroups, else none (the
        // automatic choice then keeps one wave per env / the plain split;
        // mev_set_step_split(3) forces one env per workgroup at 8 waves per SIMD).
        // Measured against the plain split's best, one MI355X (profiles/r3_esplit_shapes.txt):
        // 4096 x 1 x 64 beams (config 2) 13.3 -> 11.6 us per step at 4 envs, 4096 x 4 x 64
        // 24.1 -> 22.0 at 2, 2048 x 1 x 64 12.4 -> 10.0 at 2, 4096 x 1 x 128 15.5 -> 14.4 at 2.
        const int nr = p.N * p.R;
        int ep = 0;
        if (set_pack) {
            ep = p.step_pack;
            while (ep > 1 && ep * p.N > 8) ep /= 2;
            if (ep * nr > kPoolBeams) ep = 0;
        } else if (4 * p.N <= 8 && 4 * nr <= kPoolBeams / 2 && p.E / 4 >= 1024) ep = 4;
        else if (2 * p.N <= 8 && 2 * nr <= kPoolBeams && p.E / 2 >= 1024) ep = 2;
        else if (p.step_split == 3 && nr <= kPoolBeams) ep = 1;
        // automatic (mode 0) from 2 envs per workgroup, or forced (mode 3)
        esplit = may_esplit && (p.step_split == 3 ? ep > 0 : ep >= 2);
        // Otherwise several small envs share a wave's lanes (1, 2, 4 or 8 of them, within the 8
        // agent slots), so one latency chain serves them all.  Automatic: the most envs per wave
        // that keeps >= 2048 waves (2 per SIMD) -- config 2 (4096 x 1 agent): 2 envs per wave,
        // 177 -> 202 M agent-steps/s; 4 envs per wave (1024 waves, one per SIMD) 194 M
        // (profiles/r2_pack_sweep.txt).
        if (esplit) pack = ep;
        else {
            pack = set_pack ? p.step_pack : 4;
            if (!set_pack)
                while (pack > 1 && p.E / pack < 2048) pack /= 2;
            while (pack > 1 && pack * p.N > 8) pack /= 2;
        }
        const unsigned wg = (unsigned)((p.E + pack - 1) / pack);
        // two waves per workgroup: the car part / LiDAR overlap
        split = !esplit && p.step_split != 1 && (p.step_split == 2 || wg <= (unsigned)kSplitMaxWg);
        // the beams (P1) and agents per env (NC) the kernel has at compile time
        int p1 = 0, nc = 0;
        if (esplit) {  // (config 2: 4 envs x 1 agent x 64 beams; the reference's defaults: one agent, 96 beams)
            if ((pack == 4 || pack == 2) && p.N == 1) { nc = 1; p1 = fr == (pack == 4 ? 64 : 96) ? fr : 0; }
        } else if (split && pack == 1) {  // (configs 3 / 5 and 96 beams' shapes in smaller batches; config 1: one agent)
            if (p.N == 8 && fr) { p1 = fr; nc = 8; }
            else if (p.N == 1) nc = 1;
        } else if (pack == 1) {  // (one wave per env: a P1 always)
            p1 = fr ? fr : (p.R & (WAVE - 1)) == 0 ? 1 : 2;
            nc = fr && p.N == 8 ? 8 : 0;
        }
        // the reference's world at compile time: the one-wave-per-env kernels of 8 agents x 64 / 128
        // beams (the metric's shape and config 5's; launch_step also asks for plain rows)
        const bool two = esplit || split;  // a car wave and a LiDAR wave
        const int wc = p.world && !two && pack == 1 && nc == 8 && (p1 == 64 || p1 == 128);
        st = {{false, 8, MAXK, pack, two, esplit, p1, nc, wc}, wg, two ? 2u * WAVE : 1u * WAVE, FixedLayout<8>::bytes};
        one = st;  // (k_serve: only where this is one workgroup per env, below)
    } else {
        st = one = {{false, 0, MAXK, 1, false, false, 0, 0}, (unsigned)p.E, WAVE, dyn_lds};
    }
    pl.pack = 1;
    if (pl.path == 2) {
        pl.step = st;
        pl.pack = pack;
        pl.split = esplit ? 2 : split ? 1 : 0;
    }

    // ---- k_serve runs the handle's fused step, one workgroup per env: the compile-time
    // layouts for small batches -- the split kernel without traffic, one ego with <= 32 NPC
    // slots -- and, for more NPC slots (env.py's 64), the dynamic traffic layout, which at one
    // env may take more than a wave's 10 KB share (so whatever the automatic path is)
    pl.serve_fits = pl.path != 0 && p.step_kernel != 1 && !p.dims && p.E <= kServeMaxWG &&
                    (p.traffic ? fits_t || (p.K > 32 && fusable) : fits8 && pack == 1 && split);
    if (pl.serve_fits) pl.serve = one;
    return pl;
}

// The rows the launchers run for plan pl, and the getter reports (mev_get_step_row): k_step's
// row in kStepKeys, -1 unless path 2 -- plain_rows: the call's observation rows are 31 + R
// floats, every column written by the step, neither compact gather format (plain_rows() in
// mev_kernels.h); only then does the key keep its wc -- and k_serve's row in kServeKeys, -1
// where the server does not apply.  (-1 on path 2 / with serve_fits: a plan without a kernel,
// a bug.)
inline int step_row(const StepPlan& pl, bool plain_rows) {
    if (pl.path != 2) return -1;
    StepKey k = pl.step.key;
    if (!plain_rows) k.wc = 0;
    return key_row(kStepKeys, k);
}
inline int serve_row(const StepPlan& pl) { return pl.serve_fits ? serve_row(pl.serve.key) : -1; }

// ---- mev_rollout_policy (k_rollout, mev_kernels.hip): the fused step in a loop with an MLP policy in
// front of it, one wave per env.  The compiled rows: X(TRAFFIC, NM, KM, P1, NC), each for both TAB --
// the three runtime layouts, which also run per-car sizes and written beam lists, and 8 agents x 64
// beams without traffic with the counts at compile time.
constexpr int kPolicyMaxWidth = 128;  // == MEV_POLICY_MAX_WIDTH
constexpr int kPolicyGroup = 8;       // agents per policy pass (the LDS rows are [k][8])
constexpr int kPolicyObsHead = 31;   // == OBS_HEAD (mev_world.h): the columns before the LiDAR block
#define MEV_ROLLOUT_KERNELS(X) \
    X(false, 0, MAXK, 0, 0)    \
    X(true, 0, 32, 0, 0)       \
    X(true, 0, 64, 0, 0)       \
    X(false, 8, MAXK, 64, 8)
constexpr int kRolloutRows = 4;
constexpr int kRolloutRowFixed = 3;  // the compile-time row
struct RolloutPlan {
    int row;                    // in MEV_ROLLOUT_KERNELS' order; -1: the shape is not supported
    unsigned grid, block, lds;  // one wave per env; the dynamic LDS, the policy's scratch included
    int pol_off;                // where in the dynamic LDS the policy's scratch starts
};
// obs_dim: the handle's D (<= 31 + 128); hidden: the policy's hidden widths summed (the scratch holds 8
// observation rows and 8 rows of each hidden layer).  The scratch lies in the step's LiDAR area, which
// is dead between sub-steps, growing the launch's LDS where the area is smaller; where that would pass
// a workgroup's 64 KB it lies at the start of the block instead (the car part's arrays are dead too).
inline RolloutPlan plan_rollout(StepShape s, int obs_dim, int hidden = 2 * 64) {
    RolloutPlan r{-1, 0, 0, 0, 0};
    s.step_kernel = 2;
    s.step_pack = s.step_split = 0;
    if (plan_step(s).path != 2 || obs_dim < kPolicyObsHead || obs_dim > kPolicyObsHead + kPolicyMaxWidth) return r;
    if (hidden < 1 || hidden > 2 * kPolicyMaxWidth) return r;
    const bool fixed = !s.traffic && !s.dims && s.N == 8 && s.R == 64 && s.lidar_slots == 64;
    const int npc_cap = s.K <= 32 ? 32 : 64;
    r.row = s.traffic ? (npc_cap == 32 ? 1 : 2) : fixed ? kRolloutRowFixed : 0;
    const unsigned dyn = fixed ? (unsigned)FixedLayout<8>::bytes : (unsigned)step_layout(s).bytes;
    const unsigned lidar = fixed ? (unsigned)FixedLayout<8>::lidar : (unsigned)step_layout(s).lidar;
    const unsigned stat = !s.traffic ? 0u : npc_cap == 32 ? (unsigned)sizeof(NpcLDST<32, true>) : (unsigned)sizeof(NpcLDST<64, true>);
    const unsigned need = (unsigned)(kPolicyGroup * (obs_dim + hidden)) * 4u;
    r.pol_off = (int)lds_al(lidar);
    if (stat + r.pol_off + need > 64u * 1024u) r.pol_off = 0;
    r.lds = dyn > r.pol_off + need ? dyn : r.pol_off + need;
    r.grid = (unsigned)s.E;
    r.block = WAVE;
    return r;
}

}  // namespace mev
