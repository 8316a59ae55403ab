// mev_refworld.h — the world a handle's SimParams describe, derived in one place:
// world_consts() is what mev_create fills SimParams from, kRefWorld is the same
// derivation of mev_config_default's values (the reference's three-lane
// intersection and its 250 px / 4 px LiDAR) at compile time, and StepWorld / StepRows are
// how the step kernels read those fields: from SimParams / Outputs, or -- in the
// instantiations plan_step chooses for a handle whose world is kRefWorld and whose
// observation rows are plain -- as constants that need no scalar register.
#pragma once

#include "mev_world.h"

namespace mev {

// mev_config_default's world (cpp/IntersectionEnv.cpp:113-116)
constexpr int kRefNumLanes = 3;
constexpr float kRefLidarMaxDist = 250.0f;
constexpr float kRefLidarStep = 4.0f;

// more march probes than this per beam: mev_create refuses the configuration
constexpr int kMaxMarchProbes = 1 << 20;

struct WorldConsts {
    int32_t num_lanes;
    int32_t irw;        // road half width in px (L*42)
    int32_t line_stop;  // LineMask stop offset int(L*42) + 84 (LineMask.cpp:52-54)
    float rw;           // road half width (RoadGeometry.h:16)
    float lidar_max, lidar_step;
    float lidar_inv;      // 1 / max_dist (Lidar.cpp:94)
    int32_t lidar_steps;  // march probes with dist < max_dist, as Lidar.cpp:33 accumulates dist
                          // (counted up to kMaxMarchProbes + 1)
    bool dist_exact;      // every accumulated probe distance equals k * step: no table needed
};

constexpr WorldConsts world_consts(int num_lanes, float lidar_max_dist, float lidar_step) {
    WorldConsts w{};
    w.num_lanes = num_lanes;
    w.irw = int(num_lanes * int(LANE_WIDTH_PX));
    w.line_stop = int(num_lanes * int(LANE_WIDTH_PX)) + int(CORNER_RADIUS);
    w.rw = num_lanes * LANE_WIDTH_PX;
    w.lidar_max = lidar_max_dist;
    w.lidar_step = lidar_step;
    w.lidar_inv = (lidar_max_dist > 0.0f) ? (1.0f / lidar_max_dist) : 0.0f;
    w.dist_exact = true;
    int n = 0;
    for (float dist = 0.0f; dist < lidar_max_dist && n <= kMaxMarchProbes; dist += lidar_step) {
        if (dist != float(n) * lidar_step) w.dist_exact = false;
        ++n;
    }
    w.lidar_steps = n;
    return w;
}

constexpr WorldConsts kRefWorld = world_consts(kRefNumLanes, kRefLidarMaxDist, kRefLidarStep);
static_assert(kRefWorld.dist_exact, "the reference's LiDAR step sums exactly: its handles read no distance table");

// IntersectionEnv.cpp:22 (the same for every world; a constant operand folds it)
MEV_HD float world_max_progress() { return hypotf(float(WIDTH), float(HEIGHT)); }

#if defined(__HIPCC__)
#define MEV_CONST_FIELD(T, name, value)                      \
    template <class P>                                       \
    static __device__ __forceinline__ T name(const P& p) {   \
        if constexpr (WC) return (value);                    \
        else return p.name;                                  \
    }
// How the bodies of k_step read the fields of SimParams that the world fixes.  WC: the handle's
// world is kRefWorld -- every accessor is a constant; otherwise each reads its field.
// (SimParams::dist_tab is not among them: null in this world, but LiDAR phase 3 keeps its
// run-time test of the pointer -- with it folded away the metric's kernel is scheduled into
// 116 VGPRs instead of 56 and runs 3.6 us slower)
template <bool WC>
struct StepWorld {
    MEV_CONST_FIELD(int32_t, irw, kRefWorld.irw)
    MEV_CONST_FIELD(int32_t, line_stop, kRefWorld.line_stop)
    MEV_CONST_FIELD(float, rw, kRefWorld.rw)
    MEV_CONST_FIELD(float, lidar_max, kRefWorld.lidar_max)
    MEV_CONST_FIELD(float, lidar_step, kRefWorld.lidar_step)
    MEV_CONST_FIELD(float, lidar_inv, kRefWorld.lidar_inv)
    MEV_CONST_FIELD(int32_t, lidar_steps, kRefWorld.lidar_steps)
    MEV_CONST_FIELD(float, max_progress, world_max_progress())
    MEV_CONST_FIELD(int32_t, beam_cull, 1)
};
// ... and the layout of the observation rows (SimParams::lidar_slots, Outputs).  WC: plain float
// rows of 31 + P1 columns, each of the P1 beams in the observation, and neither compact gather
// format (their code is not compiled in).
template <bool WC, int P1>
struct StepRows {
    static_assert(!WC || P1 >= 64, "constant rows need the beam count at compile time");
    MEV_CONST_FIELD(int32_t, lidar_slots, P1)
    MEV_CONST_FIELD(int32_t, obs_ld, OBS_HEAD + P1)
    MEV_CONST_FIELD(uint8_t*, lidar_u8, nullptr)
    MEV_CONST_FIELD(uint8_t*, state, nullptr)
};
#undef MEV_CONST_FIELD
#endif

}  // namespace mev
