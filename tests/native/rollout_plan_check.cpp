// plan_rollout (csrc/mev_plan.h): the k_rollout row and launch of mev_rollout_policy for named shapes,
// the shapes it refuses, and over a grid of shapes the launch's invariants -- supported exactly where the
// fused step kernel holds the shape and obs_dim <= 31 + 128; the policy's scratch inside the launch's LDS,
// 16-byte aligned; static + dynamic LDS within a workgroup's 64 KB; never less LDS than the step needs.
//
//   rollout_plan_check              check everything, print ROLLOUT PLAN OK
#include <cstdio>
#include <initializer_list>

#include "mev_plan.h"

using namespace mev;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED line %d: %s\n", __LINE__, #c);               \
            ++fails;                                                    \
        }                                                               \
    } while (0)

static StepShape shape(int E, int N, int R, int K, int D, int traffic, int dims) {
    StepShape s{};
    s.E = E; s.N = N; s.R = R; s.K = K;
    s.lidar_slots = R < D - 31 ? R : D - 31;
    s.traffic = traffic; s.dims = dims;
    return s;
}

static unsigned npc_static(const StepShape& s) {
    return !s.traffic ? 0u : s.K <= 32 ? (unsigned)sizeof(NpcLDST<32, true>) : (unsigned)sizeof(NpcLDST<64, true>);
}

int main() {
    // ---- the rows of the shapes the GPU tests run
    CHECK(plan_rollout(shape(5, 3, 8, 32, 127, 0, 0), 127, 32).row == 0);
    CHECK(plan_rollout(shape(4, 8, 64, 32, 127, 0, 0), 127).row == kRolloutRowFixed);
    CHECK(plan_rollout(shape(4096, 8, 64, 32, 95, 0, 0), 95).row == kRolloutRowFixed);
    CHECK(plan_rollout(shape(4, 8, 64, 32, 127, 0, 1), 127).row == 0);   // per-car sizes: the runtime layout
    CHECK(plan_rollout(shape(4, 8, 64, 32, 63, 0, 0), 63).row == 0);     // 32 of the 64 beams in the row
    CHECK(plan_rollout(shape(4, 8, 96, 32, 127, 0, 0), 127).row == 0);
    CHECK(plan_rollout(shape(4, 7, 64, 32, 127, 0, 0), 127).row == 0);
    CHECK(plan_rollout(shape(4, 1, 16, 32, 127, 1, 0), 127, 32).row == 1);
    CHECK(plan_rollout(shape(4, 1, 16, 16, 127, 1, 0), 127, 32).row == 1);
    CHECK(plan_rollout(shape(4, 1, 16, 64, 127, 1, 0), 127, 32).row == 2);
    CHECK(plan_rollout(shape(4096, 1, 64, 33, 95, 1, 1), 95).row == 2);
    {
        // the forced kernel choice of the handle does not matter: the call has its own kernel
        StepShape s = shape(4, 8, 64, 32, 127, 0, 0);
        s.step_kernel = 1; s.step_pack = 4; s.step_split = 2;
        CHECK(plan_rollout(s, 127).row == kRolloutRowFixed);
        const RolloutPlan r = plan_rollout(s, 127);
        CHECK(r.grid == 4u && r.block == (unsigned)WAVE);
        CHECK(r.pol_off == FixedLayout<8>::lidar);
        CHECK(r.lds == (unsigned)(FixedLayout<8>::lidar + 8 * (127 + 128) * 4));  // (the scratch outgrows the LiDAR area)
        const RolloutPlan f = plan_rollout(shape(4096, 8, 64, 32, 95, 0, 0), 95);
        CHECK(f.lds == (unsigned)FixedLayout<8>::bytes);  // 95-64-64: inside the LiDAR area, no more LDS than the step
    }
    // ---- refused
    CHECK(plan_rollout(shape(2, 1, 8, 32, 31 + 129, 0, 0), 31 + 129).row == -1);
    CHECK(plan_rollout(shape(2, 1, 8, 32, 31 + 128, 0, 0), 31 + 128).row == 0);
    {
        StepShape big = shape(2, 64, 8, 64, 127, 1, 0);  // 64 egos + 64 NPC slots: the fused LDS passes 64 KB
        big.step_kernel = 2;
        CHECK(plan_step(big).path == 0);
        CHECK(plan_rollout(big, 127).row == -1);
    }
    CHECK(plan_rollout(shape(2, 1, 8, 32, 127, 0, 0), 127, 0).row == -1);
    CHECK(plan_rollout(shape(2, 1, 8, 32, 127, 0, 0), 127, 257).row == -1);
    // ---- the grid
    int supported = 0, moved = 0, grown = 0;
    const int Ns[] = {1, 2, 3, 8, 12, 33, 64}, Rs[] = {8, 16, 64, 96, 128, 200}, Ks[] = {16, 32, 64};
    const int Ds[] = {39, 95, 127, 159, 160}, Hs[] = {1, 32, 128, 256};
    for (int N : Ns) for (int R : Rs) for (int K : Ks) for (int traffic = 0; traffic < 2; ++traffic)
    for (int dims = 0; dims < 2; ++dims) for (int D : Ds) for (int H : Hs) for (int E : {3, 4096}) {
        StepShape s = shape(E, N, R, K, D, traffic, dims);
        const RolloutPlan r = plan_rollout(s, D, H);
        s.step_kernel = 2;
        const StepPlan sp = plan_step(s);
        const bool want = sp.path == 2 && D <= 31 + kPolicyMaxWidth;
        CHECK((r.row >= 0) == want);
        if (r.row < 0) continue;
        ++supported;
        const unsigned need = 8u * (unsigned)(D + H) * 4u;
        CHECK(r.row < kRolloutRows && r.grid == (unsigned)E && r.block == (unsigned)WAVE);
        CHECK((r.row == 1 || r.row == 2) == (traffic != 0));
        CHECK(r.pol_off % 16 == 0 && (unsigned)r.pol_off + need <= r.lds);
        CHECK(npc_static(s) + r.lds <= 64u * 1024u);
        CHECK(r.lds >= (r.row == kRolloutRowFixed ? (unsigned)FixedLayout<8>::bytes : (unsigned)step_layout(s).bytes));
        moved += r.pol_off == 0;
        grown += r.lds > (unsigned)step_layout(s).bytes && r.row != kRolloutRowFixed;
    }
    printf("supported %d, scratch at the block's start %d, LDS grown %d\n", supported, moved, grown);
    CHECK(supported > 1000 && grown > 0);
    if (fails) return 1;
    printf("ROLLOUT PLAN OK\n");
    return 0;
}
