// plan_step (csrc/mev_plan.h) for handles whose world is the reference's (StepShape::world):
// over the grid of step_plan_check.cpp, with the member set,
//   - every chosen key has a kernel row (and k_serve's row lookup drops the new field),
//   - the plan is the member-0 plan in everything but the key's wc,
//   - wc is set exactly where a specialised kernel exists: one wave per env, 8 agents at
//     compile time, 64 or 128 beams at compile time, no traffic, every car 54 x 24.
// Prints STEP PLAN WORLD OK.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "mev_plan.h"

using namespace mev;

// step_plan_check.cpp's grid: every threshold of the policy from both sides
static const int kE[] = {1, 16, 48, 63, 64, 65, 100, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192,
                         8193, 16384, 16385};
static const int kN[] = {1, 2, 3, 4, 5, 8, 9, 16, 64};
static const int kR[] = {16, 63, 64, 65, 96, 127, 128, 129, 256, 512, 2048, 4096};
static const int kTraffic[][2] = {{0, 0}, {0, 64}, {1, 16}, {1, 32}, {1, 33}, {1, 64}};  // traffic, max_npcs
static const int kKernel[] = {0, 1, 2}, kPack[] = {0, 1, 2, 4, 8}, kSplit[] = {0, 1, 2, 3};

static int bad = 0;
static long shapes = 0, chosen = 0;

static void fail(const StepShape& s, const char* what) {
    if (++bad <= 20)
        printf("%s: E %d N %d R %d K %d slots %d traffic %d dims %d kernel %d pack %d split %d\n", what, s.E, s.N, s.R,
               s.K, s.lidar_slots, s.traffic, s.dims, s.step_kernel, s.step_pack, s.step_split);
}

static bool same_launch(const StepLaunch& a, const StepLaunch& b, bool but_wc) {
    StepKey ka = a.key, kb = b.key;
    if (but_wc) ka.wc = kb.wc = 0;
    return ka == kb && a.grid == b.grid && a.block == b.block && a.lds == b.lds;
}

static void check(StepShape s) {
    s.world = 0;
    const StepPlan p0 = plan_step(s);
    s.world = 1;
    const StepPlan p1 = plan_step(s);
    ++shapes;
    if (p0.step.key.wc != 0 || p0.serve.key.wc != 0) fail(s, "wc set without the world");
    if (p0.path != p1.path || p0.pack != p1.pack || p0.split != p1.split || p0.serve_fits != p1.serve_fits ||
        !same_launch(p0.step, p1.step, true) || !same_launch(p0.serve, p1.serve, false))
        fail(s, "the plan differs in more than wc");
    if (p1.path == 2 && key_row(kStepKeys, p1.step.key) < 0) fail(s, "no kernel row");
    if (p1.serve_fits && serve_row(p1.serve.key) < 0) fail(s, "no k_serve row");
    const StepKey& k = p1.step.key;
    const bool special = p1.path == 2 && !k.traffic && !s.dims && k.nm == 8 && k.pk == 1 && !k.split && !k.esplit &&
                         k.nc == 8 && (k.p1 == 64 || k.p1 == 128);
    if ((k.wc != 0) != special) fail(s, special ? "wc not set at a specialised shape" : "wc set without a specialised row");
    if (k.wc != 0 && k.wc != 1) fail(s, "wc is 0 or 1");
    if (k.wc) {
        ++chosen;
        if (s.N != 8 || (s.R != 64 && s.R != 128) || s.lidar_slots != s.R) fail(s, "wc at another shape than 8 x 64 / 128");
    }
}

int main() {
    for (int kernel : kKernel)
        for (int pack : kPack)
            for (int split : kSplit)
                for (const auto& t : kTraffic)
                    for (int dims = 0; dims < 2; ++dims)
                        for (int E : kE)
                            for (int N : kN)
                                for (int R : kR)
                                    for (int slots : {R, R - 1})
                                        check(StepShape{E, N, R, t[1], slots, t[0], dims, kernel, pack, split});
    // the metric's shape and config 5's take the specialised kernels; the same shapes in two waves do not
    for (int R : {64, 128}) {
        StepShape s{4096, 8, R, 64, R, 0, 0, 0, 0, 0, 1};
        const StepPlan pl = plan_step(s);
        const StepKey want{false, 8, MAXK, 1, false, false, R, 8, 1};
        if (pl.path != 2 || !(pl.step.key == want)) fail(s, "the metric's shapes");
        s.E = 64;
        if (plan_step(s).step.key.wc) fail(s, "two waves per env");
        s.step_split = 1;
        if (!(plan_step(s).step.key == want)) fail(s, "64 envs, the split off");
    }
    // k_serve's lookup drops the field
    if (serve_row(StepKey{false, 8, MAXK, 1, true, false, 64, 8, 1}) != serve_row(StepKey{false, 8, MAXK, 1, true, false, 64, 8, 0}))
        ++bad, printf("serve_row keeps wc\n");
    if (!chosen) ++bad, printf("no shape of the grid chose a specialised kernel\n");
    if (bad) {
        printf("%d failures over %ld shapes\n", bad, shapes);
        return 1;
    }
    printf("STEP PLAN WORLD OK (%ld shapes, %ld with wc)\n", shapes, chosen);
    return 0;
}
