// mev_layout.h — the LDS geometry of the step kernels: pure arithmetic, no HIP.
// The kernels (mev_kernels.hip) carve their LDS by it, the host plan (mev_plan.h)
// sizes and chooses the launches by it, and host-only code can include it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)  // a plain C++ compiler
#define __host__
#define __device__
#endif

namespace mev {

constexpr int WAVE = 64;
constexpr int MAXN = 64;
constexpr int MAXK = 64;

// capacity KM NPC slots (k_cars / k_reset: MAXK; the fused k_step: the smallest
// of 32 / 64 that holds the handle's max_npcs, so that the NPC arrays leave room
// in the wave's LDS for a LiDAR pool).  DIMS: with each NPC's length / width (last).
template <int KM, bool DIMS = false>
struct NpcLDST {
    static constexpr bool kDims = DIMS;
    static constexpr int kCap = KM;
    float x[KM], y[KM], v[KM], h[KM], c[KM], s[KM], acc[KM], steer[KM];
    int32_t pidx[KM], route[KM], intent[KM];
    uint8_t alive[KM];
    union {
        struct {  // the car corners (collision phase, after the controller)
            float cx[KM][4], cy[KM][4];
        };
        struct {  // the controller's round-A states (npc_phase part 2), dead once committed
            float xn[KM], yn[KM], vn[KM], hn[KM], accn[KM], steern[KM], cn[KM], sn[KM];
            float mdcn[KM];  // the round-A state's distance to the centre
        };
    };
    unsigned long long col[KM];
    // the controller's parallel rounds: throttles of round A / B, ghost-scan candidates
    // (others that passed the filters) and which of them k must yield to, new path index
    float thr_a[KM], thr_b[KM];
    unsigned long long em[KM], ym[KM];      // this round's filtered others / yields (scans)
    unsigned long long em_a[KM], ym_a[KM];  // round A's
    float mc_a[KM];                         // round A's conflict distance (< 0: none)
    int32_t pidxn[KM];
    // the controller's per-NPC terms that depend on its own start-of-step state only
    int32_t pidx0[KM];          // after the first update_path_index of its turn
    float nsteer[KM], ntan[KM];  // Car::update's new steering angle and its tangent
    float accb[KM], mdc[KM];  // cruise throttle, distance to the centre
    float endx[KM], endy[KM];  // the route's last point (arrival test)
    // Per-NPC length / width (Car::length / Car::width), after every other array: only in
    // the kernels that can run a handle with per-car sizes (k_cars, k_reset, k_step<NM =
    // 0>); zero-length elsewhere, so the compile-time layouts keep their size
    float len[DIMS ? KM : 0], wid[DIMS ? KM : 0];
};

// LDS path windows of the car part's first pass (k_step, no traffic): 4 x 1 KB + 1 KB
constexpr int kWinBytes = 5 * 1024;

__host__ __device__ constexpr size_t lds_al(size_t b) { return (b + 15) & ~size_t(15); }

// (P below: SimParams, or the host plan's StepShape -- the fields N, R, K, traffic)
// NPC slots that need obstacle entries in k_cars' LDS (none without traffic)
template <class P>
__host__ __device__ inline int cars_k(const P& p) { return p.traffic ? p.K : 0; }

// dims: the handle has cars of other sizes (two more per-ego arrays at the end)
__host__ __device__ constexpr size_t cars_lds_bytes(int N, int K, bool dims = false) {
    const size_t n = (size_t)N, ob = (size_t)(N + K);
    return 22 * lds_al(n * 4) + 2 * lds_al(n * 16) + 3 * lds_al(n * 4) + 4 * lds_al(n) + lds_al(n * 8) +
           lds_al(ob * 16) + 3 * lds_al(ob * 4) + lds_al(n * 16) + (dims ? 2 * lds_al(n * 4) : 0);
}

struct LidarLayout {
    int ag, dir, res, seg_jo, seg_rg, seg_bx, queue, scr, bytes;
};

template <class P>
__host__ __device__ inline int lidar_cand_max(const P& p) { return p.N - 1 + (p.traffic ? p.K : 0); }

// with_bx: a per-segment copy of the obstacle box (k_lidar, whose boxes are in
// HBM); k_step reads them from its own LDS obstacle table instead.
// beams: capacity of the beam arrays (>= G * R).
__host__ __device__ constexpr LidarLayout lidar_layout_beams(int G, int beams, int cmax, bool with_bx) {
    LidarLayout L{};
    const int C = G * cmax;
    int off = 0;
    L.ag = off; off += G * 16;
    L.dir = off; off += beams * 8;
    L.res = off; off += beams * 4;
    off = (off + 15) & ~15;
    L.seg_rg = off; off += C * 16;
    L.seg_bx = off; off += with_bx ? C * 16 : 0;
    L.seg_jo = off; off += C * 4;
    L.queue = L.seg_rg;
    if (off < L.queue + beams * 2) off = L.queue + beams * 2;
    off = (off + 15) & ~15;
    L.scr = off; off += WAVE * 4;  // the car phase's segment lookup (3c)
    L.bytes = (off + 15) & ~15;
    return L;
}
__host__ __device__ inline LidarLayout lidar_layout(int G, int R, int cmax, bool with_bx = true) {
    return lidar_layout_beams(G, G * R, cmax, with_bx);
}

// Agents per LiDAR pool in k_step: the env's N agents in the fewest pools of at
// most 512 beams, balanced (all N in one pool at config 3; 8 x 96 beams as 4 + 4
// agents, 384 beams each, not 5 + 3: each pool's march ends on its longest beams,
// and 4 agents of 96 beams fill six whole 64-lane chunks in phase 1).
__host__ __device__ constexpr int step_pool_n(int N, int R) {
    int g = 512 / (R > 0 ? R : 1);
    g = g < 1 ? 1 : g;
    if (g >= N) return N;
    const int pools = (N + g - 1) / g;
    return (N + pools - 1) / pools;
}
template <class P>
__host__ __device__ inline int step_pool(const P& p) { return step_pool_n(p.N, p.R); }

// LDS of one k_step wave: cars LDS, the staged heads [N][31], the beam offsets
// [R], the env flags [8], then the LiDAR pool of step_pool(p) agents.
struct StepLayout {
    int head, rel, envw, lidar, bytes;
};
template <class P>
__host__ __device__ inline StepLayout step_layout(const P& p) {
    StepLayout L;
    int off = (int)lds_al(cars_lds_bytes(p.N, cars_k(p), true));  // (k_step<NM = 0> keeps the car sizes)
    L.head = off;  // (no staged heads: the car part writes its rows' heads itself)
    L.rel = off; off += (int)lds_al((size_t)p.R * 4);
    L.envw = off; off += 32;
    L.lidar = off; off += lidar_layout(step_pool(p), p.R, lidar_cand_max(p), false).bytes;
    L.bytes = off;
    return L;
}

// Compile-time LDS geometry (NM > 0): every array sized for its capacity --
// N <= NM agents, R <= kFixedRays beams per agent, one LiDAR pool of <= 512
// beams, no NPCs -- so each LDS address is a constant offset from the wave's
// base instead of a runtime pointer held in an SGPR.  The ~40 runtime LDS
// pointers of the NM = 0 layout made k_step spill 131 SGPRs into VGPR lanes
// (a v_readlane per reload).
constexpr int kFixedRays = 128;
constexpr int kPoolBeams = 512;
template <int NM, int KM = 0>
struct FixedLayout {
    static_assert(NM >= 1 && NM <= 64, "agents per env");
    static constexpr int beams = NM * kFixedRays < kPoolBeams ? NM * kFixedRays : kPoolBeams;
    static constexpr int cars = (int)lds_al(cars_lds_bytes(NM, KM));
    static constexpr int rel = cars;
    static constexpr int envw = rel + kFixedRays * 4;
    static constexpr int lidar = envw + 32;
    static constexpr LidarLayout lay = lidar_layout_beams(NM, beams, NM - 1 + KM, false);
    static constexpr int bytes = lidar + lay.bytes;
};
// The 8-slot layout's car phase keeps one segment per lane (lidar_body, SEGL): seg_rg int4[64]
// from lay.seg_rg, 8 entries past the C = 56 the layout counts.  They lie in seg_jo's words,
// which that path does not use, and end before scr, which it does.
static_assert(FixedLayout<8>::lay.seg_bx == FixedLayout<8>::lay.seg_jo &&
                  FixedLayout<8>::lay.seg_rg + WAVE * 16 <= FixedLayout<8>::lay.scr,
              "segments by lane: 64 ranges between seg_rg and scr");

// the traffic early split: kTsplitEnvs envs (car waves) + one LiDAR wave per workgroup,
// kTsplitWpe waves per SIMD (config 4: 4096 envs -> 6144 waves on 1024 SIMDs).  Two envs,
// not four: the LiDAR wave's march of its egos' beams, which the light envs' car waves wait
// for at barrier H, halves -- config 4 148.4 -> 150.8 M, 1024 / 2048 / 3072 envs 2-4 %
// faster (profiles/r6_ab_ts2_*.txt; variant builds ts2* via MEV_TSPLIT_ENVS)
#ifndef MEV_TSPLIT_ENVS
#define MEV_TSPLIT_ENVS 2
#endif
constexpr int kTsplitEnvs = MEV_TSPLIT_ENVS;
constexpr int kTsplitRays = kFixedRays;  // LiDAR pool beams per env

}  // namespace mev
