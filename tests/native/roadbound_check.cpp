// Host check of the LiDAR march's road bounds (csrc/mev_roadbound.h): the code
// the kernels ship, against the reference's road predicate.
//
//   1. safety: from a point p along a direction d, every probe p + d * (k * step),
//      k = 1 .. safe_steps(bound), is on screen and on the road at its truncated
//      pixel (p's own pixel on screen, the bounds' precondition) -- for road_safe, road_safe_uniform and road_entry_safe;
//   2. the march: lidar_body's march (mev_kernels.hip: the jump from the car
//      centre, LIDAR_NPR probes, then iterations of n probes and a jump) stops
//      at the index the reference's probe-by-probe march stops at, for the old
//      bound and for the entry bound in both orders (probes -> bound, and
//      bound -> jump -> probes), with the pooled pass's 2 probes per iteration
//      and a helper group's 12;
//   3. tightness: over all sampled beams the entry bound needs no more march
//      iterations than road_safe (printed; the test asserts the condition).
//
// The predicate is RoadGeometry::is_on_road (cpp/RoadGeometry.h:19-58, restated in
// oracle/marl_oracle.c:225-241) at integer pixels, as Lidar::update (cpp/Lidar.cpp:31-48)
// applies it: probe k stops the beam if its truncated pixel is off screen, or (k > 0)
// off the road.
//
// Samples (float32; lanes 2 and 3, so the road's half width is no constant): a
// strided sweep of the 0.25 px grid over the screen and a 30 px apron; points
// within 3 px of every grass edge and 4 px of the corner discs' rims; the beams
// of 64-, 96- and 128-beam fans at headings on a 1 degree grid; the exact axis
// directions (+-1, +-0).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <vector>

#include "mev_roadbound.h"

namespace {

constexpr int W = 750, S = 63;
constexpr float STP = 4.0f, INV_STP = 0.25f, CR = 84.0f, LANE_W = 42.0f;
constexpr int NPR = 2;  // LIDAR_NPR

struct World {
    float rw, rwm, ccen;
    explicit World(int lanes) : rw(lanes * LANE_W), rwm(rw - 1.5f), ccen(rw + CR) {}
};

bool on_road(const World& w, float x, float y) {  // RoadGeometry::is_on_road
    const float CX = W * 0.5f, CY = W * 0.5f, rw = w.rw, cr = CR, r2 = cr * cr;
    const float gx[4] = {CX - rw - cr, CX + rw + cr, CX - rw - cr, CX + rw + cr};
    const float gy[4] = {CY - rw - cr, CY - rw - cr, CY + rw + cr, CY + rw + cr};
    for (int k = 0; k < 4; ++k) {
        const float dx = x - gx[k], dy = y - gy[k];
        if (dx * dx + dy * dy <= r2) return false;
    }
    if ((x >= CX - rw && x <= CX + rw) || (y >= CY - rw && y <= CY + rw)) return true;
    if (x >= CX - rw - cr && x <= CX - rw && y >= CY - rw - cr && y <= CY - rw) return true;
    if (x >= CX + rw && x <= CX + rw + cr && y >= CY - rw - cr && y <= CY - rw) return true;
    if (x >= CX - rw - cr && x <= CX - rw && y >= CY + rw && y <= CY + rw + cr) return true;
    if (x >= CX + rw && x <= CX + rw + cr && y >= CY + rw && y <= CY + rw + cr) return true;
    return false;
}

// the reference's stop test of probe k of a beam from (cx, cy): 0 go on, 1 stop
bool probe_stops(const World& w, float cx, float cy, float dx, float dy, int k, float* fx, float* fy) {
    const float d = (float)k * STP;
    *fx = cx + dx * d;
    *fy = cy + dy * d;
    const int px = (int)*fx, py = (int)*fy;
    if (px < 0 || px >= W || py < 0 || py >= W) return true;
    return k > 0 && !on_road(w, (float)px, (float)py);
}

int safe_steps(float safe) { return safe >= STP ? (int)(safe * INV_STP) : 0; }

enum Bound { OLD, OLD_UNIFORM, ENTRY };

float bound(const World& w, Bound b, float fx, float fy, float dx, float dy) {
    const float idx = 1.0f / dx, idy = 1.0f / dy;
    const float iadx = mev::fabs_f(idx), iady = mev::fabs_f(idy);
    switch (b) {
        case OLD: return mev::road_safe(fx, fy, dx, dy, idx, idy, iadx, iady, w.rwm, w.ccen, CR);
        case OLD_UNIFORM: return mev::road_safe_uniform(fx, fy, dx, dy, idx, idy, iadx, iady, w.rwm, w.ccen, CR);
        default: return mev::road_entry_safe(fx, fy, dx, dy, idx, idy, iadx, iady, w.rwm, w.ccen, CR);
    }
}

int brute(const World& w, float cx, float cy, float dx, float dy) {
    float fx, fy;
    for (int k = 0; k < S; ++k)
        if (probe_stops(w, cx, cy, dx, dy, k, &fx, &fy)) return k;
    return S;
}

// lidar_body's march.  b1: phase 1's bound from the car centre; b2: phase 2's;
// pre: phase 2 jumps by the bound at the beam's last tested probe before its
// probes (else after them, from the last of them); n2: probes per phase-2
// iteration.  Returns the stop index (S: none); *iters: phase-2 iterations.
int march(const World& w, Bound b1, Bound b2, bool pre, int n2, float cx, float cy, float dx, float dy, int* iters) {
    *iters = 0;
    float fx = cx, fy = cy;
    const int px = (int)cx, py = (int)cy;
    const bool on = px >= 0 && px < W && py >= 0 && py < W;
    int k = on ? 1 + safe_steps(bound(w, b1, cx, cy, dx, dy)) : 0;
    for (int t = 0; t < NPR; ++t, ++k) {
        if (k >= S) return S;
        if (probe_stops(w, cx, cy, dx, dy, k, &fx, &fy)) return k;
    }
    for (;;) {  // phase 2: k = the next probe to test, (fx, fy) = the point of probe k - 1
        if (k >= S) return S;
        ++*iters;
        if (pre) {
            k += safe_steps(bound(w, b2, fx, fy, dx, dy));
            if (k >= S) return S;
        }
        for (int t = 0; t < n2; ++t, ++k) {
            if (k >= S) return S;
            if (probe_stops(w, cx, cy, dx, dy, k, &fx, &fy)) return k;
        }
        if (!pre) k += safe_steps(bound(w, b2, fx, fy, dx, dy));
    }
}

struct Stats {
    long long beams = 0, unsafe = 0, wrong = 0;
    long long it_old = 0, it_a = 0, it_b = 0;  // phase-2 iterations at 2 probes: old, entry (a), entry (b)
    long long q_old = 0, q_a = 0;              // beams phase 1 leaves to phase 2
    void add(const Stats& o) {
        beams += o.beams; unsafe += o.unsafe; wrong += o.wrong;
        it_old += o.it_old; it_a += o.it_a; it_b += o.it_b; q_old += o.q_old; q_a += o.q_a;
    }
};

std::atomic<int> g_reports{0};

void check_beam(const World& w, float cx, float cy, float dx, float dy, Stats& st) {
    ++st.beams;
    // 1. safety of each bound from this point (the bounds' precondition: its own pixel is on
    //    screen, as the car centre and every probe the march jumps from are)
    const int px0 = (int)cx, py0 = (int)cy;
    const bool on0 = px0 >= 0 && px0 < W && py0 >= 0 && py0 < W;
    for (Bound b : {OLD, OLD_UNIFORM, ENTRY}) {
        if (!on0) break;
        const int n = safe_steps(bound(w, b, cx, cy, dx, dy));
        for (int k = 1; k <= n && k < 4 * S; ++k) {
            const float d = (float)k * STP, fx = cx + dx * d, fy = cy + dy * d;
            const int px = (int)fx, py = (int)fy;
            const bool ok = px >= 0 && px < W && py >= 0 && py < W && on_road(w, (float)px, (float)py);
            if (!ok) {
                ++st.unsafe;
                if (g_reports.fetch_add(1) < 20)
                    printf("UNSAFE bound %d rw %.0f p (%.9g, %.9g) d (%.9g, %.9g): %d safe steps, probe %d at pixel "
                           "(%d, %d) is off\n", (int)b, w.rw, cx, cy, dx, dy, n, k, px, py);
                break;
            }
        }
    }
    // 2. the march
    const int want = brute(w, cx, cy, dx, dy);
    int it;
    struct V { Bound b1, b2; bool pre; int n2; };
    const V vs[] = {{OLD_UNIFORM, OLD, false, 2}, {ENTRY, ENTRY, false, 2}, {OLD_UNIFORM, ENTRY, true, 2},
                    {OLD_UNIFORM, OLD, false, 12}, {ENTRY, ENTRY, false, 12}, {OLD_UNIFORM, ENTRY, true, 12}};
    for (int v = 0; v < 6; ++v) {
        const int got = march(w, vs[v].b1, vs[v].b2, vs[v].pre, vs[v].n2, cx, cy, dx, dy, &it);
        if (got != want) {
            ++st.wrong;
            if (g_reports.fetch_add(1) < 20)
                printf("WRONG STOP variant %d rw %.0f p (%.9g, %.9g) d (%.9g, %.9g): got %d want %d\n", v, w.rw, cx, cy,
                       dx, dy, got, want);
        }
        if (v == 0) { st.it_old += it; st.q_old += it > 0; }
        if (v == 1) { st.it_a += it; st.q_a += it > 0; }
        if (v == 2) st.it_b += it;
    }
}

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    float uni(float a, float b) { return a + (b - a) * ((float)(next() & 0xffffff) / 16777216.0f); }
};

void fan_dir(float h, int R, int i, float* dx, float* dy) {  // Lidar.cpp:24-26 with a 360 degree fan
    const float rel = (-180.0f + (float)i * (360.0f / (float)(R - 1))) * (float)(M_PI / 180.0);
    float sn, cs;
    mev::sincosf(h + rel, &sn, &cs);
    *dx = cs;
    *dy = -sn;
}

// edge poses: within 3 px of a grass edge (half of them pixel-aligned) or 4 px of a disc rim
void edge_point(const World& w, Rng& r, float* x, float* y) {
    const float sx = (r.next() & 1) ? 1.0f : -1.0f, sy = (r.next() & 1) ? 1.0f : -1.0f;
    float u, v;
    const int mode = r.next() % 5;
    if (mode == 0) { u = w.rw + r.uni(-3, 3); v = r.uni(0, 400); }
    else if (mode == 1) { v = w.rw + r.uni(-3, 3); u = r.uni(0, 400); }
    else if (mode == 2) { u = w.ccen + r.uni(-3, 3); v = r.uni(w.rw - 3, w.ccen + 3); }
    else if (mode == 3) { v = w.ccen + r.uni(-3, 3); u = r.uni(w.rw - 3, w.ccen + 3); }
    else {
        const float a = r.uni(0, 6.2831853f), rad = CR + r.uni(-4, 4);
        u = w.ccen + rad * cosf(a);
        v = w.ccen + rad * sinf(a);
    }
    *x = 375.0f + sx * u;
    *y = 375.0f + sy * v;
    if (r.next() & 1) { *x = rintf(*x); *y = rintf(*y); }
}

void worker(int tid, int nthreads, Stats* out) {
    Stats st;
    for (int lanes = 2; lanes <= 3; ++lanes) {
        const World w(lanes);
        Rng r{0x9e3779b97f4a7c15ull * (uint64_t)(tid + 1) + (uint64_t)lanes};
        // (i) the 0.25 px grid over [-30, 780)^2, strided; a 64-beam fan at a 1 degree heading each,
        //     and the exact axis directions
        const long long G = 3240, total = G * G;
        long long n = 0;
        for (long long i = 7 + 499LL * tid; i < total; i += 499LL * nthreads, ++n) {
            const float x = -30.0f + 0.25f * (float)(i % G), y = -30.0f + 0.25f * (float)(i / G);
            const float h = (float)((int)(r.next() % 360) - 180) * (float)(M_PI / 180.0);
            for (int b = 0; b < 64; ++b) {
                float dx, dy;
                fan_dir(h, 64, b, &dx, &dy);
                check_beam(w, x, y, dx, dy, st);
            }
            if (n % 4 == 0) {
                const float ax[8][2] = {{1.0f, 0.0f}, {1.0f, -0.0f}, {-1.0f, 0.0f}, {-1.0f, -0.0f},
                                        {0.0f, 1.0f}, {-0.0f, 1.0f}, {0.0f, -1.0f}, {-0.0f, -1.0f}};
                for (auto& a : ax) check_beam(w, x, y, a[0], a[1], st);
            }
        }
        // (ii) every beam of 64-, 96- and 128-beam fans, headings on the 1 degree grid, from edge poses
        for (int hd = -180 + tid; hd < 180; hd += nthreads) {
            const float h = (float)hd * (float)(M_PI / 180.0);
            for (int R : {64, 96, 128}) {
                for (int rep = 0; rep < 6; ++rep) {
                    float x, y;
                    edge_point(w, r, &x, &y);
                    for (int b = 0; b < R; ++b) {
                        float dx, dy;
                        fan_dir(h, R, b, &dx, &dy);
                        check_beam(w, x, y, dx, dy, st);
                    }
                }
            }
        }
        // (iii) edge poses with free headings (40 % axis-aligned: the fan's own rounding of the axes)
        for (int i = 0; i < 6000; ++i) {
            float x, y;
            edge_point(w, r, &x, &y);
            float h = r.uni(-3.1415927f, 3.1415927f);
            if (r.next() % 10 < 4) h = (float)((int)(r.next() % 5) - 2) * (float)(M_PI / 2.0);
            for (int b = 0; b < 64; b += 1 + (int)(r.next() % 3)) {
                float dx, dy;
                fan_dir(h, 64, b, &dx, &dy);
                check_beam(w, x, y, dx, dy, st);
            }
        }
    }
    *out = st;
}

}  // namespace

int main() {
    const int nthreads = 4;
    std::vector<Stats> parts(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t) th.emplace_back(worker, t, nthreads, &parts[t]);
    for (auto& t : th) t.join();
    Stats st;
    for (auto& p : parts) st.add(p);
    const double n = (double)st.beams;
    printf("%lld beams: %lld unsafe bounds, %lld wrong stops\n", st.beams, st.unsafe, st.wrong);
    printf("beams left to phase 2: road_safe %.4f, entry bound in phase 1 %.4f\n", st.q_old / n, st.q_a / n);
    printf("mean phase-2 iterations per beam: road_safe %.4f, entry bound (a) %.4f, (b) %.4f\n", st.it_old / n,
           st.it_a / n, st.it_b / n);
    bool ok = st.unsafe == 0 && st.wrong == 0;
    if (st.it_a > st.it_old || st.it_b > st.it_old) {
        printf("TIGHTNESS: the entry bound needs more iterations than road_safe\n");
        ok = false;
    }
    printf(ok ? "ROADBOUND OK\n" : "ROADBOUND FAILED\n");
    return ok ? 0 : 1;
}
