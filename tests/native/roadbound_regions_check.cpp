// Host check of road_entry_safe_uniform (csrc/mev_roadbound.h): from a start point every lane shares
// it branches on the point's road region (the centre cross, a vertical arm, a horizontal arm, anything
// else) and must return the bits road_entry_safe returns at the same arguments.
//
// Origins, for roads of 2, 3 and 4 lanes: a 12.5 px lattice over the screen, and per axis the
// coordinates at which |r| = |p - 375| equals rwm, sqm and 0, each with the floats one ulp either side
// (the region tests are comparisons with rwm; sqm and 0 are where the general form's own selects turn).
// Directions: 4096 evenly spaced angles, and the eight directions with a zero or negative-zero
// component (infinite reciprocals).  Prints how many origins fell into each case; each must occur.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <thread>
#include <vector>

#include "mev_roadbound.h"

namespace {

constexpr float CR = 84.0f, LANE_W = 42.0f;
constexpr int NANG = 4096;

struct Dir { float dx, dy, iadx, iady; };

uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

std::vector<float> axis_coords(float rwm, float sqm) {
    std::vector<float> v;
    for (int i = 0; i <= 60; ++i) v.push_back(12.5f * (float)i);
    const float marks[5] = {375.0f - sqm, 375.0f - rwm, 375.0f, 375.0f + rwm, 375.0f + sqm};
    for (float m : marks) {
        v.push_back(nextafterf(m, -1.0e9f));
        v.push_back(m);
        v.push_back(nextafterf(m, 1.0e9f));
    }
    return v;
}

struct Result {
    long long pairs = 0, diff = 0;
    long long cases[4] = {0, 0, 0, 0};  // centre cross, vertical arm, horizontal arm, general
};

void worker(int tid, int nthreads, int lanes, const std::vector<Dir>* dirs, Result* out) {
    Result r;
    const float rw = (float)lanes * LANE_W, rwm = rw - 1.5f, ccen = rw + CR, sqm = ccen - 1.55f;
    const std::vector<float> ax = axis_coords(rwm, sqm);
    const int n = (int)ax.size();
    int reports = 0;
    for (int i = tid; i < n * n; i += nthreads) {
        const float fx = ax[i % n], fy = ax[i / n];
        const bool xin = mev::fabs_f(fx - 375.0f) < rwm, yin = mev::fabs_f(fy - 375.0f) < rwm;
        ++r.cases[xin && yin ? 0 : (xin ? 1 : (yin ? 2 : 3))];
        for (const Dir& d : *dirs) {
            // (idx, idy are unused by both; the reciprocals' magnitudes as the callers pass them)
            const float want = mev::road_entry_safe(fx, fy, d.dx, d.dy, 0.0f, 0.0f, d.iadx, d.iady, rwm, ccen, CR);
            const float got = mev::road_entry_safe_uniform(fx, fy, d.dx, d.dy, 0.0f, 0.0f, d.iadx, d.iady, rwm, ccen, CR);
            ++r.pairs;
            if (bits(want) != bits(got)) {
                ++r.diff;
                if (reports++ < 5)
                    printf("DIFF lanes %d p (%.9g, %.9g) d (%.9g, %.9g): uniform %.9g (%08x), general %.9g (%08x)\n", lanes,
                           fx, fy, d.dx, d.dy, got, bits(got), want, bits(want));
            }
        }
    }
    *out = r;
}

}  // namespace

int main() {
    std::vector<Dir> dirs;
    auto add = [&](float dx, float dy) {
        dirs.push_back({dx, dy, mev::fabs_f(1.0f / dx), mev::fabs_f(1.0f / dy)});
    };
    for (int k = 0; k < NANG; ++k) {
        float sn, cs;
        mev::sincosf((float)(-M_PI + (double)k * (2.0 * M_PI / NANG)), &sn, &cs);
        add(cs, -sn);
    }
    const float axd[8][2] = {{1.0f, 0.0f}, {1.0f, -0.0f}, {-1.0f, 0.0f}, {-1.0f, -0.0f},
                             {0.0f, 1.0f}, {-0.0f, 1.0f}, {0.0f, -1.0f}, {-0.0f, -1.0f}};
    for (auto& a : axd) add(a[0], a[1]);

    bool ok = true;
    const int nthreads = 4;
    for (int lanes = 2; lanes <= 4; ++lanes) {
        std::vector<Result> parts(nthreads);
        std::vector<std::thread> th;
        for (int t = 0; t < nthreads; ++t) th.emplace_back(worker, t, nthreads, lanes, &dirs, &parts[t]);
        for (auto& t : th) t.join();
        Result r;
        for (auto& p : parts) {
            r.pairs += p.pairs;
            r.diff += p.diff;
            for (int c = 0; c < 4; ++c) r.cases[c] += p.cases[c];
        }
        printf("lanes %d: %lld origin-direction pairs, %lld differ; origins: cross %lld, vertical arm %lld, "
               "horizontal arm %lld, general %lld\n", lanes, r.pairs, r.diff, r.cases[0], r.cases[1], r.cases[2],
               r.cases[3]);
        if (r.diff != 0) ok = false;
        for (int c = 0; c < 4; ++c)
            if (r.cases[c] == 0) ok = false;
    }
    printf(ok ? "REGIONS OK\n" : "REGIONS FAILED\n");
    return ok ? 0 : 1;
}
