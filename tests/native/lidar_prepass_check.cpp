// Host check of what LiDAR phase 1's agent pre-pass and the per-handle beam model hoist out of the beam
// passes (csrc/mev_roadbound.h, csrc/mev_beams.h; lidar_body in csrc/mev_kernels.hip).
//
// 1. The pre-pass's bits -- road_region_xin, road_region_yin, road_point_on_screen, evaluated once per
//    agent -- equal the comparisons the beam passes made in every lane: |p - 375| < rwm per axis, and
//    max((unsigned)(int)x, (unsigned)(int)y) < 750.  Coordinates: the lattice of
//    roadbound_regions_check.cpp, one ulp either side of |r| = rwm on each axis and both signs, of 0 and
//    of 750, negative, NaN and infinite ones.  (The conversion of a NaN or an infinity to int is the
//    platform's; both sides convert alike, which is all the kernel needs: it evaluates one expression.)
// 2. road_entry_safe_uniform with the bits supplied returns the bits of road_entry_safe, over the origin x
//    direction grid of roadbound_regions_check.cpp (2, 3 and 4 lanes; 4096 angles and the eight axis
//    directions) plus the extra coordinates of 1.  Every region must occur.
// 3. beam_model's rel0, dphi, idphi, period and inv_r have the bits of the expressions phase 3 evaluated
//    on the device every step, for the beam lists mev_create makes (64, 96 and 128 beams, fov 360 and
//    120), a reversed list and a single beam.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <thread>
#include <vector>

#include "mev_beams.h"
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

void around(std::vector<float>& v, float m) {
    v.push_back(nextafterf(m, -1.0e9f));
    v.push_back(m);
    v.push_back(nextafterf(m, 1.0e9f));
}

std::vector<float> axis_coords(float rwm, float sqm) {
    std::vector<float> v;
    for (int i = 0; i <= 60; ++i) v.push_back(12.5f * (float)i);
    const float marks[7] = {0.0f, 375.0f - sqm, 375.0f - rwm, 375.0f, 375.0f + rwm, 375.0f + sqm, 750.0f};
    for (float m : marks) around(v, m);
    around(v, 1.0f);  // (int) truncates towards zero: (-1, 1) is pixel 0
    around(v, -1.0f);
    const float inf = std::numeric_limits<float>::infinity();
    const float extra[8] = {-0.0f, -0.5f, -37.5f, -1.0e9f, 1.0e9f, inf, -inf, std::numeric_limits<float>::quiet_NaN()};
    for (float e : extra) v.push_back(e);
    return v;
}

struct Result {
    long long pairs = 0, diff = 0, bitdiff = 0;
    long long cases[4] = {0, 0, 0, 0};  // centre cross, vertical arm, horizontal arm, general
    long long onscr[2] = {0, 0};
};

void worker(int tid, int nthreads, int lanes, const std::vector<Dir>* dirs, Result* out) {
    Result r;
    const float rw = (float)lanes * LANE_W, rwm = rw - 1.5f, ccen = rw + CR, sqm = ccen - 1.55f;
    const std::vector<float> ax = axis_coords(rwm, sqm);
    const int n = (int)ax.size();
    int reports = 0;
    for (int i = tid; i < n * n; i += nthreads) {
        const float fx = ax[i % n], fy = ax[i / n];
        // 1: the pre-pass against the per-lane comparisons
        const bool xin = mev::road_region_xin(fx, rwm), yin = mev::road_region_yin(fy, rwm);
        const bool on = mev::road_point_on_screen(fx, fy);
        const bool xin_w = mev::fabs_f(fx - 375.0f) < rwm, yin_w = mev::fabs_f(fy - 375.0f) < rwm;
        const int px = (int)fx, py = (int)fy;
        const unsigned pmax = (unsigned)px > (unsigned)py ? (unsigned)px : (unsigned)py;
        const bool on_w = pmax < 750u;
        if (xin != xin_w || yin != yin_w || on != on_w) {
            ++r.bitdiff;
            if (reports++ < 5) printf("BITS lanes %d p (%.9g, %.9g): pre-pass %d%d%d, per lane %d%d%d\n", lanes, fx, fy, xin, yin, on, xin_w, yin_w, on_w);
        }
        if (fx != fx || fy != fy) {  // a NaN coordinate takes the general form
            if (fx != fx && xin) ++r.bitdiff;
            if (fy != fy && yin) ++r.bitdiff;
        }
        ++r.cases[xin && yin ? 0 : (xin ? 1 : (yin ? 2 : 3))];
        ++r.onscr[on ? 1 : 0];
        // 2: the bound with the bits supplied against the general form
        for (const Dir& d : *dirs) {
            const float want = mev::road_entry_safe(fx, fy, d.dx, d.dy, 0.0f, 0.0f, d.iadx, d.iady, rwm, ccen, CR);
            const float got = mev::road_entry_safe_uniform(fx, fy, d.dx, d.dy, d.iadx, d.iady, rwm, ccen, CR, xin, yin);
            ++r.pairs;
            if (bits(want) != bits(got)) {
                ++r.diff;
                if (reports++ < 5)
                    printf("DIFF lanes %d p (%.9g, %.9g) d (%.9g, %.9g): with bits %.9g (%08x), general %.9g (%08x)\n", lanes,
                           fx, fy, d.dx, d.dy, got, bits(got), want, bits(want));
            }
        }
    }
    *out = r;
}

// the beam offsets as mev_create computes them (the reference's Lidar.cpp:4-14)
std::vector<float> beam_list(int rays, float fov_deg) {
    std::vector<float> rel((size_t)rays);
    const float start_angle_deg = -fov_deg * 0.5f;
    const float step_deg = (rays > 1) ? (fov_deg / float(rays - 1)) : 0.0f;
    const float PI_F2 = 3.14159265358979323846f;
    for (int ii = 0; ii < rays; ++ii) {
        const float deg = start_angle_deg + float(ii) * step_deg;
        rel[(size_t)ii] = deg * PI_F2 / 180.0f;
    }
    return rel;
}

// phase 3's own expressions, as the kernel evaluated them at the head of every step
bool beams_ok(const char* name, const std::vector<float>& rel) {
    const int R = (int)rel.size();
    const float* r = rel.data();
    const float rel0 = r[0];
    const float dphi = R > 1 ? (r[R - 1] - rel0) / (float)(R - 1) : 1.0f;
    const float idphi = 1.0f / dphi;
    const float period = 6.28318531f * idphi;
    const float invR = 1.0f / (float)R;
    const mev::BeamModel m = mev::beam_model(r, R);
    const bool ok = bits(m.rel0) == bits(rel0) && bits(m.dphi) == bits(dphi) && bits(m.idphi) == bits(idphi) &&
                    bits(m.period) == bits(period) && bits(m.inv_r) == bits(invR);
    // ... and in double, rounded once: a contracted or reassociated host build would show here
    const double dd = ((double)r[R > 1 ? R - 1 : 0] - (double)r[0]) / (double)(R > 1 ? R - 1 : 1);
    const bool near = R == 1 || fabs((double)m.dphi - dd) <= 1.0e-6 * fabs(dd) + 1.0e-12;
    printf("beams %-14s R %3d rel0 %08x dphi %08x idphi %08x period %08x inv_r %08x %s\n", name, R, bits(m.rel0),
           bits(m.dphi), bits(m.idphi), bits(m.period), bits(m.inv_r), ok && near ? "ok" : "DIFFER");
    return ok && near;
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
            r.bitdiff += p.bitdiff;
            for (int c = 0; c < 4; ++c) r.cases[c] += p.cases[c];
            for (int c = 0; c < 2; ++c) r.onscr[c] += p.onscr[c];
        }
        printf("lanes %d: %lld origin-direction pairs, %lld differ, %lld origins with other bits; origins: cross %lld, "
               "vertical arm %lld, horizontal arm %lld, general %lld; on screen %lld, off %lld\n", lanes, r.pairs, r.diff,
               r.bitdiff, r.cases[0], r.cases[1], r.cases[2], r.cases[3], r.onscr[1], r.onscr[0]);
        if (r.diff != 0 || r.bitdiff != 0) ok = false;
        for (int c = 0; c < 4; ++c)
            if (r.cases[c] == 0) ok = false;
        if (r.onscr[0] == 0 || r.onscr[1] == 0) ok = false;
    }

    int nlists = 0;
    for (int rays : {64, 96, 128})
        for (float fov : {360.0f, 120.0f}) {
            char name[32];
            snprintf(name, sizeof name, "%d/fov%d", rays, (int)fov);
            ok = beams_ok(name, beam_list(rays, fov)) && ok;
            ++nlists;
        }
    std::vector<float> rev = beam_list(64, 360.0f);
    for (size_t i = 0; i < rev.size() / 2; ++i) {
        const float t = rev[i];
        rev[i] = rev[rev.size() - 1 - i];
        rev[rev.size() - 1 - i] = t;
    }
    ok = beams_ok("64/reversed", rev) && ok;
    ok = beams_ok("1/fov360", beam_list(1, 360.0f)) && ok;
    nlists += 2;
    printf("beam lists %d\n", nlists);
    printf(ok ? "PREPASS OK\n" : "PREPASS FAILED\n");
    return ok ? 0 : 1;
}
