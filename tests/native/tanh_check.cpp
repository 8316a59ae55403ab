// tanh_c (csrc/mev_act.h) against its stated properties and against tanh in double.
//
//   tanh_check             strided: every binade of finite f32 at a stride, and exhaustively the 2^16 floats on
//                          either side of every value the sequence branches on (its three thresholds, where the
//                          form first gives 1, and every boundary of the range reduction's n)
//   tanh_check exhaustive  every finite float, monotonicity across every adjacent pair
//
// Checked for every visited y >= 0: tanh_c(-y) has the bits of -tanh_c(y); 0 <= tanh_c(y) <= 1; across adjacent
// floats (stride 1) tanh_c does not decrease; the error against tanh in double, in ulp of the result, stays within
// the recorded bound of its region.  The bounds are the exhaustive run's maxima rounded up to the next whole ulp.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "mev_act.h"

static uint32_t f2u_(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float u2f_(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// the regions the error is reported for
enum { R_TINY, R_POLY, R_EXP, R_SAT, R_COUNT };
static const char* kRegion[R_COUNT] = {"identity  a < 2^-12", "polynomial  2^-12 <= a < 0.5625", "exponential  0.5625 <= a < 8",
                                       "saturation  a >= 8"};
// the exhaustive run's maxima (0.333, 0.814, 1.537 and 0.500 ulp; no decreasing pair among all 2139095040 finite
// floats), rounded up to the next whole ulp
static const double kBound[R_COUNT] = {1.0, 1.0, 2.0, 1.0};
static int region(float a) { return a < mev::kTanhTiny ? R_TINY : a < mev::kTanhSmall ? R_POLY : a < 8.0f ? R_EXP : R_SAT; }

struct Stats {
    double err[R_COUNT] = {0, 0, 0, 0};
    float at[R_COUNT] = {0, 0, 0, 0};
    uint64_t odd = 0, bound = 0, mono = 0, n = 0;
    void merge(const Stats& o) {
        for (int r = 0; r < R_COUNT; ++r)
            if (o.err[r] > err[r]) { err[r] = o.err[r]; at[r] = o.at[r]; }
        odd += o.odd; bound += o.bound; mono += o.mono; n += o.n;
    }
};

static double ulp_err(float got, double want) {
    const float w = (float)want;  // the ulp of the result: the spacing of f32 at the rounded true value
    int e;
    std::frexp(w, &e);
    const double ulp = std::ldexp(1.0, std::max(e - 24, -149));
    return std::fabs((double)got - want) / ulp;
}

// bit patterns lo .. hi (positive floats), every step-th; step == 1 also checks adjacent pairs, from lo - 1 on
static Stats sweep(uint32_t lo, uint32_t hi, uint32_t step) {
    Stats s;
    float prev = lo > 0 && step == 1 ? mev::tanh_c(u2f_(lo - 1)) : 0.0f;
    for (uint64_t u = lo; u <= hi; u += step) {
        const float y = u2f_((uint32_t)u), v = mev::tanh_c(y);
        ++s.n;
        if (f2u_(mev::tanh_c(-y)) != (f2u_(v) ^ 0x80000000u)) ++s.odd;
        if (!(v >= 0.0f && v <= 1.0f)) ++s.bound;
        if (step == 1) {
            if (!(v >= prev)) {
                if (s.mono < 4) std::printf("  tanh_c decreases at %a: %a after %a\n", y, v, prev);
                ++s.mono;
            }
            prev = v;
        }
        const int r = region(y);
        const double e = ulp_err(v, std::tanh((double)y));
        if (e > s.err[r]) { s.err[r] = e; s.at[r] = y; }
    }
    return s;
}

static Stats around(float c) {
    const uint32_t u = f2u_(c);
    return sweep(u > 65536u ? u - 65536u : 0u, u + 65536u, 1);
}

int main(int argc, char** argv) {
    const bool exhaustive = argc > 1 && std::strcmp(argv[1], "exhaustive") == 0;
    const uint32_t kMaxFinite = 0x7f7fffffu;
    int rc = 0;
    Stats all;
    if (exhaustive) {
        const unsigned T = std::max(1u, std::thread::hardware_concurrency());
        std::vector<Stats> part(T);
        std::vector<std::thread> th;
        const uint64_t total = (uint64_t)kMaxFinite + 1, chunk = (total + T - 1) / T;
        for (unsigned t = 0; t < T; ++t)
            th.emplace_back([&, t] {
                const uint64_t lo = t * chunk, hi = std::min(total, lo + chunk) - 1;
                if (lo <= hi) part[t] = sweep((uint32_t)lo, (uint32_t)hi, 1);
            });
        for (auto& x : th) x.join();
        for (auto& p : part) all.merge(p);
    } else {
        all.merge(sweep(0, kMaxFinite, 1021));  // (every binade: 2^23 patterns each, 8216 of them visited)
        all.merge(sweep(0, 65536, 1));          // the subnormals next to zero
        all.merge(sweep(kMaxFinite - 65536, kMaxFinite, 1));
        all.merge(around(mev::kTanhTiny));
        all.merge(around(mev::kTanhSmall));
        all.merge(around(mev::kTanhSat));
        all.merge(around(9.0109f));  // where 2 / (E + 1) falls below 2^-25: the form's first exact 1
        for (int n = 1; n <= 29; ++n)  // the range reduction's boundaries: 2 a log2(e) = n + 1/2
            all.merge(around((float)((n + 0.5) * 0.5 * 0.6931471805599453)));
    }
    std::printf("%llu values\n", (unsigned long long)all.n);
    for (int r = 0; r < R_COUNT; ++r) {
        std::printf("max error, %s: %.3f ulp at %a (bound %.0f)\n", kRegion[r], all.err[r], all.at[r], kBound[r]);
        if (all.err[r] > kBound[r]) rc = 1;
    }
    std::printf("oddness failures %llu, bound failures %llu, decreasing pairs %llu\n", (unsigned long long)all.odd,
                (unsigned long long)all.bound, (unsigned long long)all.mono);
    if (all.odd || all.bound || all.mono) rc = 1;

    // the special values
    uint64_t bad = 0;
    auto want = [&](float y, uint32_t bits, const char* what) {
        if (f2u_(mev::tanh_c(y)) != bits) {
            std::printf("  tanh_c(%s) = %a (0x%08x), expected 0x%08x\n", what, mev::tanh_c(y), f2u_(mev::tanh_c(y)), bits);
            ++bad;
        }
    };
    want(0.0f, 0x00000000u, "+0");
    want(-0.0f, 0x80000000u, "-0");
    want(NAN, 0x00000000u, "NaN");
    want(-NAN, 0x00000000u, "-NaN");
    want(u2f_(0x7f800001u), 0x00000000u, "sNaN");
    want(u2f_(0xffc12345u), 0x00000000u, "-NaN with payload");
    want(INFINITY, 0x3f800000u, "+inf");
    want(-INFINITY, 0xbf800000u, "-inf");
    want(3e38f, 0x3f800000u, "3e38");
    want(-3e38f, 0xbf800000u, "-3e38");
    want(10.0f, 0x3f800000u, "10");
    want(u2f_(1u), 1u, "the smallest subnormal");
    want(u2f_(0x807fffffu), 0x807fffffu, "the largest negative subnormal");
    want(u2f_(0x00800000u), 0x00800000u, "the smallest normal");
    std::printf("special values: %llu wrong\n", (unsigned long long)bad);
    if (bad) rc = 1;
    std::printf(rc ? "TANH MISMATCH\n" : "TANH OK\n");
    return rc;
}
