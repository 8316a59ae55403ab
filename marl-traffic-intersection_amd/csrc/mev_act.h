// mev_act.h — the activations of the rollout policies (include/marlenv.h, "THE ARITHMETIC IS PART OF THE
// CONTRACT"), usable on the gfx950 device and on the host.
//
// tanh_c is a tanh DEFINED AS ARITHMETIC: a fixed sequence of f32 operations -- add, subtract, multiply, the
// IEEE divide, fmaf, rintf, comparisons, selects and bit operations -- with no libm or device transcendental, no
// approximate reciprocal and nothing in double.  Built with -ffp-contract=off the same source gives the same bits
// under g++ on x86-64 and on gfx950 (mev_tanh, the host export, runs this very function).  It is written as
// selects, not branches: a lane of the policy kernels holds 8 agents' values, and a divergent branch would run
// both ways there.
//
// THE SEQUENCE, for an input y (every operation f32, one rounding each):
//
//   a  = |y|                                   (the sign bit cleared)
//   ac = a < 10.0f ? a : 10.0f                 (NaN gives 10: every later operand is finite)
//   -- the polynomial form, used for a < 0.5625:
//   s  = ac * ac
//   q  = fmaf(s, fmaf(s, fmaf(s, fmaf(s, Q4, Q3), Q2), Q1), Q0)
//   p  = fmaf(ac * s, q, ac)
//   -- the exponential form, used for a >= 0.5625:
//   x  = ac + ac
//   n  = rintf(x * LOG2E)                      (round to nearest even; 2 <= n <= 29 where the form is used)
//   r  = fmaf(-n, LN2_LO, fmaf(-n, LN2_HI, x)) (Cody-Waite; the inner fmaf is exact)
//   g  = fmaf(r, fmaf(r, fmaf(r, fmaf(r, G4, G3), G2), G1), G0)
//   E  = fmaf(r, fmaf(r, g, 1.0f), 1.0f) * 2^n (2^n built from its bits, (n + 127) << 23: an exact scaling)
//   t  = 1.0f - 2.0f / (E + 1.0f)              (the correctly rounded divide)
//   -- the choice:
//   m  = a < 0x1p-12f ? a : a < 0.5625f ? p : t
//   tanh_c(y) = y != y ? +0.0f : copysign(m, y)
//
// So: below 2^-12 the input itself (the correctly rounded value there; +-0 and subnormals exact); an odd polynomial
// y + y s Q(s) below 0.5625 (tanh(0.5625) > 0.5, so the exponential form's subtraction never loses a bit to
// cancellation where it is used); 1 - 2 / (exp(2a) + 1) above; and from a = 10 on every input is computed as 10,
// where the form gives exactly 1.0f (it does from 9.02 on: 2 / (E + 1) is below 2^-25).  NaN gives +0.0f, as
// the ReLU does: a NaN never leaves a hidden layer.  tanh_c(-y) has the bits of -tanh_c(y), |tanh_c| <= 1, and
// tanh_c is non-decreasing across every pair of adjacent finite floats (tests/native/tanh_check.cpp, whose
// `exhaustive` mode visits every float).
//
// The constants (least-squares fits on Chebyshev nodes, rounded to f32):
//   Q(s) ~ (tanh(y) / y - 1) / s on s in [0, 0.5625^2]; G(r) ~ (exp(r) - 1 - r) / r^2 on |r| <= ln(2) / 2.
//
// MEASURED against tanh in double over every finite float (tanh_check exhaustive), the maximum error in ulp of
// the result: 0.333 where y itself is returned (at 0x1.fffffep-13), 0.814 in the polynomial region (at
// 0x1.14e8bp-1), 1.537 in the exponential region below 8 (at 0x1.211b7ap-1, just above the threshold, where
// the result's ulp is smallest against the quotient's), 0.500 from 8 on.  No region exceeds 2 ulp, and no pair
// of adjacent floats decreases.  The strided test asserts these rounded up to whole ulps: 1, 1, 2, 1.
#pragma once

#include "mev_math.h"

namespace mev {

constexpr float kTanhTiny = 0x1p-12f;    // below: y itself
constexpr float kTanhSmall = 0.5625f;    // below: the polynomial form
constexpr float kTanhSat = 10.0f;        // from here on: computed as 10, exactly 1
constexpr float kTanhQ0 = -0x1.555554p-2f, kTanhQ1 = 0x1.110fbap-3f, kTanhQ2 = -0x1.b9915ep-5f,
                kTanhQ3 = 0x1.5c6c6p-6f, kTanhQ4 = -0x1.abecbp-8f;
constexpr float kTanhLog2e = 0x1.715476p+0f, kTanhLn2Hi = 0x1.62e4p-1f, kTanhLn2Lo = 0x1.7f7d1cp-20f;
constexpr float kTanhG0 = 0x1p-1f, kTanhG1 = 0x1.5554dcp-3f, kTanhG2 = 0x1.5554e8p-5f, kTanhG3 = 0x1.120c74p-7f,
                kTanhG4 = 0x1.6d445ep-10f;

MEV_HD float tanh_c(float y) {
    const float a = fabs_f(y);
    const float ac = a < kTanhSat ? a : kTanhSat;
    const float s = ac * ac;
    const float q = __builtin_fmaf(
        s, __builtin_fmaf(s, __builtin_fmaf(s, __builtin_fmaf(s, kTanhQ4, kTanhQ3), kTanhQ2), kTanhQ1), kTanhQ0);
    const float p = __builtin_fmaf(ac * s, q, ac);
    const float x = ac + ac;
    const float n = __builtin_rintf(x * kTanhLog2e);
    const float r = __builtin_fmaf(-n, kTanhLn2Lo, __builtin_fmaf(-n, kTanhLn2Hi, x));
    const float g = __builtin_fmaf(
        r, __builtin_fmaf(r, __builtin_fmaf(r, __builtin_fmaf(r, kTanhG4, kTanhG3), kTanhG2), kTanhG1), kTanhG0);
    const float scale = u2f((uint32_t)((int32_t)n + 127) << 23);
    const float E = __builtin_fmaf(r, __builtin_fmaf(r, g, 1.0f), 1.0f) * scale;
    const float t = 1.0f - 2.0f / (E + 1.0f);
    const float m = a < kTanhTiny ? a : a < kTanhSmall ? p : t;
    return y != y ? 0.0f : u2f(f2u(m) | (f2u(y) & 0x80000000u));
}

}  // namespace mev
