// mev_roadbound.h — the LiDAR road march's safe-distance bounds, usable on the
// gfx950 device and on the host (tests/native/roadbound_check.cpp runs exactly
// this code against the reference's road predicate).
//
// A bound is a distance along a beam from a real point over which every march
// probe is provably on screen and on the road, so the march may skip those
// probes without testing them (mev_kernels.hip, "LiDAR").  A bound may be too
// short (the march then only takes more iterations), never too long.  The
// point's own truncated pixel must be on screen (the car centre the march
// starts from is tested, and so is every probe it jumps from); it may be off
// the road, where every bound is 0.
//
// Host and device differ in the last place of the reciprocals the caller passes
// (1/x against the rcp builtin) and of the square root (sqrtf against the sqrt
// builtin): that moves a bound by < 1e-3 px, which the 0.01 - 2 px margins
// below cover; the device's bits are checked by the GPU parity tests
// (tests/test_road_bound_gpu.py, tests/test_lidar_stress_gpu.py).
#pragma once

#include "mev_math.h"

namespace mev {

// Straight-line LiDAR arithmetic: the value is computed on every lane (an empty
// volatile asm statement the compiler cannot sink into a branch), so a select
// replaces the divergent branch -- exec-mask bookkeeping and a pipeline break --
// the compiler would otherwise wrap around a short computation.  No instruction
// is emitted for it.  (Host: the identity.)
template <class T>
MEV_HD T lidar_keep(T v) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    return v;
}
MEV_HD float rb_sqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(x);
#else
    return __builtin_sqrtf(x);
#endif
}
// a condition every lane of the wave shares, as a scalar branch (host: itself)
MEV_HD bool rb_uniform(bool c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane((int)c) != 0;
#else
    return c;
#endif
}
MEV_HD float rb_min(float a, float b) { return __builtin_fminf(a, b); }
MEV_HD float rb_max(float a, float b) { return __builtin_fmaxf(a, b); }

// Distance along a beam from its real point (fx, fy) over which every probe is
// provably on screen and on the road (the truncated pixel is within 1 px per
// axis, < 1.42 px, of the real point).  Each bound below alone guarantees its
// stretch, so the road bound is their maximum; all are directional:
//  - strips: distance to the strip edge (|x - 375| = rw - 1.5) the ray heads for;
//  - centre square: inside the square shrunk by 1.55 px, within the current
//    quadrant (only its own grass disc can be met there), outside that disc
//    grown by 2 px (extra margin for the tangent-case rounding of the root):
//    distance to the first of the grown disc, the shrunk square's edge and the
//    quadrant's edge;
//  - screen: distance to the half-pixel-inset screen edge.
MEV_HD float road_safe(float fx, float fy, float dx, float dy, float idx, float idy, float iadx, float iady, float rwm,
                       float ccen, float crf) {
    const float big = 1.0e6f;
    const float rx = fx - 375.0f, ry = fy - 375.0f;
    const float ax = fabs_f(rx), ay = fabs_f(ry);
    const float sx = ax < rwm ? rwm * iadx - rx * idx : 0.0f;
    const float sy = ay < rwm ? rwm * iady - ry * idy : 0.0f;
    const float sqm = ccen - 1.55f, rg = crf + 2.0f;
    // the quadrant the ray is in, or heads into from an axis (rx == 0: the sign of dx)
    const float qx = rx != 0.0f ? rx : dx, qy = ry != 0.0f ? ry : dy;
    const float ocx = rx - (qx >= 0.0f ? ccen : -ccen), ocy = ry - (qy >= 0.0f ? ccen : -ccen);
    const float bq = ocx * dx + ocy * dy;
    const float cq = ocx * ocx + ocy * ocy - rg * rg;
    const float disc = bq * bq - cq;
    const float troot = lidar_keep(-bq - rb_sqrt(disc));
    const float tdisc = cq <= 0.0f ? 0.0f : ((disc < 0.0f || bq >= 0.0f) ? big : troot);
    const float tsq = rb_min(sqm * iadx - rx * idx, sqm * iady - ry * idy);
    const float tq = rb_min(rx * dx < 0.0f ? -rx * idx : big, ry * dy < 0.0f ? -ry * idy : big);
    const float sc = rb_max(ax, ay) < sqm ? rb_min(tdisc, rb_min(tsq, tq)) : 0.0f;
    const float road = rb_max(rb_max(sx, sy), sc);
    const float tx = (dx > 0.0f ? 748.5f - fx : fx - 0.5f) * iadx;
    const float ty = (dy > 0.0f ? 748.5f - fy : fy - 0.5f) * iady;
    return rb_min(road, rb_min(tx, ty));
}

// road_safe from a point every lane of the wave shares (phase 1: the car centre
// of the pass's agent): the strip and centre-square terms are wave-uniform
// branches, so a car outside the centre square does not evaluate the disc root.
MEV_HD float road_safe_uniform(float fx, float fy, float dx, float dy, float idx, float idy, float iadx, float iady,
                               float rwm, float ccen, float crf) {
    const float big = 1.0e6f;
    const float rx = fx - 375.0f, ry = fy - 375.0f;
    const float ax = fabs_f(rx), ay = fabs_f(ry);
    const float sqm = ccen - 1.55f, rg = crf + 2.0f;
    float road = 0.0f;
    if (rb_uniform(ax < rwm)) road = rb_max(road, rwm * iadx - rx * idx);
    if (rb_uniform(ay < rwm)) road = rb_max(road, rwm * iady - ry * idy);
    if (rb_uniform(rb_max(ax, ay) < sqm)) {
        const float qx = rx != 0.0f ? rx : dx, qy = ry != 0.0f ? ry : dy;
        const float ocx = rx - (qx >= 0.0f ? ccen : -ccen), ocy = ry - (qy >= 0.0f ? ccen : -ccen);
        const float bq = ocx * dx + ocy * dy;
        const float cq = ocx * ocx + ocy * ocy - rg * rg;
        const float disc = bq * bq - cq;
        const float troot = lidar_keep(-bq - rb_sqrt(disc));
        const float tdisc = cq <= 0.0f ? 0.0f : ((disc < 0.0f || bq >= 0.0f) ? big : troot);
        const float tsq = rb_min(sqm * iadx - rx * idx, sqm * iady - ry * idy);
        const float tq = rb_min(rx * dx < 0.0f ? -rx * idx : big, ry * dy < 0.0f ? -ry * idy : big);
        road = rb_max(road, rb_min(tdisc, rb_min(tsq, tq)));
    }
    const float tx = (dx > 0.0f ? 748.5f - fx : fx - 0.5f) * iadx;
    const float ty = (dy > 0.0f ? 748.5f - fy : fy - 0.5f) * iady;
    return rb_min(road, rb_min(tx, ty));
}

// The same guarantee from a global view of the road: the distance to the ray's
// first entry into the off-road set, whatever strips and squares it crosses on
// the way.  road_safe's terms each end at the border of the region the point is
// in, so a beam from a strip through the centre into the opposite strip needs a
// bound and probes per region; this one needs them once.
//
// With r = (fx, fy) - 375, the off-road pixels lie in four grass quadrants, one
// per sign pair (sx, sy): u = sx*rx >= rw and v = sy*ry >= rw, minus the corner
// square (u, v <= rw + cr) outside the grass disc of radius cr about (rw + cr,
// rw + cr).  Each is grown to a set of REAL points that holds every real point
// whose truncated pixel (within 1 px per axis, < 1.42 px, of it) is off the
// road, with road_safe's margins:
//   Q        = {u > rwm and v > rwm},  rwm = rw - 1.5: a pixel with |p - 375| >=
//              rw (the discs' tangent pixels sit at rw) has |r| > rw - 1;
//   straight = Q and max(u, v) >= sqm,  sqm = ccen - 1.55: a pixel past the
//              corner square, max|p - 375| > ccen, has max(u, v) > ccen - 1;
//   disc     = Q and |(u, v) - (ccen, ccen)| <= rg,  rg = cr + 2: a pixel in the
//              grass disc (d^2 < cr^2 + 1) is within cr + 1.42 of the centre;
//              the rest of the 2 px absorbs the rounding of the root, largest
//              for a tangent ray (an error s along the ray there moves the
//              point only s^2 / (2 rg) into the disc).
// The 0.05 - 0.58 px of slack in each also covers the float rounding of the
// entry times (< 1e-3 px anywhere on or near the screen).
//
// Q is convex, so the ray is inside it over one interval [t_in, t_out), from the
// per-axis times at which u and v cross rwm; the quadrants are disjoint, so
// their intervals are too.  The grass is symmetric about both axes, so the ray is
// first reflected to head towards +x, +y (x = rx * sign(dx), a = |dx|; y, b
// likewise).  Then it can only meet the quadrants in the order (-,-) [only if it
// starts there], then (-,+) or (+,-) [only if it starts on their negative side;
// never both: it would have to reach x > rwm before y > -rwm and y > rwm before
// x > -rwm, and each axis reaches -rwm before +rwm], then (+,+), which it never
// leaves.  For the quadrant entered first the bound is exact: t_in if the entry
// point lies on the straight part, else the first of the disc's entry
// (road_safe's root, taken from the entry point) and of a growing coordinate
// reaching sqm -- if that comes before t_out; otherwise the ray crosses that
// corner square on the road and the quadrant yields nothing.  Every later
// quadrant contributes its t_in (its own first entry is no earlier).  The road
// bound is the minimum; in the rare beam that crosses one corner square and
// later enters another quadrant the march re-evaluates at that quadrant's
// border.  The result is min(road bound, road_safe's screen terms).
//
// Infinite or NaN times (a direction component of 0 or -0, whose reciprocal is
// infinite) only arise where "never" is meant or on the short side: a NaN needs
// a coordinate exactly on a line (0 * inf), min/max drop it, and a comparison
// with it is false, which keeps a quadrant the ray only touches.
// REG: what the caller knows about the point, as a mask.  Bit 0 (kRegX): |rx| < rwm; bit 1 (kRegY):
// |ry| < rwm.  3 is the centre cross, 1 a vertical arm, 2 a horizontal arm, 0 nothing: the general form.
// With |rx| < rwm the reflected x = +-rx is never below -rwm, whatever the sign of dx: xn is false, so
// (-,-) and (-,+) cannot be met (v4 = v2 = false, xg = true), txm is not needed, and rwm - x > 0 makes
// txp positive (or +inf), so inx = txp without the max.  |ry| < rwm likewise; with both only (+,+) is
// left: m1 = t1, o1 = m2 = never.  Every other operation is the general form's own, in its order and
// with its comparison forms, so every mask's result has the general form's bits.
//
// The products that feed a sum (ue, ve, bq, cq, disc) are fused: the bound only has to be safe, not to
// round like anything in the reference (the build's -ffp-contract=off is for the reference's
// arithmetic), and a fused operation rounds once where the unfused pair rounds twice, so its error is
// no larger and the margins above hold as argued.  cq is also reassociated, ocx^2 + (ocy^2 - rg^2) in
// two fused steps where it was (ocx^2 + ocy^2) - rg^2: each step's rounding is at most half an ulp of a
// value below 2^18 px^2 (< 0.01 px^2: a change of the disc's radius below 1e-4 px at rg = 86 px), far
// inside the same margins; tests/native/roadbound_check.cpp checks the safety of exactly this code.  Not symmetric in x and y any more (ocx * a is the
// fused product of bq, ocy * b the rounded one), which is why the arms are two cases of one body and
// not one case called with swapped axes.
constexpr int kRegX = 1, kRegY = 2;
template <int REG>
MEV_HD float road_entry_region(float fx, float fy, float dx, float dy, float iadx, float iady, float rwm, float ccen,
                               float crf) {
    constexpr bool xin = (REG & kRegX) != 0, yin = (REG & kRegY) != 0;
    const float never = 1.0e6f;
    const float rx = fx - 375.0f, ry = fy - 375.0f;
    const float sqm = ccen - 1.55f, rg = crf + 2.0f;
    const float x = dx < 0.0f ? -rx : rx, y = dy < 0.0f ? -ry : ry;
    const float a = fabs_f(dx), b = fabs_f(dy);
    // the times at which x and y reach +rwm, -rwm and sqm
    const float txp = (rwm - x) * iadx, txm = (-rwm - x) * iadx, txs = (sqm - x) * iadx;
    const float typ = (rwm - y) * iady, tym = (-rwm - y) * iady, tys = (sqm - y) * iady;
    const float inx = xin ? txp : rb_max(txp, 0.0f), iny = yin ? typ : rb_max(typ, 0.0f);  // x > rwm, y > rwm from then on
    const float t1 = rb_max(inx, iny);                             // (+,+): entered at t1, never left
    const bool xn = !xin && x < -rwm, yn = !yin && y < -rwm;
    const bool v4 = xn && yn;        // (-,-): from 0 until x or y reaches -rwm
    const bool v2 = xn && iny < txm;  // (-,+): from iny until x reaches -rwm
    const bool v3 = yn && inx < tym;  // (+,-): from inx until y reaches -rwm
    // the first quadrant entered (at m1, left at o1; xg / yg: its x / y coordinate grows) and the next one's entry (m2)
    const float mA = v2 ? iny : (v3 ? inx : t1);
    const float oA = v2 ? txm : (v3 ? tym : never);
    const float mB = (v2 || v3) ? t1 : never;
    const float m1 = v4 ? 0.0f : mA, o1 = v4 ? rb_min(txm, tym) : oA, m2 = v4 ? mA : mB;
    const bool xg = !(v4 || v2), yg = !(v4 || v3);
    // from its entry point e: u = |ex|, v = |ey| there
    const float ue = fabs_f(__builtin_fmaf(a, m1, x)), ve = fabs_f(__builtin_fmaf(b, m1, y));
    const float ocx = ue - ccen, ocy = ve - ccen;
    const float bq = __builtin_fmaf(ocx, xg ? a : -a, ocy * (yg ? b : -b));
    const float cq = __builtin_fmaf(ocx, ocx, __builtin_fmaf(ocy, ocy, -(rg * rg)));
    const float disc = __builtin_fmaf(bq, bq, -cq);
    const float troot = lidar_keep(-bq - rb_sqrt(disc));
    const float tdisc = cq <= 0.0f ? 0.0f : ((disc < 0.0f || bq >= 0.0f) ? never : troot);
    const float tcorner = rb_min(m1 + tdisc, rb_min(xg ? txs : never, yg ? tys : never));
    const float tq = rb_max(ue, ve) >= sqm ? m1 : (tcorner < o1 ? tcorner : never);
    const float road = rb_min(tq, m2);
    const float tx = ((dx > 0.0f ? 373.5f : 374.5f) - x) * iadx;  // 748.5 - fx or fx - 0.5
    const float ty = ((dy > 0.0f ? 373.5f : 374.5f) - y) * iady;
    return rb_min(road, rb_min(tx, ty));
}

MEV_HD float road_entry_safe(float fx, float fy, float dx, float dy, float idx, float idy, float iadx, float iady,
                             float rwm, float ccen, float crf) {
    (void)idx;
    (void)idy;
    return road_entry_region<0>(fx, fy, dx, dy, iadx, iady, rwm, ccen, crf);
}

// road_entry_safe from a point every lane of the wave shares (phase 1: the car centre of the pass's
// agent; road_safe_uniform's contract): which grass quadrants a ray can start in depends on the point
// alone.  A car on the road is in the centre cross or in an arm unless it sits on a corner fillet;
// anything else takes the general form.  The same bits as road_entry_safe.
//
// The region of the point, the very comparisons the general form makes (a NaN coordinate fails both and
// takes the general form):
MEV_HD bool road_region_xin(float fx, float rwm) { return fabs_f(fx - 375.0f) < rwm; }
MEV_HD bool road_region_yin(float fy, float rwm) { return fabs_f(fy - 375.0f) < rwm; }
// ... and whether the point's truncated pixel is on the 750 px screen (phase 1 skips the safe stretch from
// the car centre only then): both coordinates in [0, 750) in one unsigned comparison.
MEV_HD bool road_point_on_screen(float fx, float fy) {
    const int px = (int)fx, py = (int)fy;
    const unsigned pmax = (unsigned)px > (unsigned)py ? (unsigned)px : (unsigned)py;
    return pmax < 750u;
}
// xin, yin: road_region_xin(fx, rwm) and road_region_yin(fy, rwm), from the caller and wave-uniform (phase
// 1's agent pre-pass evaluates them once per agent, one agent per lane, and hands each pass its agent's two
// bits as scalars, so the beam passes no longer redo them in every lane).
MEV_HD float road_entry_safe_uniform(float fx, float fy, float dx, float dy, float iadx, float iady, float rwm,
                                     float ccen, float crf, bool xin, bool yin) {
    if (xin && yin) return road_entry_region<kRegX | kRegY>(fx, fy, dx, dy, iadx, iady, rwm, ccen, crf);
    if (xin) return road_entry_region<kRegX>(fx, fy, dx, dy, iadx, iady, rwm, ccen, crf);
    if (yin) return road_entry_region<kRegY>(fx, fy, dx, dy, iadx, iady, rwm, ccen, crf);
    return road_entry_region<0>(fx, fy, dx, dy, iadx, iady, rwm, ccen, crf);
}
// ... and for a caller that has not: the bits derived here, in every lane.  No kernel calls this form any
// more -- phase 1's pair loop supplies the bits, every other caller of the entry bound takes road_entry_safe;
// it is kept for the host check tests/native/roadbound_regions_check.cpp, which pins it to the general form.
MEV_HD float road_entry_safe_uniform(float fx, float fy, float dx, float dy, float idx, float idy, float iadx,
                                     float iady, float rwm, float ccen, float crf) {
    (void)idx;
    (void)idy;
    return road_entry_safe_uniform(fx, fy, dx, dy, iadx, iady, rwm, ccen, crf, rb_uniform(road_region_xin(fx, rwm)),
                                   rb_uniform(road_region_yin(fy, rwm)));
}

}  // namespace mev
