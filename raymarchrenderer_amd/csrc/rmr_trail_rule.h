// rmr_trail_rule.h — the acceptance rule of the lane-slot kernels' trailing steps (rmr_trace.h
// RMR_TRAIL_STEPS, trace_main), as arithmetic on plain floats. The kernel and the host program
// csrc/trail_rule_test.cpp compile these statements.
//
// A map-loop iteration evaluates the whole approximate map at the march point p0 = fma(d, t0, o) of
// every marching lane (the anchor). Its fold leaves, in registers, the approximate minimiser w and the
// runner-up s2: the second smallest approximate distance, so a_j >= s2 for every primitive j != w
// (am_take / am_boxes keep that whether or not w is the unique minimiser). A trailing step is a march
// step, after that iteration's own, which evaluates primitive w alone.
//
// Derivation. F_j(x) is the float evaluation of primitive j's distance at x (sd_box / sd_sphere), f_j
// the exact one.
//  (1) |a_j - F_j(p0)| <= err(a_j) = 2^-21 (|a_j| + R) + 2^-40 (rmr_trace.h AMin; R the largest sphere
//      radius), and err is monotonic, so F_j(p0) >= s2 - err(s2) for j != w.
//  (2) |F_j(x) - f_j(x)| <= eps(x) = 2^-17 (|x|_inf + E) (rmr_trace.h npc_eps: 4x slack over the
//      rounding analysis, the rounding of x = fma(d, t, o) itself included).
//  (3) f_j is 1-Lipschitz, and a trailing point p = fma(d, t, o) of the same ray lies within
//      delta = (t - t0)(1 + 2^-21) of p0 (|d| <= 1 + 2^-22 for the kernels' normalised directions; the
//      factor also covers the subtraction's rounding). t >= t0 because a march only advances by
//      distances >= 0.001 times stepMultiply > 0 (the host turns the steps off for other stepMultiply).
// So F_j(p) >= s2 - err(s2) - eps(p0) - delta - eps(p) for every j != w. When that exceeds F_w(p), w is
// the strict minimiser of the float fold at p, and with F_w(p) < maxDist the fold opU((maxDist, -1), ...)
// returns (F_w(p), id_w) whatever the scene order — the value the full map returns there, by its
// direct result or by its exact fallback. am_dmax < maxDist (rmr_api.cpp am_direct_bound) is the
// direct result's own condition and the one tested.
//
// What the float statements add: trail_anchor subtracts 2^-19 (|s2| + 2 R) + 2^-39, which is more than
// err(s2) + 2^-20 |s2|; the second term covers the rounding of the four subtractions from s2 down to
// the compare (each at most 2^-24 of a value bounded by |s2| + delta, and delta < |s2| + |F| where the
// rule accepts; eps's slack covers the |F| part). eps is taken at |p|_inf + 0.002, which bounds it at
// p and at getNormal's six probes of p.
//
// F_w(p) is (k + sqrt(len2)) - rad with the box form of either primitive (rmr_trace.h prim_dist_at:
// a sphere is the box of half-extent 0 minus its radius, bit-identical to sd_sphere at points without
// NaN). The kernel's square root is sqrt_cr_big, equal to the correctly rounded one for len2 = 0 and
// len2 >= 2^-96 only, so other values are refused, as are points that are not finite.
//
// A hit found on a trailing step carries the one-primitive certificate of getNormal's probes (the cache
// kernels' form, rmr_trace.h march_update CACHE): every probe q lies within h (1 + 2^-21) <=
// NPC_PROBE_DELTA of p, so F_j(q) >= bound - delta - NPC_PROBE_DELTA - eps for j != w and F_w(q) <= F_w(p)
// + NPC_PROBE_DELTA + 2 eps: w is the strict minimiser at all six when bound - delta - 2 NPC_PROBE_DELTA
// - 3 eps > F_w(p). A hit without it parks uncertified and the batch probes run the whole map.
#pragma once
#ifndef __HIPCC_RTC__
#include <math.h>
#endif

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define RMR_TRAIL_HD __host__ __device__ inline
#else
#define RMR_TRAIL_HD inline
#endif

namespace rmr {

constexpr float kTrailProbeDelta = 0.0010001f;   // rmr_trace.h NPC_PROBE_DELTA
constexpr int kTrailMaxSteps = 3;                // trailing steps per map-loop iteration (two bits of the launch word)

// |p|_inf
RMR_TRAIL_HD float trail_linf(float x, float y, float z) { return fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z))); }
// eps(x) from |x|_inf; eps0 = 2^-17 E + 2^-60 (KParams::npc_eps0)
RMR_TRAIL_HD float trail_eps(float linf, float eps0) { return fmaf(linf, 0x1p-17f, eps0); }
// neither NaN nor infinite (a sum that overflows refuses a finite point, which is allowed)
RMR_TRAIL_HD bool trail_finite(float x, float y, float z) {
    const float s = (x + y) + z;
    return s - s == 0.0f;
}
// The anchor's bound: below every F_j(p0), j != w, by the rule's own rounding and eps(p0). r2 = 2 R.
// An infinite or NaN s2 (a one-primitive scene, a NaN point) gives NaN or +-inf; NaN refuses every
// step, and +inf is right: no other primitive.
RMR_TRAIL_HD float trail_anchor(float s2, float r2, float eps_p0) {
    return (s2 - fmaf(fabsf(s2) + r2, 0x1p-19f, 0x1p-39f)) - eps_p0;
}
// the box form's two parts at q = |p - c| - half-extent: k = min(max q, 0), len2 = |max(q, 0)|^2
RMR_TRAIL_HD float trail_k(float qx, float qy, float qz) { return fminf(fmaxf(qx, fmaxf(qy, qz)), 0.0f); }
RMR_TRAIL_HD float trail_len2(float qx, float qy, float qz) {
    const float ox = fmaxf(qx, 0.0f), oy = fmaxf(qy, 0.0f), oz = fmaxf(qz, 0.0f);
    return fmaf(ox, ox, fmaf(oy, oy, oz * oz));   // rmr_math.h dot
}

struct TrailStep {
    bool accept;   // map(p) is (F, id_w): take the march step with it
    bool cert;     // ... and, should it be a hit, getNormal's six probes have w as their minimiser too
};
// anchor: trail_anchor at the lane's last full map; t0 its ray parameter; (t, linf, fin): the trailing
// point's parameter, |p|_inf and trail_finite; (F, len2): primitive w there; eps0: KParams::npc_eps0;
// am_dmax: KParams::am_dmax. Every comparison is false for a NaN operand.
RMR_TRAIL_HD TrailStep trail_rule(float anchor, float t0, float t, float linf, bool fin, float F, float len2, float eps0,
                                  float am_dmax) {
    const float delta = (t - t0) * (1.0f + 0x1p-21f);
    const float b = anchor - delta;
    const float eps = trail_eps(linf + 0.002f, eps0);
    const bool big = (len2 == 0.0f) | (len2 >= 0x1p-96f);
    TrailStep r;
    r.accept = fin & big & (b - eps > F) & (F < am_dmax);
    // (|b| 2^-20: this test's own rounding, as the cache kernels' certificate)
    r.cert = r.accept & (b - fmaf(fabsf(b), 0x1p-20f, fmaf(3.0f, eps, 2.0f * kTrailProbeDelta)) > F);
    return r;
}

}  // namespace rmr
