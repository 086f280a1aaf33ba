// rmr_trail_rule.h — the acceptance rule of the lane-slot kernels' trailing steps (rmr_trace.h
// RMR_TRAIL_STEPS, trace_main), as arithmetic on plain floats. The kernel and the host programs
// csrc/trail_rule_test.cpp (the first statements: trail_anchor, trail_rule) and csrc/trail_lean_test.cpp (the
// statements the kernel runs: trail_anchor_hi, trail_rule_hi, trail_row) compile these statements.
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
// The launch's eps_hi (KParams::trail_eps_hi, accel.cpp trail_eps_bound) stands for eps(p0) and eps(p):
// eps_hi = RU(2^-17 (B + 0.002 + E) + 2^-60), where B bounds |x|_inf over every point x a pass or its anchor
// can evaluate, so eps_hi >= eps(x) there and at getNormal's six probes of x (the 0.002). The bound B:
//   * a lane takes part in a pass only while it marches from outside (not L.inside) with a finite anchor;
//   * trail_anchor_hi is NaN where a coordinate of p0 is not finite (its 0 x p0 terms), and any NaN or
//     infinite coordinate of the ray's origin o or direction d makes that coordinate of p0 = fma(d, t0, o) NaN
//     or infinite; so o and d are finite, and ray_exit gave the march a finite escape bound texit;
//   * march_update ends a march whose t passes texit, so 0 <= t <= texit, and x = fma(d, t, o) lies, up
//     to its rounding, on the segment from o to the ray's exit from the inflated escape boxes, whose ends
//     bound |x|_inf (the norm is convex);
//   * o is the eye, or a bounce origin: a hit point (within 0.001 of a primitive, plus its float error,
//     which the boxes' inflation covers) moved 0.003 along the normal; the exit lies on a face of an
//     inflated box up to ray_exit's slab error 2^-21 (|B| + |o|) and its widening of texit by 2^-19.
//   So B = (max(|eye|_inf, max corner |.|_inf of the inflated boxes) + 0.01) (1 + 2^-15), the factor being
//   far more than the slab error, the widening and the FMA's rounding together.
// Where the launch has no escape bound, or B is not finite, the host passes eps_hi = +inf and K = 0: the
// anchor is then -inf or NaN, the rule refuses every lane, and no pass runs.
//
// The float statements (trail_anchor_hi, trail_rule_hi). The anchor subtracts
// 2^-19 (|s2| + 2 R) + 2^-39 + 2 eps_hi from s2 in one fma and one subtraction: 2^-19 (|s2| + 2 R) + 2^-39 is
// more than err(s2) + 2^-20 |s2|, and the second term covers the rounding of the two subtractions from s2
// down to the compare, anchor - delta > F (each at most 2^-24 of a value bounded by |s2| + delta, and delta
// < |s2| + |F| where the rule accepts; eps's slack covers the |F| part and the rounding of the constant
// 2^-39 + 2 eps_hi). 2 eps_hi >= eps(p0) + eps(p).
//
// F_w(p) is (k + sqrt(len2)) - rad with the box form of either primitive (trail_row: a sphere is the box
// of half-extent 0 minus its radius, a box subtracts the radius 0; bit-identical to sd_sphere / sd_box at
// points without NaN). The kernel's square root is sqrt_cr_big, equal to the correctly rounded one for
// len2 = 0 and len2 >= 2^-96 only, so other values are refused.
//
// Points that are not finite need no test of their own in a pass:
//  1. a p0 with a coordinate that is NaN or infinite gives a NaN anchor (above), which refuses every step;
//  2. with p0 finite, o and d are finite (above). For finite t, p = fma(d, t, o) can only overflow, to
//     +-inf in a coordinate; t = +inf or NaN gives delta = +inf or NaN, and anchor - delta > F is false;
//  3. an infinite coordinate of p gives |p - c| - h = +inf there, len2 = +inf, k = 0 and F = +inf, which
//     fails F < am_dmax (am_dmax is finite or -inf).
//
// A hit found on a trailing step carries the one-primitive certificate of getNormal's probes (the cache
// kernels' form, rmr_trace.h march_update CACHE): every probe q lies within h (1 + 2^-21) <=
// NPC_PROBE_DELTA of p, so F_j(q) >= bound - delta - NPC_PROBE_DELTA - eps for j != w and F_w(q) <= F_w(p)
// + NPC_PROBE_DELTA + 2 eps: w is the strict minimiser at all six when bound - delta - 2 NPC_PROBE_DELTA
// - 3 eps > F_w(p). With b = anchor - delta, which has 2 eps_hi subtracted already, the statement takes
// another 3 eps_hi + 2 NPC_PROBE_DELTA, a launch constant, and |b| 2^-20 for its own rounding. A hit without
// the certificate parks uncertified and the batch probes run the whole map.
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
constexpr int kTrailMaxSteps = 15;               // trailing passes per map-loop iteration (four bits of the launch word)
constexpr int kTrailMaxRatio = 8;                // the pass rule's ratio in eighths (8: every active lane takes part)

// The trailing passes' launch word, bits 16-24 of the lane-slot kernels' KParams::shade_threshold (below them
// the park and the batch thresholds): after each pass a wave takes another one iff fewer than k_max have run,
// (park_exit) its finished lanes are still fewer than the park threshold, and 8 x the lanes still taking
// part >= ratio x its active lanes (ratio 0: no lane test). (k, 0, false) is the fixed schedule of k passes.
constexpr int kTrailWordShift = 16;
RMR_TRAIL_HD int trail_word(int k_max, int ratio, bool park_exit) { return k_max | (ratio << 4) | ((int)park_exit << 8); }
RMR_TRAIL_HD int trail_word_k(int word) { return word & 15; }
RMR_TRAIL_HD int trail_word_ratio(int word) { return (word >> 4) & 15; }
RMR_TRAIL_HD bool trail_word_park_exit(int word) { return ((word >> 8) & 1) != 0; }
RMR_TRAIL_HD bool trail_word_valid(int k_max, int ratio, int park_exit) {
    return k_max >= 0 && k_max <= kTrailMaxSteps && ratio >= 0 && ratio <= kTrailMaxRatio && (park_exit == 0 || park_exit == 1);
}

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

// ---- the statements the kernel runs (launch-constant eps, box-form table row) ----

// The table row a pass consumes: c.xyz, h.x | h.yz, rad, mid. A sphere has h = 0 and rad = r.x, a box
// h = r and rad = 0, so that (trail_k + sqrt(trail_len2)) - rad at q = |p - c| - h has sd_sphere's / sd_box's bits.
RMR_TRAIL_HD void trail_row(bool box, float cx, float cy, float cz, float rx, float ry, float rz, float mid, float* row) {
    row[0] = cx;
    row[1] = cy;
    row[2] = cz;
    row[3] = box ? rx : 0.0f;
    row[4] = box ? ry : 0.0f;
    row[5] = box ? rz : 0.0f;
    row[6] = box ? 0.0f : rx;
    row[7] = mid;
}
RMR_TRAIL_HD float trail_row_dist(const float* row, float px, float py, float pz, float sqrt_len2) {
    const float qx = fabsf(px - row[0]) - row[3], qy = fabsf(py - row[1]) - row[4], qz = fabsf(pz - row[2]) - row[5];
    return (trail_k(qx, qy, qz) + sqrt_len2) - row[6];
}
// the launch's two constants from eps_hi (KParams::trail_eps_hi): the anchor's and the certificate's
RMR_TRAIL_HD float trail_anchor_const(float eps_hi) { return fmaf(2.0f, eps_hi, 0x1p-39f); }
RMR_TRAIL_HD float trail_cert_const(float eps_hi) { return fmaf(3.0f, eps_hi, 2.0f * kTrailProbeDelta); }
// The anchor's bound: below every F_j(p), j != w, by the rule's own rounding, eps(p0) and eps(p). r2 = 2 R,
// ak = trail_anchor_const. (x0, y0, z0) = p0: 0 x p0 is +-0 for a finite coordinate and NaN otherwise, and
// r2 + (+-0) is r2 (a +0 for r2 = 0), so a p0 that is not finite gives NaN and a finite one changes no bit.
// An infinite or NaN s2 (a one-primitive scene, a NaN point) gives NaN or +-inf; NaN refuses every
// step, and +inf is right: no other primitive.
RMR_TRAIL_HD float trail_anchor_hi(float s2, float r2, float ak, float x0, float y0, float z0) {
    const float r2p = fmaf(x0, 0.0f, fmaf(y0, 0.0f, fmaf(z0, 0.0f, r2)));
    return s2 - fmaf(fabsf(s2) + r2p, 0x1p-19f, ak);
}
// anchor: trail_anchor_hi at the lane's last full map; t0 its ray parameter; t: the trailing point's
// parameter; (F, len2): primitive w there; ck: trail_cert_const; am_dmax: KParams::am_dmax. Every
// comparison is false for a NaN operand.
// The rule's five comparisons, one by one: the kernel forms the wave's mask of accepting lanes from the
// comparisons' own masks (trail_accept of every lane at once), which costs it no vector instruction.
struct TrailTests {
    bool zero, big;   // len2 is 0 / at least 2^-96: the square root is the correctly rounded one
    bool below;       // F is under the bound
    bool nearer;      // F < am_dmax
    bool probes;      // ... under the bound less the certificate's margin
};
RMR_TRAIL_HD TrailTests trail_tests_hi(float anchor, float t0, float t, float F, float len2, float ck, float am_dmax) {
    const float delta = (t - t0) * (1.0f + 0x1p-21f);
    const float b = anchor - delta;
    TrailTests c;
    c.zero = len2 == 0.0f;
    c.big = len2 >= 0x1p-96f;
    c.below = b > F;
    c.nearer = F < am_dmax;
    c.probes = b - fmaf(fabsf(b), 0x1p-20f, ck) > F;
    return c;
}
RMR_TRAIL_HD bool trail_accept(const TrailTests& c) { return (c.zero | c.big) & c.below & c.nearer; }
RMR_TRAIL_HD TrailStep trail_rule_hi(float anchor, float t0, float t, float F, float len2, float ck, float am_dmax) {
    const TrailTests c = trail_tests_hi(anchor, t0, t, F, len2, ck, am_dmax);
    TrailStep r;
    r.accept = trail_accept(c);
    r.cert = r.accept & c.probes;
    return r;
}

}  // namespace rmr
