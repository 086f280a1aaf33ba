// rmr_aov_rule.h — the sampled AOVs' rule (include/rmr.h rmr_render_aov), written once
// for the host (aov.cpp) and the device (rmr_aov.hip): the per-pixel state, the fold of one sample's first
// hit into it, and the resolve of a state into the four output planes.
// Plain C++ and HIP: no library call but the correctly rounded square root, no fused multiply-add, every
// select a comparison, so both sides run the same operations and NumPy float32 / float64 reproduces them
// (tests/aov_ref.py).
#pragma once
#include <stdint.h>
#include "../../include/rmr.h"

#if defined(__HIP__)
#define RMR_AOV_HD __host__ __device__ inline
#else
#define RMR_AOV_HD inline
#endif

namespace rmr {

constexpr int kAovPlanes = 5;            // state planes (RMR_AOV_*), float4 per pixel each: 80 B
constexpr int kAovResolved = 5;          // resolved planes (RMR_AOV_R_*), float4 per pixel each
constexpr float kAovMaxSamples = 16777216.0f;   // 2^24: float32 counts are exact up to here

struct Aov4 {
    float x, y, z, w;
};

// One pixel's state, in plane order: stats (n, h, sum_t, min_t), normal (sum n, other), position (sum pos, 0),
// ids01 (id0, c0, id1, c1), ids23 (id2, c2, id3, c3).
struct AovState {
    Aov4 stats, nrm, pos, ids01, ids23;
};

RMR_AOV_HD AovState aov_initial() {
    AovState s;
    s.stats = Aov4{0.0f, 0.0f, 0.0f, __builtin_inff()};
    s.nrm = Aov4{0.0f, 0.0f, 0.0f, 0.0f};
    s.pos = Aov4{0.0f, 0.0f, 0.0f, 0.0f};
    s.ids01 = Aov4{-1.0f, 0.0f, -1.0f, 0.0f};
    s.ids23 = Aov4{-1.0f, 0.0f, -1.0f, 0.0f};
    return s;
}

// fminf without the library: the smaller of a and b; a NaN loses to a number (t of a hit is never NaN).
RMR_AOV_HD float aov_min(float a, float b) { return b < a ? b : (a != a ? b : a); }

// The fold of one sample (pos, t, n, id), an rmr_hit as k_cast_rays<NP, true> produces it: id < 0 is a
// miss (a far hit, t >= maxDist, already has id -1 there). The slots are written without an index, so the
// state stays in registers.
RMR_AOV_HD void aov_fold1(AovState& s, float px, float py, float pz, float t, float nx, float ny, float nz, float id) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    s.stats.x = s.stats.x + 1.0f;
    if (id < 0.0f) return;
    s.stats.y = s.stats.y + 1.0f;
    s.stats.z = s.stats.z + t;
    s.stats.w = aov_min(s.stats.w, t);
    s.nrm.x = s.nrm.x + nx;
    s.nrm.y = s.nrm.y + ny;
    s.nrm.z = s.nrm.z + nz;
    s.pos.x = s.pos.x + px;
    s.pos.y = s.pos.y + py;
    s.pos.z = s.pos.z + pz;
    // the first slot holding the id, else the first empty slot, else `other`
    const bool e0 = s.ids01.x == id, e1 = s.ids01.z == id, e2 = s.ids23.x == id, e3 = s.ids23.z == id;
    const bool any = e0 || e1 || e2 || e3;
    const bool f0 = !any && s.ids01.x == -1.0f;
    const bool f1 = !any && !f0 && s.ids01.z == -1.0f;
    const bool f2 = !any && !f0 && !f1 && s.ids23.x == -1.0f;
    const bool f3 = !any && !f0 && !f1 && !f2 && s.ids23.z == -1.0f;
    const bool m0 = e0, m1 = !e0 && e1, m2 = !e0 && !e1 && e2, m3 = !e0 && !e1 && !e2 && e3;
    s.ids01.y = m0 ? s.ids01.y + 1.0f : (f0 ? 1.0f : s.ids01.y);
    s.ids01.x = f0 ? id : s.ids01.x;
    s.ids01.w = m1 ? s.ids01.w + 1.0f : (f1 ? 1.0f : s.ids01.w);
    s.ids01.z = f1 ? id : s.ids01.z;
    s.ids23.y = m2 ? s.ids23.y + 1.0f : (f2 ? 1.0f : s.ids23.y);
    s.ids23.x = f2 ? id : s.ids23.x;
    s.ids23.w = m3 ? s.ids23.w + 1.0f : (f3 ? 1.0f : s.ids23.w);
    s.ids23.z = f3 ? id : s.ids23.z;
    s.nrm.w = (any || f0 || f1 || f2 || f3) ? s.nrm.w : s.nrm.w + 1.0f;
}

// The resolved planes of one pixel, in plane order (RMR_AOV_R_*).
struct AovResolved {
    Aov4 depth, nrm, pos, ids01, ids23;
};

// slot a sorts before slot b: a used slot before an empty one, then count descending, then id ascending
RMR_AOV_HD bool aov_before(float ida, float ca, float idb, float cb) {
    const bool ua = !(ida < 0.0f), ub = !(idb < 0.0f);
    if (ua != ub) return ua;
    if (!ua) return false;
    return ca > cb || (ca == cb && ida < idb);
}
RMR_AOV_HD void aov_cswap(float& ida, float& ca, float& idb, float& cb) {
    if (aov_before(idb, cb, ida, ca)) {
        const float ti = ida, tc = ca;
        ida = idb; ca = cb;
        idb = ti; cb = tc;
    }
}

RMR_AOV_HD AovResolved aov_resolve1(const AovState& s, float max_dist) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    AovResolved r;
    const float n = s.stats.x, h = s.stats.y;
    const float alpha = n > 0.0f ? h / n : 0.0f;
    r.depth.x = h > 0.0f ? s.stats.z / h : max_dist;
    r.depth.y = h > 0.0f ? s.stats.w : max_dist;
    r.depth.z = alpha;
    r.depth.w = n;
    const float xx = s.nrm.x * s.nrm.x, yy = s.nrm.y * s.nrm.y, zz = s.nrm.z * s.nrm.z;
    const float len = __builtin_sqrtf((xx + yy) + zz);
    const bool have_n = h > 0.0f && len > 0.0f && __builtin_isfinite(len);
    r.nrm.x = have_n ? s.nrm.x / len : 0.0f;
    r.nrm.y = have_n ? s.nrm.y / len : 0.0f;
    r.nrm.z = have_n ? s.nrm.z / len : 0.0f;
    r.nrm.w = alpha;
    const bool have_p = h > 0.0f;
    r.pos.x = have_p ? s.pos.x / h : 0.0f;
    r.pos.y = have_p ? s.pos.y / h : 0.0f;
    r.pos.z = have_p ? s.pos.z / h : 0.0f;
    r.pos.w = have_p ? h : 0.0f;
    // the four slots through a five-comparator sorting network; (id, count) pairs are distinct unless empty
    float i0 = s.ids01.x, c0 = s.ids01.y, i1 = s.ids01.z, c1 = s.ids01.w;
    float i2 = s.ids23.x, c2 = s.ids23.y, i3 = s.ids23.z, c3 = s.ids23.w;
    aov_cswap(i0, c0, i1, c1);
    aov_cswap(i2, c2, i3, c3);
    aov_cswap(i0, c0, i2, c2);
    aov_cswap(i1, c1, i3, c3);
    aov_cswap(i1, c1, i2, c2);
    // coverage c / n; an empty slot stays (-1, 0) (a used slot implies n > 0)
    r.ids01.x = i0; r.ids01.y = i0 < 0.0f ? 0.0f : c0 / n;
    r.ids01.z = i1; r.ids01.w = i1 < 0.0f ? 0.0f : c1 / n;
    r.ids23.x = i2; r.ids23.y = i2 < 0.0f ? 0.0f : c2 / n;
    r.ids23.z = i3; r.ids23.w = i3 < 0.0f ? 0.0f : c3 / n;
    return r;
}

}  // namespace rmr
