// rmr_bake_rule.h — the parts of the light bake's rule (include/rmr.h rmr_bake_points) that
// the host (bake.cpp) and the device (rmr_bake.hip) share: a point's invocation, the reject rule, the frame
// normal of the degenerate case, the ray's origin, the cosine and the fold over a point's samples.
// Plain C++ and HIP: float32 sums, products and quotients, fma only where the header writes it, every select
// a comparison, so both sides run the same operations and NumPy reproduces them (tests/bake_ref.py).
#pragma once
#include <stdint.h>
#include "../../include/rmr.h"

#if defined(__HIP__)
#define RMR_BAKE_HD __host__ __device__ inline
#else
#define RMR_BAKE_HD inline
#endif

namespace rmr {

constexpr uint64_t kBakeMaxIndex = (uint64_t)1 << 36;   // idx < 2^36: gy = idx >> 12 < 2^24, so gy + time is one rounding
constexpr int kBakeFlags = RMR_BAKE_RADIANCE | RMR_BAKE_AO;

// What every bake kernel reads of the call.
struct BakeList {
    const float* points;    // [n][3]
    const float* normals;   // [n][3]
    uint64_t n;
    uint64_t first_index;
    const float* times;     // [nspp], device
    uint32_t nspp;
    float bias;
    float extent;           // the caller's bound on |origin coordinate| (+inf: none)
};

// the invocation of list index idx = first_index + i: a 4096-wide image of points
RMR_BAKE_HD int32_t bake_gx(uint64_t idx) { return (int32_t)(idx & 4095u); }
RMR_BAKE_HD int32_t bake_gy(uint64_t idx) { return (int32_t)(idx >> 12); }

// A point is used iff every coordinate of p and n is finite and |n.n - 1| <= 1e-6. The length test is in
// double, each product and sum rounded on its own (as rmr_ray_check.h ray_ok: a fused n.n would move the
// verdict of a normal at the bound between the host and the device).
RMR_BAKE_HD bool bake_point_ok(const float p[3], const float n[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && __builtin_isfinite(p[k]) && __builtin_isfinite(n[k]);
    const double x = (double)n[0], y = (double)n[1], z = (double)n[2];
    const double xx = x * x, yy = y * y, zz = z * z;
    const double nn = (xx + yy) + zz;
    const double e = nn - 1.0;
    return ok && (e < 0.0 ? -e : e) <= 1e-6;
}

// randHemisphere's frame vanishes for n.x == 0 && n.z == 0 (other than exactly (0, 1, 0)): such a normal
// samples about (0, 1, 0) and mirrors the direction's y when it points down.
RMR_BAKE_HD bool bake_degenerate(const float n[3]) { return n[0] == 0.0f && n[2] == 0.0f; }

// the ray's origin: o = fma(n, bias, p)
RMR_BAKE_HD void bake_origin(const float p[3], const float n[3], float bias, float o[3]) {
    for (int k = 0; k < 3; k++) o[k] = __builtin_fmaf(n[k], bias, p[k]);
}

// c = max(0, fma(n.z, d.z, fma(n.y, d.y, n.x * d.x)))
RMR_BAKE_HD float bake_cosine(const float n[3], const float d[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float xx = n[0] * d[0];
    const float c = __builtin_fmaf(n[2], d[2], __builtin_fmaf(n[1], d[1], xx));
    return c > 0.0f ? c : 0.0f;
}

// A point's running state over its samples in ascending k.
struct BakeState {
    float s[3];     // S: the sum of L_k c_k over the used samples
    float n_used;   // exact up to 2^24 samples
    float sum_c;    // the occlusion's denominator
    float sum_cv;   // and numerator
};
RMR_BAKE_HD void bake_state_init(BakeState& b) {
    b.s[0] = b.s[1] = b.s[2] = 0.0f;
    b.n_used = b.sum_c = b.sum_cv = 0.0f;
}
// S += L c (the product rounded, then the sum); a sample with a non-finite component of L is skipped
RMR_BAKE_HD void bake_fold_radiance(BakeState& b, float lr, float lg, float lb, float c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(__builtin_isfinite(lr) && __builtin_isfinite(lg) && __builtin_isfinite(lb))) return;
    const float pr = lr * c, pg = lg * c, pb = lb * c;
    b.s[0] = b.s[0] + pr;
    b.s[1] = b.s[1] + pg;
    b.s[2] = b.s[2] + pb;
    b.n_used = b.n_used + 1.0f;
}
RMR_BAKE_HD void bake_fold_ao(BakeState& b, float c, float cv) {
    b.sum_c = b.sum_c + c;
    b.sum_cv = b.sum_cv + cv;
}
// out.rgb = (S + S) / n_used, out.a = n_used; n_used == 0: rgb = 0
RMR_BAKE_HD void bake_resolve_radiance(const BakeState& b, float out[4]) {
    for (int k = 0; k < 3; k++) {
        const float two = b.s[k] + b.s[k];
        out[k] = b.n_used > 0.0f ? two / b.n_used : 0.0f;
    }
    out[3] = b.n_used;
}
// ao = sum_cv / sum_c; a denominator of 0: 1
RMR_BAKE_HD float bake_resolve_ao(const BakeState& b) { return b.sum_c == 0.0f ? 1.0f : b.sum_cv / b.sum_c; }

}  // namespace rmr
