// rmr_bloom_rule.h — the HDR bloom stage's rule (include/rmr.h rmr_bloom), written once
// for the host (bloom.cpp) and the device (rmr_bloom.hip): the bright part of a pixel, the 4-tap down
// filter, the 2-tap up filter, the level sizes and the final add.
// Plain C++ and HIP: no library call and no fused multiply-add, every select a comparison, so both sides
// run the same operations and NumPy float32 / float64 reproduces them (tests/bloom_ref.py).
#pragma once
#include <stdint.h>
#include "../../include/rmr.h"

#if defined(__HIP__)
#define RMR_BL_HD __host__ __device__ inline
#else
#define RMR_BL_HD inline
#endif

namespace rmr {

constexpr int kBloomMaxLevels = 8;

struct Bloom3 {
    float x, y, z;
};

RMR_BL_HD int bloom_half(int n) { return (n + 1) >> 1; }
RMR_BL_HD int bloom_cl(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// A pixel the stage spreads nothing from and copies bit for bit.
RMR_BL_HD bool bloom_invalid(float r, float g, float b, float a) {
    return a == 0.0f || !__builtin_isfinite(r) || !__builtin_isfinite(g) || !__builtin_isfinite(b);
}

// The bright part P of a source pixel. max(c, 0) is `c > 0 ? c : +0`: either zero (and every negative)
// reads as +0, so P has no -0 and no result depends on a zero's sign.
RMR_BL_HD Bloom3 bloom_bright(float r, float g, float b, float a, float T, float clamp) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const Bloom3 zero = {0.0f, 0.0f, 0.0f};
    if (bloom_invalid(r, g, b, a)) return zero;
    const float cr = r > 0.0f ? r : 0.0f, cg = g > 0.0f ? g : 0.0f, cb = b > 0.0f ? b : 0.0f;
    const float pr = 0.2126f * cr, pg = 0.7152f * cg, pb = 0.0722f * cb;
    const float L = (pr + pg) + pb;
    if (!__builtin_isfinite(L)) return zero;
    float e = L - T;
    if (!(e > 0.0f)) return zero;
    if (clamp > 0.0f && e > clamp) e = clamp;
    const float f = e / L;
    const Bloom3 p = {cr * f, cg * f, cb * f};
    return p;
}

// d_j of the down filter from a[cl(i-1)], a[cl(i)], a[cl(i+1)], a[cl(i+2)], i = 2j.
RMR_BL_HD float bloom_down1(float am, float a0, float a1, float a2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float outer = am + a2;
    const float inner = a0 + a1;
    const float t = 3.0f * inner;
    return (outer + t) * 0.125f;
}

// u_i of the up filter from b[j] and b[cl(i odd ? j+1 : j-1)], j = i >> 1.
RMR_BL_HD float bloom_up1(float near, float far) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float t = 3.0f * near;
    return (t + far) * 0.25f;
}

// The far tap of the up filter at i, of m values.
RMR_BL_HD int bloom_up_far(int i, int m) { return bloom_cl((i & 1) ? (i >> 1) + 1 : (i >> 1) - 1, m); }

RMR_BL_HD Bloom3 bloom_down3(const Bloom3& am, const Bloom3& a0, const Bloom3& a1, const Bloom3& a2) {
    const Bloom3 d = {bloom_down1(am.x, a0.x, a1.x, a2.x), bloom_down1(am.y, a0.y, a1.y, a2.y),
                      bloom_down1(am.z, a0.z, a1.z, a2.z)};
    return d;
}

RMR_BL_HD Bloom3 bloom_up3(const Bloom3& near, const Bloom3& far) {
    const Bloom3 u = {bloom_up1(near.x, far.x), bloom_up1(near.y, far.y), bloom_up1(near.z, far.z)};
    return u;
}

// U_k = B_k + s up: the product rounded first, then the sum.
RMR_BL_HD float bloom_mad(float base, float s, float v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float t = s * v;
    return base + t;
}

// gain = (float)((double)I / sum_{j<N} (double)s^j), on the host.
inline float bloom_gain(float intensity, float scatter, int levels) {
    double sum = 0.0, pw = 1.0;
    for (int j = 0; j < levels; j++) {
        sum += pw;
        pw *= (double)scatter;
    }
    return (float)((double)intensity / sum);
}

}  // namespace rmr
