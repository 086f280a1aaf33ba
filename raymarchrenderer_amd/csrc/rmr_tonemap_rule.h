// rmr_tonemap_rule.h — the tone-mapping stage's rule (include/rmr.h rmr_tonemap),
// written once for the host (tonemap.cpp) and the device (rmr_tonemap.hip): the luminance bin of a
// pixel, the metering of a histogram and the three curves.
// Plain C++ and HIP: no library call and no fused multiply-add, so both sides run the same operations
// and NumPy float32 / float64 reproduces them (tests/tonemap_ref.py).
#pragma once
#include <stdint.h>
#include "../../include/rmr.h"

#if defined(__HIP__)
#define RMR_TM_HD __host__ __device__ inline
#else
#define RMR_TM_HD inline
#endif

namespace rmr {

constexpr int kToneBins = 256;
constexpr int kToneSkipped = 256;      // the word after the bins: pixels that are not counted
constexpr int kToneWords = 257;
constexpr int kToneBinBias = (127 - 16) << 3;

RMR_TM_HD uint32_t tone_bits(float x) { return __builtin_bit_cast(uint32_t, x); }

// The luminance bin of a pixel, 0..255, or -1 for a pixel that is skipped.
RMR_TM_HD int lum_bin(float r, float g, float b, float a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float pr = 0.2126f * r, pg = 0.7152f * g, pb = 0.0722f * b;
    const float L = (pr + pg) + pb;
    const bool counted = a != 0.0f && __builtin_isfinite(r) && __builtin_isfinite(g) && __builtin_isfinite(b) &&
                         __builtin_isfinite(L) && L >= 0.0f;
    if (!counted) return -1;
    // (the sign bit dropped: L = -0 passes L >= 0 and belongs to bin 0)
    const int k = (int)((tone_bits(L) & 0x7fffffffu) >> 20) - kToneBinBias;
    return k < 0 ? 0 : (k > 255 ? 255 : k);
}

// What the meter needs beside the histogram (made on the host: tonemap.cpp meter_setup).
struct ToneMeter {
    double low, high;        // (double)low_pct, (double)high_pct
    double log2_key;         // log2((double)key)
    double ev;               // (double)exposure_ev
    double adapt;            // (double)adapt
};

// l of the metering rule. hist: the 256 bins (bin 0 is not metered); lc: lc[b - 1] is bin b's centre in
// log2, b = 1..255; has_prev / l_prev: the adaptation state.
//
// The three parts, so that the device can give each bin's weight a thread of its own (k_meter) and
// still add them in bin order. The cumulative count is an integer (below 2^53, so the double of it is
// the running double sum the rule states).
// One bin: C pixels in the metered bins before it, n in it, of N in all. w = its overlap with the
// window, t = w lc_b.
RMR_TM_HD void meter_bin(uint64_t C, uint32_t n, uint64_t N, const ToneMeter& M, double lc_b, double& w, double& t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double lo = M.low * (double)N, hi = M.high * (double)N;
    const double c0 = (double)C, c1 = (double)(C + n);
    const double a = c0 > lo ? c0 : lo, z = c1 < hi ? c1 : hi;
    w = z > a ? z - a : 0.0;
    t = w * lc_b;
}

// l from the sums over the bins in order (sw > 0: the window of a non-empty histogram is not empty).
RMR_TM_HD double meter_finish(double swl, double sw, const ToneMeter& M, bool has_prev, double l_prev) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double mean = swl / sw;
    const double target = (M.log2_key - mean) + M.ev;
    if (!has_prev) return target;
    const double d = target - l_prev;
    const double s = M.adapt * d;
    return l_prev + s;
}

RMR_TM_HD double meter_l(const uint32_t* hist, const double* lc, const ToneMeter& M, bool has_prev, double l_prev) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    uint64_t N = 0;
    for (int b = 1; b < kToneBins; b++) N += hist[b];
    if (N == 0) return has_prev ? l_prev : M.ev;
    uint64_t C = 0;
    double sw = 0.0, swl = 0.0;
    for (int b = 1; b < kToneBins; b++) {
        double w, t;
        meter_bin(C, hist[b], N, M, lc[b - 1], w, t);
        swl = swl + t;
        sw = sw + w;
        C += hist[b];
    }
    return meter_finish(swl, sw, M, has_prev, l_prev);
}

// One colour channel through the curve. iw2: (float)(1 / white^2), used by RMR_TONE_REINHARD only.
// The selects are fmaxf / fminf with their NaN rule (the other operand) spelled out, and a -0 product
// reads as +0, so that no result depends on how a library orders the two zeros.
RMR_TM_HD float tone_curve(int curve, float c, float scale, float iw2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float t = c * scale;
    const float x = t > 0.0f ? t : 0.0f;
    float v;
    if (curve == RMR_TONE_LINEAR) {
        v = x;
    } else if (curve == RMR_TONE_REINHARD) {
        const float xi = x * iw2;
        const float num = x * (1.0f + xi);
        v = num / (1.0f + x);
    } else {
        const float n1 = 2.51f * x, d1 = 2.43f * x;
        const float num = x * (n1 + 0.03f);
        const float den = x * (d1 + 0.59f) + 0.14f;
        v = num / den;
    }
    const float m = v < 1.0f ? v : 1.0f;   // fminf(v, 1): NaN gives 1
    return m > 0.0f ? m : 0.0f;            // fmaxf(m, 0)
}

}  // namespace rmr
