// tonemap.cpp — see tonemap.hpp. No HIP: built into librmr.so and, with tonemap_test.cpp, into a
// stand-alone CPU check (plain and under the sanitizers). The context-free entry points run the same
// header the kernels compile (rmr_tonemap_rule.h).
#include "tonemap.hpp"

#include <cmath>

namespace rmr {

bool tonemap_params_ok(const rmr_tonemap_params& p) {
    return p.curve >= RMR_TONE_LINEAR && p.curve <= RMR_TONE_ACES && (p.auto_exposure == 0 || p.auto_exposure == 1) &&
           std::isfinite(p.exposure_ev) && std::fabs(p.exposure_ev) <= 32.0f && std::isfinite(p.key) && p.key > 0.0f &&
           p.low_pct >= 0.0f && p.low_pct < p.high_pct && p.high_pct <= 1.0f && p.adapt > 0.0f && p.adapt <= 1.0f &&
           std::isfinite(p.white) && p.white > 0.0f;
}

void tonemap_lc_table(double lc[255]) {
    for (int b = 1; b < kToneBins; b++) {
        const int e = (b >> 3) - 16, m = b & 7;
        lc[b - 1] = (double)e + std::log2(1.0 + ((double)m + 0.5) / 8.0);
    }
}

ToneMeter tonemap_meter(const rmr_tonemap_params& p) {
    ToneMeter M;
    M.low = (double)p.low_pct;
    M.high = (double)p.high_pct;
    M.log2_key = std::log2((double)p.key);
    M.ev = (double)p.exposure_ev;
    M.adapt = (double)p.adapt;
    return M;
}

float tonemap_iw2(const rmr_tonemap_params& p) { return (float)(1.0 / ((double)p.white * (double)p.white)); }

}  // namespace rmr

extern "C" {

void rmr_default_tonemap_params(rmr_tonemap_params* p) {
    if (!p) return;
    p->curve = RMR_TONE_ACES;
    p->auto_exposure = 0;
    p->exposure_ev = 0.0f;
    p->key = 0.18f;
    p->low_pct = 0.10f;
    p->high_pct = 0.90f;
    p->adapt = 1.0f;
    p->white = 4.0f;
}

int rmr_check_tonemap_params(const rmr_tonemap_params* p) {
    return p && rmr::tonemap_params_ok(*p) ? RMR_OK : RMR_E_INVALID;
}

int rmr_luminance_bins(const float* rgba, size_t n, int32_t* bins) {
    if ((!rgba || !bins) && n) return RMR_E_INVALID;
    for (size_t i = 0; i < n; i++) bins[i] = rmr::lum_bin(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]);
    return RMR_OK;
}

int rmr_exposure_from_histogram(const uint32_t hist[256], const rmr_tonemap_params* p, double l_prev, double* l_out) {
    if (!hist || !l_out) return RMR_E_INVALID;
    rmr_tonemap_params q;
    rmr_default_tonemap_params(&q);
    if (p) q = *p;
    if (!rmr::tonemap_params_ok(q) || std::isinf(l_prev)) return RMR_E_INVALID;
    double lc[255];
    rmr::tonemap_lc_table(lc);
    const bool has_prev = !std::isnan(l_prev);
    *l_out = rmr::meter_l(hist, lc, rmr::tonemap_meter(q), has_prev, has_prev ? l_prev : 0.0);
    return RMR_OK;
}

int rmr_tonemap_pixels(const rmr_tonemap_params* p, float scale, const float* rgba, size_t n, float* out) {
    if ((!rgba || !out) && n) return RMR_E_INVALID;
    rmr_tonemap_params q;
    rmr_default_tonemap_params(&q);
    if (p) q = *p;
    if (!rmr::tonemap_params_ok(q)) return RMR_E_INVALID;
    const float iw2 = rmr::tonemap_iw2(q);
    for (size_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) out[4 * i + k] = rmr::tone_curve(q.curve, rgba[4 * i + k], scale, iw2);
        out[4 * i + 3] = rgba[4 * i + 3];
    }
    return RMR_OK;
}

}  // extern "C"
