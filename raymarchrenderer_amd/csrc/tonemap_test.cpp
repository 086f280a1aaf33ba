// tonemap_test.cpp — stand-alone CPU checks of tonemap.cpp (no HIP, no Python), run plain and under the
// address and undefined-behaviour sanitizers by tests/test_tonemap_cpu.py: the parameter ranges, and the
// three host functions on exactly sized heap arrays (bin edges, the curves' range and order, the meter
// on hand-made histograms).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "tonemap.hpp"

namespace {
int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

void check_params() {
    rmr_tonemap_params p;
    rmr_default_tonemap_params(&p);
    CHECK(p.curve == RMR_TONE_ACES && p.auto_exposure == 0 && p.exposure_ev == 0.0f && p.key == 0.18f);
    CHECK(p.low_pct == 0.10f && p.high_pct == 0.90f && p.adapt == 1.0f && p.white == 4.0f);
    CHECK(rmr_check_tonemap_params(&p) == RMR_OK);
    CHECK(rmr_check_tonemap_params(nullptr) == RMR_E_INVALID);
    rmr_default_tonemap_params(nullptr);
    auto bad = [&](auto set) {
        rmr_default_tonemap_params(&p);
        set(p);
        CHECK(rmr_check_tonemap_params(&p) == RMR_E_INVALID);
    };
    bad([](rmr_tonemap_params& q) { q.curve = 3; });
    bad([](rmr_tonemap_params& q) { q.curve = -1; });
    bad([](rmr_tonemap_params& q) { q.auto_exposure = 2; });
    for (float b : {33.0f, -33.0f, kNaN, kInf}) bad([b](rmr_tonemap_params& q) { q.exposure_ev = b; });
    for (float b : {0.0f, -1.0f, kNaN, kInf}) bad([b](rmr_tonemap_params& q) { q.key = b; });
    for (float b : {0.0f, -1.0f, kNaN, kInf}) bad([b](rmr_tonemap_params& q) { q.white = b; });
    for (float b : {0.0f, -0.5f, 1.5f, kNaN}) bad([b](rmr_tonemap_params& q) { q.adapt = b; });
    for (float b : {-0.1f, 0.9f, 1.0f, kNaN}) bad([b](rmr_tonemap_params& q) { q.low_pct = b; });
    for (float b : {0.1f, 0.05f, 1.1f, kNaN}) bad([b](rmr_tonemap_params& q) { q.high_pct = b; });
}

void check_bins() {
    // the rule's specials
    const size_t n = 12;
    std::vector<float> px(4 * n);
    std::vector<int32_t> bins(n);
    const float rows[n][4] = {{0, 0, 0, 1},        {-0.0f, -0.0f, -0.0f, 1}, {1, 1, 1, 0},    {kNaN, 0, 0, 1},
                              {0, kInf, 0, 1},     {0, 0, -kInf, 1},         {-1, 0, 0, 1},   {-1, 4, 0, 1},
                              {1e-30f, 1e-30f, 0, 1}, {3e38f, 3e38f, 3e38f, 1}, {1, 1, 1, 1}, {1e6f, 1e6f, 1e6f, kNaN}};
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 4; k++) px[4 * i + k] = rows[i][k];
    CHECK(rmr_luminance_bins(px.data(), n, bins.data()) == RMR_OK);
    const int32_t want[n] = {0, 0, -1, -1, -1, -1, -1, -2, 0, -2, -2, 255};
    for (size_t i = 0; i < n; i++)
        if (want[i] != -2) CHECK(bins[i] == want[i]);
    CHECK(bins[7] > 0 && bins[7] < 255);   // a negative channel with positive L is counted
    CHECK(bins[9] == 255);   // (the weights sum to 1: L stays finite)
    CHECK(bins[10] == ((127 << 3) - rmr::kToneBinBias) || bins[10] == ((127 << 3) - rmr::kToneBinBias) - 1);
    CHECK(rmr_luminance_bins(nullptr, 0, nullptr) == RMR_OK);
    CHECK(rmr_luminance_bins(nullptr, 1, bins.data()) == RMR_E_INVALID);
    // the lower edge of every bin 1..255 and the float below it: red-only pixels, r searched near
    // L / 0.2126f so that 0.2126f r lands on the wanted L where some r does, next to it otherwise; the
    // bin is compared with the closed form on the L the pixel really has
    for (int b = 1; b < 256; b++) {
        const uint32_t edge = (uint32_t)(b + rmr::kToneBinBias) << 20;
        const float lo = from_bits(edge), below = from_bits(edge - 1);
        for (float target : {lo, below}) {
            float r = target / 0.2126f;
            for (int it = 0; it < 8 && 0.2126f * r < target; it++) r = std::nextafter(r, kInf);
            for (int it = 0; it < 8 && 0.2126f * r > target; it++) r = std::nextafter(r, 0.0f);
            const float L = (0.2126f * r + 0.7152f * 0.0f) + 0.0722f * 0.0f;
            const float one[4] = {r, 0.0f, 0.0f, 1.0f};
            int32_t got = -7;
            CHECK(rmr_luminance_bins(one, 1, &got) == RMR_OK);
            uint32_t u;
            std::memcpy(&u, &L, sizeof u);
            int k = (int)(u >> 20) - rmr::kToneBinBias;
            k = k < 0 ? 0 : (k > 255 ? 255 : k);
            CHECK(got == k);
            if (L == lo) CHECK(got == b);
            if (L == below) CHECK(got == b - 1);
        }
    }
}

void check_curves() {
    const size_t n = 4096;
    std::vector<float> in(4 * n), out(4 * n);
    for (size_t i = 0; i < n; i++) {
        const float x = std::exp2(-24.0f + 48.0f * (float)i / (float)(n - 1));
        in[4 * i] = x;
        in[4 * i + 1] = -x;
        in[4 * i + 2] = i == 7 ? kNaN : (i == 9 ? kInf : x);
        in[4 * i + 3] = (float)i;
    }
    for (int curve = RMR_TONE_LINEAR; curve <= RMR_TONE_ACES; curve++) {
        for (float scale : {0.125f, 1.0f, 5.6568542f}) {
            rmr_tonemap_params p;
            rmr_default_tonemap_params(&p);
            p.curve = curve;
            CHECK(rmr_tonemap_pixels(&p, scale, in.data(), n, out.data()) == RMR_OK);
            float prev = 0.0f;
            for (size_t i = 0; i < n; i++) {
                const float v = out[4 * i];
                CHECK(v >= 0.0f && v <= 1.0f && v >= prev);
                prev = v;
                CHECK(out[4 * i + 1] == 0.0f && !std::signbit(out[4 * i + 1]));
                CHECK(out[4 * i + 3] == (float)i);
            }
            CHECK(out[4 * 7 + 2] == 0.0f);   // NaN
            CHECK(out[4 * 9 + 2] == 1.0f);   // +inf
            CHECK(out[4 * (n - 1)] == 1.0f);
        }
    }
    rmr_tonemap_params p;
    rmr_default_tonemap_params(&p);
    p.white = 0.0f;
    CHECK(rmr_tonemap_pixels(&p, 1.0f, in.data(), n, out.data()) == RMR_E_INVALID);
    CHECK(rmr_tonemap_pixels(nullptr, 1.0f, in.data(), 1, out.data()) == RMR_OK);
}

void check_meter() {
    std::vector<uint32_t> h(256, 0u);
    rmr_tonemap_params p;
    rmr_default_tonemap_params(&p);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double l = -1.0;
    // nothing metered: exposure_ev, or the previous l
    p.exposure_ev = 1.5f;
    h[0] = 1000;
    CHECK(rmr_exposure_from_histogram(h.data(), &p, nan, &l) == RMR_OK && l == 1.5);
    CHECK(rmr_exposure_from_histogram(h.data(), &p, -2.25, &l) == RMR_OK && l == -2.25);
    // one bin: l = log2(key) - lc_b + ev
    const int b = (16 << 3) | 3;   // e = 0, m = 3
    h[b] = 77;
    const double lc = std::log2(1.0 + 3.5 / 8.0);
    CHECK(rmr_exposure_from_histogram(h.data(), &p, nan, &l) == RMR_OK);
    CHECK(std::fabs(l - (std::log2((double)0.18f) - lc + 1.5)) < 1e-12);
    // adapt from a previous state
    p.adapt = 0.25f;
    double l2 = 0.0;
    CHECK(rmr_exposure_from_histogram(h.data(), &p, 4.0, &l2) == RMR_OK);
    CHECK(std::fabs(l2 - (4.0 + 0.25 * (l - 4.0))) < 1e-12);
    // two bins, the window cutting both: counts 100 and 300, window [0.1, 0.9) of 400 = [40, 360)
    p.adapt = 1.0f;
    p.exposure_ev = 0.0f;
    std::fill(h.begin(), h.end(), 0u);
    h[b] = 100;
    h[b + 8] = 300;
    CHECK(rmr_exposure_from_histogram(h.data(), &p, nan, &l) == RMR_OK);
    // the float percentages are not 0.1 and 0.9: compare with the rule's own window
    const double lo = (double)0.10f * 400.0, hi = (double)0.90f * 400.0;
    const double w0 = 100.0 - lo, w1 = hi - 100.0;
    const double mean = (w0 * lc + w1 * (1.0 + lc)) / (w0 + w1);
    CHECK(std::fabs(l - (std::log2((double)0.18f) - mean)) < 1e-12);
    CHECK(rmr_exposure_from_histogram(h.data(), &p, std::numeric_limits<double>::infinity(), &l) == RMR_E_INVALID);
    CHECK(rmr_exposure_from_histogram(nullptr, &p, nan, &l) == RMR_E_INVALID);
}
}  // namespace

int main() {
    check_params();
    check_bins();
    check_curves();
    check_meter();
    if (failures) {
        std::printf("tonemap_test: %d failures\n", failures);
        return 1;
    }
    std::printf("tonemap_test ok\n");
    return 0;
}
