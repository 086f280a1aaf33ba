// bloom_test.cpp — stand-alone CPU checks of bloom.cpp (no HIP, no Python), run plain and under the
// address and undefined-behaviour sanitizers by tests/test_bloom_cpu.py: the parameter ranges, the level
// sizes, and rmr_bloom_pixels on exactly sized heap arrays (every level count at sizes down to 1 x 1, the
// copy rule, a constant image, an image below the threshold).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "bloom.hpp"

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

void check_params() {
    static_assert(sizeof(rmr_bloom_params) == 32, "rmr_bloom_params is 32 bytes");
    rmr_bloom_params p;
    rmr_default_bloom_params(&p);
    CHECK(p.levels == 5 && p.threshold == 1.0f && p.clamp == 0.0f && p.scatter == 0.7f && p.intensity == 0.2f);
    CHECK(p.reserved[0] == 0 && p.reserved[1] == 0 && p.reserved[2] == 0);
    CHECK(rmr_check_bloom_params(&p) == RMR_OK);
    CHECK(rmr_check_bloom_params(nullptr) == RMR_E_INVALID);
    rmr_default_bloom_params(nullptr);
    auto good = [&](auto set) {
        rmr_default_bloom_params(&p);
        set(p);
        CHECK(rmr_check_bloom_params(&p) == RMR_OK);
    };
    auto bad = [&](auto set) {
        rmr_default_bloom_params(&p);
        set(p);
        CHECK(rmr_check_bloom_params(&p) == RMR_E_INVALID);
    };
    for (int n : {1, 8}) good([n](rmr_bloom_params& q) { q.levels = n; });
    for (int n : {0, 9, -1}) bad([n](rmr_bloom_params& q) { q.levels = n; });
    for (float v : {0.0f, 1e30f}) good([v](rmr_bloom_params& q) { q.threshold = q.clamp = q.intensity = v; });
    for (float v : {-1e-6f, kNaN, kInf, -kInf}) {
        bad([v](rmr_bloom_params& q) { q.threshold = v; });
        bad([v](rmr_bloom_params& q) { q.clamp = v; });
        bad([v](rmr_bloom_params& q) { q.intensity = v; });
    }
    for (float v : {0.0f, 1.0f}) good([v](rmr_bloom_params& q) { q.scatter = v; });
    for (float v : {-0.01f, 1.01f, kNaN, kInf}) bad([v](rmr_bloom_params& q) { q.scatter = v; });
    for (int k = 0; k < 3; k++) bad([k](rmr_bloom_params& q) { q.reserved[k] = 1; });
}

void check_levels() {
    const rmr::BloomLevels L = rmr::bloom_levels(131, 77, 8);
    const int w[9] = {131, 66, 33, 17, 9, 5, 3, 2, 1}, h[9] = {77, 39, 20, 10, 5, 3, 2, 1, 1};
    size_t at = 0;
    for (int k = 0; k <= 8; k++) {
        CHECK(L.w[k] == w[k] && L.h[k] == h[k]);
        if (k >= 1) {
            CHECK(L.off[k] == at);
            at += (size_t)w[k] * h[k];
        }
    }
    CHECK(L.total == at);
    CHECK(rmr::bloom_levels(1, 1, 3).total == 3);
    CHECK(rmr::bloom_gain(0.5f, 0.0f, 8) == 0.5f && rmr::bloom_gain(0.5f, 1.0f, 4) == 0.125f);
}

bool same_bits(const float* a, const float* b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }

void check_pixels() {
    rmr_bloom_params p;
    rmr_default_bloom_params(&p);
    const int sizes[][2] = {{1, 1}, {2, 3}, {3, 1}, {1, 7}, {13, 9}, {44, 36}};
    uint32_t seed = 12345u;
    auto rnd = [&seed]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)(seed >> 8) * (1.0f / 16777216.0f);
    };
    for (const auto& wh : sizes) {
        const int w = wh[0], h = wh[1];
        const size_t n = (size_t)w * h;
        for (int N = 1; N <= 8; N++) {
            p.levels = N;
            // exactly sized heap arrays: a read or write past either end is the sanitizer's to find
            std::vector<float> in(4 * n), out(4 * n, -1.0f);
            for (size_t i = 0; i < n; i++) {
                for (int k = 0; k < 3; k++) in[4 * i + k] = std::exp2(rnd() * 12.0f - 6.0f);
                in[4 * i + 3] = 1.0f;
            }
            in[0] = kNaN;                       // invalid pixels: copied bit for bit
            if (n > 1) in[4 * (n - 1) + 3] = 0.0f;
            if (n > 2) in[4 * 1 + 1] = -kInf;
            if (n > 3) { in[4 * 2] = -2.0f; in[4 * 2 + 1] = 1e4f; }
            CHECK(rmr_bloom_pixels(&p, in.data(), w, h, out.data()) == RMR_OK);
            CHECK(same_bits(&in[0], &out[0], 4));
            if (n > 1) CHECK(same_bits(&in[4 * (n - 1)], &out[4 * (n - 1)], 4));
            if (n > 2) CHECK(same_bits(&in[4], &out[4], 4));
            for (size_t i = 0; i < n; i++) {
                CHECK(same_bits(&in[4 * i + 3], &out[4 * i + 3], 1));
                const bool valid = in[4 * i + 3] != 0.0f && std::isfinite(in[4 * i]) && std::isfinite(in[4 * i + 1]) &&
                                   std::isfinite(in[4 * i + 2]);
                if (valid)
                    for (int k = 0; k < 3; k++) CHECK(out[4 * i + k] >= in[4 * i + k]);   // the spread part is >= 0
            }
            // nothing above the threshold: the image comes back equal in value
            rmr_bloom_params q = p;
            q.threshold = 1e5f;
            CHECK(rmr_bloom_pixels(&q, in.data(), w, h, out.data()) == RMR_OK);
            for (size_t i = 1; i < 4 * n; i++)
                if (!std::isnan(in[i])) CHECK(out[i] == in[i]);
            // a constant image with T = 0 and one level: c + I c
            if (N == 1) {
                for (size_t i = 0; i < n; i++) {
                    in[4 * i] = 0.5f, in[4 * i + 1] = 2.0f, in[4 * i + 2] = 0.25f, in[4 * i + 3] = 1.0f;
                }
                q = p;
                q.threshold = 0.0f;
                q.intensity = 0.5f;
                CHECK(rmr_bloom_pixels(&q, in.data(), w, h, out.data()) == RMR_OK);
                for (size_t i = 0; i < n; i++)
                    for (int k = 0; k < 3; k++) CHECK(std::fabs(out[4 * i + k] - 1.5f * in[4 * i + k]) <= 1e-6f * in[4 * i + k]);
            }
        }
    }
    std::vector<float> one(4, 1.0f), res(4);
    CHECK(rmr_bloom_pixels(nullptr, one.data(), 1, 1, res.data()) == RMR_OK);
    CHECK(rmr_bloom_pixels(&p, nullptr, 1, 1, res.data()) == RMR_E_INVALID);
    CHECK(rmr_bloom_pixels(&p, one.data(), 1, 1, nullptr) == RMR_E_INVALID);
    CHECK(rmr_bloom_pixels(&p, one.data(), 0, 1, res.data()) == RMR_E_INVALID);
    CHECK(rmr_bloom_pixels(&p, one.data(), 1, -1, res.data()) == RMR_E_INVALID);
    p.levels = 9;
    CHECK(rmr_bloom_pixels(&p, one.data(), 1, 1, res.data()) == RMR_E_INVALID);
}
}  // namespace

int main() {
    check_params();
    check_levels();
    check_pixels();
    if (failures) {
        std::printf("bloom_test: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("bloom_test ok\n");
    return 0;
}
