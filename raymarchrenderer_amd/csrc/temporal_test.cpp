// temporal_test.cpp — stand-alone CPU checks of temporal.cpp (no HIP, no Python), run plain and under
// the address and undefined-behaviour sanitizers by tests/test_temporal_cpu.py: the parameter ranges,
// and the view inverse on exactly sized heap arrays (random views with and without a twist multiply
// back to the identity; degenerate views are refused).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "temporal.hpp"

namespace {
int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

uint32_t rng_state = 2463534242u;
float rnd() {   // xorshift, [0, 1)
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

void check_params() {
    rmr_temporal_params p;
    rmr_default_temporal_params(&p);
    CHECK(p.max_history == 64.0f && p.sigma_z == 0.02f && p.normal_pow2 == 5);
    CHECK(rmr_check_temporal_params(&p) == RMR_OK);
    CHECK(rmr_check_temporal_params(nullptr) == RMR_E_INVALID);
    rmr_default_temporal_params(nullptr);
    for (float b : {0.0f, 0.5f, -1.0f, kNaN, kInf, -kInf}) {
        rmr_default_temporal_params(&p);
        p.max_history = b;
        CHECK(rmr_check_temporal_params(&p) == RMR_E_INVALID);
    }
    for (float b : {0.0f, -1.0f, kNaN, kInf}) {
        rmr_default_temporal_params(&p);
        p.sigma_z = b;
        CHECK(rmr_check_temporal_params(&p) == RMR_E_INVALID);
    }
    for (int k = -2; k < 10; k++) {
        rmr_default_temporal_params(&p);
        p.normal_pow2 = k;
        CHECK((rmr_check_temporal_params(&p) == RMR_OK) == (k >= 0 && k <= 7));
    }
    rmr_default_temporal_params(&p);
    p.max_history = 1.0f;
    p.sigma_z = 1e-30f;
    CHECK(rmr_check_temporal_params(&p) == RMR_OK);
}

// a pinhole-like view: corner rays about +z, optionally with r11 scaled (a twist)
void make_view(std::vector<float>& v, float twist) {
    v.assign(15, 0.0f);
    for (int i = 0; i < 3; i++) v[i] = rnd() * 4.0f - 2.0f;
    const float hx = 0.3f + rnd(), hy = 0.3f + rnd();
    const float c[4][2] = {{-hx, -hy}, {hx, -hy}, {-hx, hy}, {hx, hy}};
    for (int k = 0; k < 4; k++) {
        v[3 + 3 * k] = c[k][0];
        v[4 + 3 * k] = c[k][1];
        v[5 + 3 * k] = 1.0f;
    }
    for (int i = 0; i < 3; i++) v[12 + i] *= 1.0f + twist;
}

void check_inverse() {
    for (int trial = 0; trial < 200; trial++) {
        std::vector<float> v;
        make_view(v, trial & 1 ? 0.05f : 0.0f);
        std::vector<double> o(12, 0.0);
        CHECK(rmr_temporal_view_inverse(v.data(), o.data()) == RMR_OK);
        double col[3][3], c[3];
        for (int i = 0; i < 3; i++) {
            col[0][i] = (double)v[6 + i] - (double)v[3 + i];
            col[1][i] = (double)v[9 + i] - (double)v[3 + i];
            col[2][i] = (double)v[3 + i];
            c[i] = ((double)v[12 + i] - (double)v[9 + i]) - col[0][i];
        }
        for (int r = 0; r < 3; r++) {
            for (int k = 0; k < 3; k++) {
                double s = 0.0;
                for (int i = 0; i < 3; i++) s += o[3 * r + i] * col[k][i];
                CHECK(std::fabs(s - (r == k ? 1.0 : 0.0)) < 1e-12);
            }
            double s = 0.0;
            for (int i = 0; i < 3; i++) s += o[3 * r + i] * c[i];
            CHECK(std::fabs(s - o[9 + r]) < 1e-12);
        }
        if (!(trial & 1)) CHECK(std::fabs(o[9]) + std::fabs(o[10]) + std::fabs(o[11]) < 1e-6);
    }
    std::vector<float> v;
    std::vector<double> o(12, 0.0);
    CHECK(rmr_temporal_view_inverse(nullptr, o.data()) == RMR_E_INVALID);
    make_view(v, 0.0f);
    CHECK(rmr_temporal_view_inverse(v.data(), nullptr) == RMR_E_INVALID);
    for (int k = 0; k < 4; k++) {   // a zero corner ray
        make_view(v, 0.0f);
        for (int i = 0; i < 3; i++) v[3 + 3 * k + i] = 0.0f;
        CHECK(rmr_temporal_view_inverse(v.data(), o.data()) == RMR_E_INVALID);
    }
    make_view(v, 0.0f);   // corners coplanar with the origin
    for (int k = 0; k < 4; k++) v[5 + 3 * k] = 0.0f;
    CHECK(rmr_temporal_view_inverse(v.data(), o.data()) == RMR_E_INVALID);
    for (float b : {kNaN, kInf}) {
        for (int i = 0; i < 15; i++) {
            make_view(v, 0.0f);
            v[i] = b;
            CHECK(rmr_temporal_view_inverse(v.data(), o.data()) == RMR_E_INVALID);
        }
    }
}
}  // namespace

int main() {
    check_params();
    check_inverse();
    if (failures) {
        std::printf("temporal_test: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("temporal_test ok\n");
    return 0;
}
