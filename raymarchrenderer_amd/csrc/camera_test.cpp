// camera_test.cpp — stand-alone CPU checks of camera.cpp (no HIP, no Python), run plain and under the
// address and undefined-behaviour sanitizers by tests/test_camera_cpu.py: the model ranges, the camera
// frame (orthonormal, oriented, degenerate views), and rmr_check_rays on exactly sized heap lists with
// the bad ray first, last and nowhere.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rmr_camera.hpp"

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

void check_models() {
    rmr_camera_model m;
    rmr_default_camera_model(&m);
    CHECK(m.model == RMR_CAMERA_VIEW && rmr_check_camera_model(&m) == RMR_OK);
    CHECK(rmr_check_camera_model(nullptr) == RMR_E_INVALID);
    const float bad[] = {-1.0f, kNaN, kInf, -kInf};
    for (int model = -2; model < 7; model++) {
        rmr_default_camera_model(&m);
        m.model = model;
        CHECK((rmr_check_camera_model(&m) == RMR_OK) == (model >= RMR_CAMERA_VIEW && model <= RMR_CAMERA_ORTHO));
        for (float b : bad) {
            for (int field = 0; field < 4; field++) {
                rmr_default_camera_model(&m);
                m.model = model;
                (field == 0 ? m.aperture : field == 1 ? m.focus : field == 2 ? m.width : m.height) = b;
                const bool own = (model == RMR_CAMERA_THIN_LENS && field < 2) || (model == RMR_CAMERA_ORTHO && field >= 2);
                const bool known = model >= RMR_CAMERA_VIEW && model <= RMR_CAMERA_ORTHO;
                CHECK((rmr_check_camera_model(&m) == RMR_OK) == (known && !own));
            }
        }
    }
    rmr_default_camera_model(&m);
    m.model = RMR_CAMERA_THIN_LENS;
    m.focus = 0.0f;
    CHECK(rmr_check_camera_model(&m) == RMR_E_INVALID);   // focus > 0, aperture >= 0
    m.focus = 1e-30f;
    CHECK(rmr_check_camera_model(&m) == RMR_OK);
    m.model = RMR_CAMERA_ORTHO;
    m.width = 0.0f;
    CHECK(rmr_check_camera_model(&m) == RMR_E_INVALID);
}

double dot(const float* a, const float* b) { return (double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2]; }

void check_frames() {
    float out[9];
    for (int it = 0; it < 200; it++) {
        float view[15];
        for (float& v : view) v = 4.0f * rnd() - 2.0f;
        if (rmr_camera_frame(view, out) != RMR_OK) continue;   // (a random view is almost never degenerate)
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) CHECK(std::fabs(dot(out + 3 * i, out + 3 * j) - (i == j ? 1.0 : 0.0)) < 1e-6);
        float du[3], dv[3], sum[3];
        for (int k = 0; k < 3; k++) {
            du[k] = view[6 + k] - view[3 + k];
            dv[k] = view[9 + k] - view[3 + k];
            sum[k] = view[3 + k] + view[6 + k] + view[9 + k] + view[12 + k];
        }
        CHECK(dot(out, du) > 0 && dot(out + 3, dv) > 0 && dot(out + 6, sum) > 0);
    }
    float view[15] = {0, 0, 0, -1, 1, 2, 1, 1, 2, -1, -1, 2, 1, -1, 2};   // a symmetric frustum along +z, y up
    CHECK(rmr_camera_frame(view, out) == RMR_OK);
    const float want[9] = {1, 0, 0, 0, -1, 0, 0, 0, 1};
    for (int k = 0; k < 9; k++) CHECK(out[k] == want[k]);
    CHECK(rmr_camera_frame(nullptr, out) == RMR_E_INVALID && rmr_camera_frame(view, nullptr) == RMR_E_INVALID);
    float v2[15];
    auto reset = [&] { for (int k = 0; k < 15; k++) v2[k] = view[k]; };
    reset(); v2[7] = kNaN;
    CHECK(rmr_camera_frame(v2, out) == RMR_E_INVALID);
    reset(); v2[0] = kInf;
    CHECK(rmr_camera_frame(v2, out) == RMR_E_INVALID);
    reset(); for (int k = 0; k < 3; k++) v2[6 + k] = v2[3 + k];                       // U vanishes
    CHECK(rmr_camera_frame(v2, out) == RMR_E_INVALID);
    reset(); for (int k = 0; k < 3; k++) v2[9 + k] = v2[3 + k] + 3.0f * (v2[6 + k] - v2[3 + k]);   // V parallel to U
    CHECK(rmr_camera_frame(v2, out) == RMR_E_INVALID);
    reset(); v2[5] = v2[8] = v2[11] = v2[14] = 0.0f;                                   // the corners' sum vanishes
    CHECK(rmr_camera_frame(v2, out) == RMR_E_INVALID);
}

void check_rays() {
    CHECK(rmr_check_rays(nullptr, 0) == RMR_OK && rmr_check_rays(nullptr, 1) == RMR_E_INVALID);
    for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1000}) {
        std::vector<rmr_ray> r(n);   // exactly n: a read past the end is the sanitizer's to find
        for (rmr_ray& y : r) {
            float d[3] = {rnd() - 0.5f, rnd() - 0.5f, rnd() - 0.5f + 1e-3f};
            const float l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            for (int k = 0; k < 3; k++) {
                y.d[k] = d[k] / l;
                y.o[k] = 100.0f * rnd() - 50.0f;
            }
            y.time = 1000.0f * rnd();
            y.rc = rnd();
            y.gx = (int32_t)(rnd() * 16777215.0f);
            y.gy = (int32_t)(rnd() * 16777215.0f);
        }
        CHECK(rmr_check_rays(r.data(), n) == RMR_OK && rmr::first_bad_ray(r.data(), n) == -1);
        for (size_t at : {(size_t)0, n / 2, n - 1}) {
            for (int what = 0; what < 7; what++) {
                std::vector<rmr_ray> b(r);
                rmr_ray& y = b[at];
                if (what == 0) y.o[1] = kNaN;
                if (what == 1) y.d[2] = kInf;
                if (what == 2) y.time = kNaN;
                if (what == 3) y.rc = -kInf;
                if (what == 4) y.gx = -1;
                if (what == 5) y.gy = 1 << 24;
                if (what == 6) { y.d[0] *= 1.001f; y.d[1] *= 1.001f; y.d[2] *= 1.001f; }   // d.d = 1.002
                CHECK(rmr_check_rays(b.data(), n) == RMR_E_INVALID && rmr::first_bad_ray(b.data(), n) == (long long)at);
            }
        }
    }
    // the bound itself: |d.d - 1| <= 1e-5 in double
    rmr_ray y{};
    y.d[2] = 1.0f + 4e-6f;
    CHECK(rmr_check_rays(&y, 1) == RMR_OK);
    y.d[2] = 1.0f + 6e-6f;
    CHECK(rmr_check_rays(&y, 1) == RMR_E_INVALID);
    y.d[2] = -(1.0f - 4e-6f);
    CHECK(rmr_check_rays(&y, 1) == RMR_OK);
    y.d[2] = 0.0f;
    CHECK(rmr_check_rays(&y, 1) == RMR_E_INVALID);
    // the origin extent the escape boxes' inflation takes
    const float eye[3] = {1.0f, -7.0f, 2.0f};
    rmr_camera_model m;
    rmr_default_camera_model(&m);
    CHECK(rmr::camera_origin_extent(m, eye) == 7.0);
    m.model = RMR_CAMERA_THIN_LENS;
    m.aperture = 0.5f;
    CHECK(rmr::camera_origin_extent(m, eye) >= 7.0 + 0.5 * std::sqrt(2.0));
    m.model = RMR_CAMERA_ORTHO;
    m.width = 4.0f;
    m.height = 2.0f;
    CHECK(rmr::camera_origin_extent(m, eye) >= 7.0 + 3.0);
}
}  // namespace

int main() {
    check_models();
    check_frames();
    check_rays();
    if (failures) {
        std::printf("camera_test: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("camera_test ok\n");
    return 0;
}
