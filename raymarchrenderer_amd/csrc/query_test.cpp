// query_test.cpp — stand-alone CPU checks of the ray rule the query kernels share with rmr_check_rays
// (rmr_ray_check.h; no HIP, no Python), run plain and under the address and undefined-behaviour
// sanitizers by tests/test_query_cpu.py: the shared rule against rmr_check_rays on a table of rays, an
// independent statement of the rule, and the origin-extent rule of rmr_trace_rays_device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "rmr_camera.hpp"
#include "rmr_ray_check.h"

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

rmr_ray good_ray() {
    rmr_ray r{};
    r.o[0] = 1.5f; r.o[1] = -2.0f; r.o[2] = 0.25f;
    r.time = 1000.016f;
    r.d[0] = 3.0f / 13.0f; r.d[1] = -4.0f / 13.0f; r.d[2] = 12.0f / 13.0f;
    r.rc = 0.5f;
    r.gx = 7;
    r.gy = 9;
    return r;
}

// the rule as include/rmr.h states it, with the library's own functions
bool stated_rule(const rmr_ray& r) {
    const float f[8] = {r.o[0], r.o[1], r.o[2], r.time, r.d[0], r.d[1], r.d[2], r.rc};
    for (float x : f)
        if (!std::isfinite(x)) return false;
    const double dd = (double)r.d[0] * (double)r.d[0] + (double)r.d[1] * (double)r.d[1] + (double)r.d[2] * (double)r.d[2];
    if (!(std::fabs(dd - 1.0) <= 1e-5)) return false;
    return r.gx >= 0 && r.gy >= 0 && r.gx < 16777216 && r.gy < 16777216;
}

int n_ok = 0, n_bad = 0;
// one ray through the shared rule, the statement, and rmr_check_rays on an exactly sized heap list with
// the ray last (the sanitizers see any read past the list)
void check_ray(const rmr_ray& r, int want) {
    const bool ok = rmr::ray_ok(r);
    CHECK(ok == stated_rule(r));
    if (want >= 0) CHECK(ok == (want != 0));
    (ok ? n_ok : n_bad)++;
    for (size_t n : {(size_t)1, (size_t)5}) {
        std::vector<rmr_ray> list(n, good_ray());
        list[n - 1] = r;
        CHECK((rmr_check_rays(list.data(), n) == RMR_OK) == ok);
        CHECK(rmr::first_bad_ray(list.data(), n) == (ok ? -1 : (long long)(n - 1)));
    }
}

float* field(rmr_ray& r, int k) {
    return k < 3 ? &r.o[k] : k == 3 ? &r.time : k < 7 ? &r.d[k - 4] : &r.rc;
}

void check_rule() {
    check_ray(good_ray(), 1);
    // each float field NaN and +-inf in turn
    for (int k = 0; k < 8; k++)
        for (float v : {kNaN, kInf, -kInf}) {
            rmr_ray r = good_ray();
            *field(r, k) = v;
            check_ray(r, 0);
        }
    // d.d - 1 just inside and just outside +-1e-5: d = (0, 0, s), searched float by float around the bound
    for (double sign : {1.0, -1.0}) {
        float s = (float)std::sqrt(1.0 + sign * 1e-5);
        // walk to the last float inside the bound, from either side
        auto inside = [](float z) { return std::fabs((double)z * (double)z - 1.0) <= 1e-5; };
        const float away = sign > 0 ? 2.0f : 0.0f, towards = 1.0f;
        while (!inside(s)) s = std::nextafter(s, towards);
        while (inside(std::nextafter(s, away))) s = std::nextafter(s, away);
        rmr_ray r = good_ray();
        r.d[0] = r.d[1] = 0.0f;
        r.d[2] = s;
        check_ray(r, 1);
        r.d[2] = std::nextafter(s, away);
        check_ray(r, 0);
        r.d[2] = -s;
        check_ray(r, 1);
        r.d[0] = std::nextafter(s, away);   // the first component: the same sum
        r.d[2] = 0.0f;
        check_ray(r, 0);
    }
    for (float s : {0.0f, 2.0f, 1.01f, 0.99f}) {
        rmr_ray r = good_ray();
        r.d[0] *= s; r.d[1] *= s; r.d[2] *= s;
        check_ray(r, 0);
    }
    // three components near the bound: whatever the verdict, every statement agrees
    for (int k = -40; k <= 40; k++) {
        rmr_ray r = good_ray();
        const float s = 1.0f + (float)k * 2.5e-7f;
        r.d[0] *= s; r.d[1] *= s; r.d[2] *= s;
        check_ray(r, -1);
    }
    // gx / gy at -1, 2^24 - 1 and 2^24
    for (int which = 0; which < 2; which++)
        for (int32_t v : {-1, (1 << 24) - 1, 1 << 24, 0, INT32_MIN, INT32_MAX}) {
            rmr_ray r = good_ray();
            (which ? r.gy : r.gx) = v;
            check_ray(r, v >= 0 && v < (1 << 24));
        }
    CHECK(n_ok >= 10 && n_bad >= 40);
    CHECK(rmr_check_rays(nullptr, 0) == RMR_OK && rmr_check_rays(nullptr, 2) == RMR_E_INVALID);
}

void check_extent() {
    for (float e : {0.0f, 1.0f, 3.5f, 1e30f, std::numeric_limits<float>::denorm_min()}) CHECK(rmr::extent_ok(e));
    CHECK(rmr::extent_ok(-0.0f));
    for (float e : {-1.0f, -1e-30f, kNaN, kInf, -kInf}) CHECK(!rmr::extent_ok(e));
    for (float e : {0.0f, 0.75f, 2.0f, 1e20f}) {
        for (int k = 0; k < 3; k++)
            for (float sg : {1.0f, -1.0f}) {
                rmr_ray r = good_ray();
                r.o[0] = r.o[1] = r.o[2] = 0.0f;
                r.o[k] = sg * e;
                CHECK(rmr::origin_within(r, e));                    // |o_k| == extent is inside
                r.o[k] = sg * std::nextafter(e, kInf);
                CHECK(!rmr::origin_within(r, e));                   // the next float is not
                r.o[k] = kNaN;
                CHECK(!rmr::origin_within(r, e));
                r.o[k] = sg * kInf;
                CHECK(!rmr::origin_within(r, e));
            }
    }
    rmr_ray r = good_ray();   // |o| = (1.5, 2, 0.25)
    CHECK(rmr::origin_within(r, 2.0f) && !rmr::origin_within(r, 1.99f));
}
}  // namespace

int main() {
    check_rule();
    check_extent();
    if (failures) {
        std::printf("query_test: %d checks failed\n", failures);
        return 1;
    }
    std::printf("query_test ok (%d rays accepted, %d rejected)\n", n_ok, n_bad);
    return 0;
}
