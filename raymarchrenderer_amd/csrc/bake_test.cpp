// bake_test.cpp — stand-alone CPU check of the light bake's host functions (bake.cpp, rmr_bake_rule.h): the
// parameter ranges, the reject rule at its bound, the fold's edge cases, the sRGB bytes against the thresholds
// and the coloured PLY's bytes. tests/test_bake_cpu.py builds and runs it, plain and under the sanitizers.
//   bake_test DIR           the checks (DIR: where the PLY is written)
//   bake_test fold IN OUT   rmr_bake_fold of a file: uint32 n, nspp, then L [nspp][n][3], c [nspp][n], cv [nspp][n];
//                           OUT: rgba [n][4], ao [n]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "rmr_bake_rule.h"

namespace {
int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            failures++;                                                          \
        }                                                                        \
    } while (0)

const float kInf = std::numeric_limits<float>::infinity();
const float kNaN = std::numeric_limits<float>::quiet_NaN();

void check_params() {
    rmr_bake_params p;
    std::memset(&p, 0xff, sizeof p);
    rmr_default_bake_params(&p);
    CHECK(p.flags == RMR_BAKE_RADIANCE && p.bias == 0.002f && p.ao_distance == kInf && p.origin_extent == 0.0f && p.first_index == 0);
    CHECK(sizeof(rmr_bake_params) == 24);
    CHECK(rmr_check_bake_params(&p) == RMR_OK);
    CHECK(rmr_check_bake_params(nullptr) == RMR_E_INVALID);
    rmr_bake_params q = p;
    q.flags = 0;
    CHECK(rmr_check_bake_params(&q) == RMR_E_INVALID);
    q.flags = 4;
    CHECK(rmr_check_bake_params(&q) == RMR_E_INVALID);
    q.flags = RMR_BAKE_RADIANCE | RMR_BAKE_AO;
    CHECK(rmr_check_bake_params(&q) == RMR_OK);
    for (float bias : {kNaN, kInf, -kInf}) {
        q = p;
        q.bias = bias;
        CHECK(rmr_check_bake_params(&q) == RMR_E_INVALID);
    }
    q = p;
    q.bias = -0.01f;   // a bias into the surface is the caller's business
    CHECK(rmr_check_bake_params(&q) == RMR_OK);
    for (float d : {kNaN, 0.0f, -1.0f, -kInf}) {
        q = p;
        q.ao_distance = d;
        CHECK(rmr_check_bake_params(&q) == RMR_E_INVALID);
    }
    q = p;
    q.ao_distance = 0.5f;
    CHECK(rmr_check_bake_params(&q) == RMR_OK);
    q.first_index = (uint64_t)1 << 36;
    CHECK(rmr_check_bake_params(&q) == RMR_OK);   // (an empty list may start there)
    q.first_index = ((uint64_t)1 << 36) + 1;
    CHECK(rmr_check_bake_params(&q) == RMR_E_INVALID);
    CHECK(rmr::bake_gx(4095) == 4095 && rmr::bake_gy(4095) == 0 && rmr::bake_gx(4096) == 0 && rmr::bake_gy(4096) == 1);
    CHECK(rmr::bake_gy(((uint64_t)1 << 36) - 1) == (1 << 24) - 1);
}

void check_points() {
    const float s = 1.000001f, t = 0.999999f;   // n.n - 1 = +2e-6 and -2e-6
    const float p[8][3] = {{0, 0, 0}, {1, 2, 3}, {kNaN, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, kInf, 0}, {0, 0, 0}, {0, 0, 0}};
    const float n[8][3] = {{0, 1, 0}, {0.6f, 0.0f, 0.8f}, {0, 1, 0}, {0, 0, 0}, {s, 0, 0}, {0, 1, 0}, {0, kNaN, 0}, {0, 0, t}};
    const bool want[8] = {true, true, false, false, false, false, false, false};
    for (int i = 0; i < 8; i++) {
        size_t bad = 99;
        const int rc = rmr_bake_check_points(p[i], n[i], 1, &bad);
        CHECK((rc == RMR_OK) == want[i]);
        CHECK(bad == (want[i] ? 1u : 0u));
    }
    size_t bad = 99;
    CHECK(rmr_bake_check_points(&p[0][0], &n[0][0], 8, &bad) == RMR_E_INVALID && bad == 2);
    CHECK(rmr_bake_check_points(&p[0][0], &n[0][0], 2, nullptr) == RMR_OK);
    CHECK(rmr_bake_check_points(nullptr, nullptr, 0, &bad) == RMR_OK && bad == 0);
    CHECK(rmr_bake_check_points(nullptr, &n[0][0], 1, &bad) == RMR_E_INVALID);
    // within the bound: 1 + 4e-7
    const float near1[3] = {0.0f, 1.0000002f, 0.0f};
    CHECK(rmr_bake_check_points(p[0], near1, 1, nullptr) == RMR_OK);
    // the degenerate frame and the cosine
    const float up[3] = {0, 1, 0}, down[3] = {-0.0f, -1, 0}, side[3] = {1, 0, 0};
    CHECK(rmr::bake_degenerate(up) && rmr::bake_degenerate(down) && !rmr::bake_degenerate(side));
    const float d[3] = {0.5f, -0.5f, 0.25f};
    CHECK(rmr::bake_cosine(side, d) == 0.5f && rmr::bake_cosine(up, d) == 0.0f && rmr::bake_cosine(down, d) == 0.5f);
    float o[3];
    rmr::bake_origin(p[1], n[1], 0.5f, o);
    CHECK(o[0] == std::fmaf(0.6f, 0.5f, 1.0f) && o[1] == 2.0f && o[2] == std::fmaf(0.8f, 0.5f, 3.0f));
}

void check_fold() {
    // two points, three samples, [k][i]: point 0 has a NaN and an inf sample, point 1 has c = 0 throughout
    const float L[3][2][3] = {{{1, 2, 3}, {1, 1, 1}}, {{kNaN, 1, 1}, {2, 2, 2}}, {{0.5f, kInf, 0}, {3, 3, 3}}};
    const float c[3][2] = {{0.5f, 0}, {1, 0}, {1, 0}};
    const float cv[3][2] = {{0.5f, 0}, {0, 0}, {1, 0}};
    float rgba[2][4], ao[2];
    CHECK(rmr_bake_fold(&L[0][0][0], &c[0][0], &cv[0][0], 2, 3, &rgba[0][0], ao) == RMR_OK);
    CHECK(rgba[0][0] == 1.0f && rgba[0][1] == 2.0f && rgba[0][2] == 3.0f && rgba[0][3] == 1.0f);   // 2 (L 0.5) / 1
    CHECK(rgba[1][0] == 0.0f && rgba[1][3] == 3.0f);
    CHECK(ao[0] == 1.5f / 2.5f && ao[1] == 1.0f);
    // every sample skipped: rgb 0, alpha 0
    const float Lbad[2][1][3] = {{{kNaN, 0, 0}}, {{0, -kInf, 0}}};
    const float c1[2][1] = {{1}, {1}};
    float one[4];
    CHECK(rmr_bake_fold(&Lbad[0][0][0], &c1[0][0], nullptr, 1, 2, one, nullptr) == RMR_OK);
    CHECK(one[0] == 0.0f && one[1] == 0.0f && one[2] == 0.0f && one[3] == 0.0f);
    float a1;
    CHECK(rmr_bake_fold(nullptr, &c1[0][0], &c1[0][0], 1, 2, nullptr, &a1) == RMR_OK && a1 == 1.0f);
    CHECK(rmr_bake_fold(&Lbad[0][0][0], &c1[0][0], nullptr, 1, 0, one, nullptr) == RMR_E_INVALID);
    CHECK(rmr_bake_fold(nullptr, &c1[0][0], nullptr, 1, 2, one, nullptr) == RMR_E_INVALID);
    CHECK(rmr_bake_fold(nullptr, &c1[0][0], nullptr, 1, 2, nullptr, &a1) == RMR_E_INVALID);
    // the sum is sequential float32: 2^24 + 1 + 1 stays 2^24
    const float Lb[3][1][3] = {{{16777216.0f, 0, 0}}, {{1, 0, 0}}, {{1, 0, 0}}};
    const float cb[3][1] = {{1}, {1}, {1}};
    CHECK(rmr_bake_fold(&Lb[0][0][0], &cb[0][0], nullptr, 1, 3, one, nullptr) == RMR_OK);
    CHECK(one[0] == 33554432.0f / 3.0f && one[3] == 3.0f);
}

void check_srgb() {
    float thr[256];
    CHECK(rmr_srgb_thresholds(thr) == RMR_OK);
    std::vector<float> in;
    std::vector<int> want;
    for (int k = 1; k < 256; k++) {
        in.push_back(thr[k]);
        want.push_back(k);
        in.push_back(std::nextafter(thr[k], 0.0f));
        want.push_back(k - 1);
    }
    for (float v : {0.0f, -0.0f, -1.0f, kNaN, -kInf}) { in.push_back(v); want.push_back(0); }
    for (float v : {1.0f, 2.0f, kInf}) { in.push_back(v); want.push_back(255); }
    while (in.size() % 3) { in.push_back(0.5f); want.push_back(188); }
    std::vector<uint8_t> out(in.size());
    CHECK(rmr_srgb8_pixels(in.data(), in.size() / 3, out.data()) == RMR_OK);
    for (size_t i = 0; i < in.size(); i++) CHECK((int)out[i] == want[i]);
    CHECK(rmr_srgb8_pixels(nullptr, 1, out.data()) == RMR_E_INVALID);
    CHECK(rmr_srgb8_pixels(nullptr, 0, nullptr) == RMR_OK);
}

std::string slurp(const std::string& path) {
    std::string s;
    if (std::FILE* f = std::fopen(path.c_str(), "rb")) {
        char buf[4096];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
        std::fclose(f);
    }
    return s;
}

void check_ply(const std::string& dir) {
    const float v[4][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}};
    const float n[4][3] = {{0, 0, 1}, {0, 0, 1}, {0, 0, 1}, {0, 0, 1}};
    const float ids[4] = {0, 1, 2, 3};
    const uint8_t rgb[4][3] = {{1, 2, 3}, {4, 5, 6}, {7, 8, 9}, {250, 251, 252}};
    const uint32_t q[4] = {0, 1, 2, 3};
    const std::string path = dir + "/bake_test.ply";
    CHECK(rmr_encode_ply_colors(path.c_str(), &v[0][0], &n[0][0], ids, &rgb[0][0], 4, q, 1) == RMR_OK);
    const std::string s = slurp(path);
    const std::string head =
        "ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
        "property float nx\nproperty float ny\nproperty float nz\nproperty float material\nproperty uchar red\n"
        "property uchar green\nproperty uchar blue\nelement face 1\nproperty list uchar uint vertex_indices\nend_header\n";
    CHECK(s.size() == head.size() + 4 * 31 + 17 && s.compare(0, head.size(), head) == 0);
    if (s.size() == head.size() + 4 * 31 + 17) {
        const char* b = s.data() + head.size();
        for (int i = 0; i < 4; i++) {
            CHECK(std::memcmp(b + 31 * i, v[i], 12) == 0 && std::memcmp(b + 31 * i + 12, n[i], 12) == 0);
            CHECK(std::memcmp(b + 31 * i + 24, ids + i, 4) == 0 && std::memcmp(b + 31 * i + 28, rgb[i], 3) == 0);
        }
        CHECK(b[124] == 4 && std::memcmp(b + 125, q, 16) == 0);
    }
    // without normals and ids: 15 bytes per vertex; without colours: rmr_encode_ply's file
    CHECK(rmr_encode_ply_colors(path.c_str(), &v[0][0], nullptr, nullptr, &rgb[0][0], 4, q, 1) == RMR_OK);
    CHECK(slurp(path).find("property float z\nproperty uchar red\n") != std::string::npos);
    CHECK(rmr_encode_ply_colors(path.c_str(), &v[0][0], &n[0][0], ids, nullptr, 4, q, 1) == RMR_OK);
    const std::string plain = slurp(path);
    CHECK(rmr_encode_ply(path.c_str(), &v[0][0], &n[0][0], ids, 4, q, 1) == RMR_OK && slurp(path) == plain);
    CHECK(plain.find("red") == std::string::npos);
    const uint32_t bad[4] = {0, 1, 2, 4};
    CHECK(rmr_encode_ply_colors(path.c_str(), &v[0][0], nullptr, nullptr, &rgb[0][0], 4, bad, 1) == RMR_E_INVALID);
    CHECK(rmr_encode_ply_colors((dir + "/no/such/dir.ply").c_str(), &v[0][0], nullptr, nullptr, &rgb[0][0], 4, q, 1) == RMR_E_IO);
    CHECK(rmr_encode_ply_colors(nullptr, &v[0][0], nullptr, nullptr, &rgb[0][0], 4, q, 1) == RMR_E_INVALID);
}

int run_fold(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    uint32_t hdr[2];
    if (std::fread(hdr, 4, 2, f) != 2) { std::fclose(f); return 2; }
    const size_t n = hdr[0], k = hdr[1];
    std::vector<float> L(3 * n * k), c(n * k), cv(n * k), rgba(4 * n), ao(n);
    const bool ok = std::fread(L.data(), 4, L.size(), f) == L.size() && std::fread(c.data(), 4, c.size(), f) == c.size() &&
                    std::fread(cv.data(), 4, cv.size(), f) == cv.size();
    std::fclose(f);
    if (!ok) return 2;
    if (rmr_bake_fold(L.data(), c.data(), cv.data(), n, (uint32_t)k, rgba.data(), ao.data()) != RMR_OK) return 3;
    f = std::fopen(out, "wb");
    if (!f) return 2;
    std::fwrite(rgba.data(), 4, rgba.size(), f);
    std::fwrite(ao.data(), 4, ao.size(), f);
    std::fclose(f);
    std::printf("bake_test fold ok\n");
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "fold") return run_fold(argv[2], argv[3]);
    if (argc != 2) {
        std::printf("usage: bake_test DIR | bake_test fold IN OUT\n");
        return 2;
    }
    check_params();
    check_points();
    check_fold();
    check_srgb();
    check_ply(argv[1]);
    if (failures) {
        std::printf("bake_test: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("bake_test ok\n");
    return 0;
}
