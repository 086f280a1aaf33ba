// probe_vis_test.cpp — stand-alone CPU check of the probes' visibility host functions (probe_vis.cpp,
// rmr_probe_vis_rule.h): the texel directions and the encode, the fold's edge cases, the lookup's weights and the
// parameter ranges. tests/test_probe_vis_cpu.py builds and runs it, plain and under the sanitizers.
//   probe_vis_test                  the checks
//   probe_vis_test texel IN OUT     the texel of directions: uint32 n, then dirs [n][3]; OUT: int32 [n]
//   probe_vis_test fold IN OUT      rmr_probe_vis_fold of a file: uint32 n, nspp, float range, then d_and_t
//                                   [nspp][n][4]; OUT: vis [n][128]
//   probe_vis_test fold2 IN OUT     the same through the rule's functions in two runs of k, the sums carried
//                                   between them as the kernels carry them
//   probe_vis_test lookup IN OUT    rmr_probe_irradiance_vis_host of a file: rmr_volume_desc, uint32 n, float bias,
//                                   then sh [points][28], vis [points][128], points [n][3], normals [n][3]; OUT:
//                                   rgba [n][4], then uint32 first_bad
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "rmr_probe_vis_rule.h"

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

void check_dirs() {
    float D[64][3];
    CHECK(rmr_probe_vis_dirs(D) == RMR_OK && rmr_probe_vis_dirs(nullptr) == RMR_E_INVALID);
    for (int j = 0; j < 64; j++) {
        const double len = std::sqrt((double)D[j][0] * D[j][0] + (double)D[j][1] * D[j][1] + (double)D[j][2] * D[j][2]);
        CHECK(std::fabs(len - 1.0) <= 2.0 * 0x1p-23);
        CHECK(rmr::vis_texel_of(D[j][0], D[j][1], D[j][2]) == j);
    }
    // the poles are +-z: the four centre texels look up, the four corner texels look down
    for (int j : {27, 28, 35, 36}) CHECK(D[j][2] > 0.97f);
    for (int j : {0, 7, 56, 63}) CHECK(D[j][2] < -0.97f);
    // the axes, -0 and NaN
    CHECK(rmr::vis_texel_of(0.0f, 0.0f, 1.0f) == 4 * 8 + 4);      // (o = 0 lies on the border of texels 3 and 4: floor)
    CHECK(rmr::vis_texel_of(1.0f, 0.0f, 0.0f) == 4 * 8 + 7);      // (clamped: ((1 * 0.5) + 0.5) * 8 = 8)
    CHECK(rmr::vis_texel_of(-1.0f, 0.0f, 0.0f) == 4 * 8 + 0);
    CHECK(rmr::vis_texel_of(0.0f, 1.0f, 0.0f) == 7 * 8 + 4);
    CHECK(rmr::vis_texel_of(0.0f, -1.0f, 0.0f) == 0 * 8 + 4);
    CHECK(rmr::vis_texel_of(0.0f, 0.0f, -1.0f) == 7 * 8 + 7);     // (sgn(0) = 1 on both axes)
    CHECK(rmr::vis_texel_of(1.0f, 0.0f, -0.0f) == 4 * 8 + 7);     // (-0 < 0 is false: the upper half)
    CHECK(rmr::vis_texel_of(0.0f, 0.0f, 0.0f) == 0);              // (0 / 0: NaN on both axes)
    CHECK(rmr::vis_texel_of(kNaN, 0.0f, 1.0f) == 0);
}

void check_fold() {
    // one probe, the +z texels: a sample along +z at distance 2 and one along -z at distance 7 (clamped to 4)
    const float range = 4.0f;
    float s[4][4] = {{0, 0, 1, 2.0f}, {0, 0, -1, 7.0f}, {0, 0, 1, kNaN}, {0, 0, 1, kInf}};
    float out[128];
    CHECK(rmr_probe_vis_fold(&s[0][0], 1, 4, range, out) == RMR_OK);
    for (int j : {27, 28, 35, 36}) CHECK(out[2 * j] == 2.0f && out[2 * j + 1] == 4.0f);
    for (int j : {0, 7, 56, 63}) CHECK(out[2 * j] == 4.0f && out[2 * j + 1] == 16.0f);
    // a probe with no finite sample: every texel sees to the range
    CHECK(rmr_probe_vis_fold(&s[2][0], 1, 2, range, out) == RMR_OK);
    for (int j = 0; j < 64; j++) CHECK(out[2 * j] == range && out[2 * j + 1] == range * range);
    // one sample: the texels of the other hemisphere see to the range
    CHECK(rmr_probe_vis_fold(&s[0][0], 1, 1, range, out) == RMR_OK);
    for (int j : {0, 7, 56, 63}) CHECK(out[2 * j] == range);
    for (float bad : {0.0f, -1.0f, kNaN, kInf}) CHECK(rmr_probe_vis_fold(&s[0][0], 1, 4, bad, out) == RMR_E_INVALID);
    CHECK(rmr_probe_vis_fold(&s[0][0], 1, 0, range, out) == RMR_E_INVALID);
    CHECK(rmr_probe_vis_fold(&s[0][0], 1, (1u << 24) + 1, range, out) == RMR_E_INVALID);
    CHECK(rmr_probe_vis_fold(nullptr, 1, 4, range, out) == RMR_E_INVALID);
    CHECK(rmr_probe_vis_fold(nullptr, 0, 4, range, nullptr) == RMR_OK);
    // c^32 by five squarings
    rmr::VisAcc a{0.0f, 0.0f, 0.0f};
    const float D[3] = {0.0f, 0.0f, 1.0f};
    rmr::vis_fold_one(a, D, 0.0f, 0.0f, 0.5f, 3.0f);
    CHECK(a.A == 0x1p-32f && a.M1 == 3.0f * 0x1p-32f && a.M2 == 9.0f * 0x1p-32f);
    rmr::vis_fold_one(a, D, 0.0f, 0.0f, -0.5f, 3.0f);
    rmr::vis_fold_one(a, D, 1.0f, 0.0f, 0.0f, 3.0f);
    rmr::vis_fold_one(a, D, kNaN, 0.0f, 0.0f, 3.0f);
    CHECK(a.A == 0x1p-32f);
}

void check_lookup() {
    // a 2 x 2 x 2 field under a constant radiance 1 (sh0 = 1 / Y0), maps that see to the range
    rmr_volume_desc d{{0.0f, 0.0f, 0.0f}, 1.0f, {2, 2, 2}};
    std::vector<float> sh(8 * 28, 0.0f), vis(8 * 128);
    for (int k = 0; k < 8; k++) {
        for (int c = 0; c < 3; c++) sh[28 * k + c] = 1.0f;
        sh[28 * k + 27] = 4.0f;
    }
    for (size_t i = 0; i < vis.size(); i += 2) { vis[i] = 3.0f; vis[i + 1] = 9.0f; }
    const float q[3][3] = {{0.5f, 0.5f, 0.5f}, {0.0f, 0.0f, 0.0f}, {kNaN, 0.0f, 0.0f}};
    const float nr[3][3] = {{0, 1, 0}, {0, 0, 1}, {0, 1, 0}};
    float out[3][4];
    size_t bad = 99;
    CHECK(rmr_probe_irradiance_vis_host(&d, sh.data(), vis.data(), &q[0][0], &nr[0][0], 2, 0.0f, &out[0][0], &bad) == RMR_OK && bad == 2);
    // on a lattice point: that probe alone, r == 0, both weights 1
    CHECK(out[1][3] == 1.0f && out[1][0] == 0.282095f);
    // mid-cell, normal along y: the four corners above (the normal faces them) weigh (h * h) + 0.2 with b = 0.5 / r,
    // the four below with b = -0.5 / r
    const float r = std::sqrt((0.25f + 0.25f) + 0.25f);
    const float bu = 0.5f / r, bd = -0.5f / r;
    const float hu = (bu + 1.0f) * 0.5f, hd = (bd + 1.0f) * 0.5f;
    const float wu = (hu * hu) + 0.2f, wd = (hd * hd) + 0.2f;
    float W = 0.0f;
    for (int k = 0; k < 8; k++) W = W + (0.125f * (((k >> 1) & 1) ? wu : wd)) * 1.0f;
    CHECK(out[0][3] == W && wu > wd);
    CHECK(std::fabs(out[0][0] - 0.282095f) <= 1e-6f);
    CHECK(rmr_probe_irradiance_vis_host(&d, sh.data(), vis.data(), &q[0][0], &nr[0][0], 3, 0.0f, &out[0][0], &bad) == RMR_E_INVALID && bad == 2);
    for (int c = 0; c < 4; c++) CHECK(out[2][c] == 0.0f);
    // occluded from every probe: the floor keeps the weights from vanishing
    for (size_t i = 0; i < vis.size(); i += 2) { vis[i] = 0.125f; vis[i + 1] = 0.125f * 0.125f; }
    CHECK(rmr_probe_irradiance_vis_host(&d, sh.data(), vis.data(), &q[0][0], &nr[0][0], 1, 0.0f, &out[0][0], nullptr) == RMR_OK);
    CHECK(std::fabs(out[0][3] - W * 0.05f) <= 1e-8f);
    CHECK(std::fabs(out[0][0] - 0.282095f) <= 1e-6f);
    for (float b : {-0.001f, kNaN, kInf})
        CHECK(rmr_probe_irradiance_vis_host(&d, sh.data(), vis.data(), &q[0][0], &nr[0][0], 1, b, &out[0][0], nullptr) == RMR_E_INVALID);
    CHECK(rmr_probe_irradiance_vis_host(&d, sh.data(), nullptr, &q[0][0], &nr[0][0], 1, 0.0f, &out[0][0], nullptr) == RMR_E_INVALID);
    CHECK(rmr_probe_irradiance_vis_host(nullptr, sh.data(), vis.data(), &q[0][0], &nr[0][0], 1, 0.0f, &out[0][0], nullptr) == RMR_E_INVALID);
    d.n[2] = 1;
    CHECK(rmr_probe_irradiance_vis_host(&d, sh.data(), vis.data(), &q[0][0], &nr[0][0], 1, 0.0f, &out[0][0], nullptr) == RMR_E_INVALID);
    CHECK(rmr::vis_range_ok(1e-30f) && !rmr::vis_range_ok(0.0f) && !rmr::vis_range_ok(kNaN) && !rmr::vis_range_ok(kInf));
    CHECK(rmr::vis_bias_ok(0.0f) && !rmr::vis_bias_ok(-0.0f - 1e-30f) && !rmr::vis_bias_ok(kNaN));
}

bool read_all(const char* path, std::vector<unsigned char>& b) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    b.resize(n > 0 ? (size_t)n : 0);
    const bool ok = b.empty() || std::fread(b.data(), 1, b.size(), f) == b.size();
    std::fclose(f);
    return ok;
}
bool write_all(const char* path, const void* p, size_t bytes, const void* q = nullptr, size_t qbytes = 0) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    bool ok = bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes;
    ok = ok && (qbytes == 0 || std::fwrite(q, 1, qbytes, f) == qbytes);
    return std::fclose(f) == 0 && ok;
}

int file_texel(const char* in, const char* out) {
    std::vector<unsigned char> b;
    if (!read_all(in, b) || b.size() < 4) return 2;
    uint32_t n;
    std::memcpy(&n, b.data(), 4);
    if (b.size() != 4 + (size_t)n * 3 * sizeof(float)) return 2;
    std::vector<float> d((size_t)n * 3);
    std::memcpy(d.data(), b.data() + 4, d.size() * sizeof(float));
    std::vector<int32_t> o(n);
    for (uint32_t i = 0; i < n; i++) o[i] = rmr::vis_texel_of(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    if (!write_all(out, o.data(), o.size() * sizeof(int32_t))) return 4;
    std::printf("probe_vis_test texel ok\n");
    return 0;
}

int file_fold(const char* in, const char* out, bool halves) {
    std::vector<unsigned char> b;
    if (!read_all(in, b) || b.size() < 12) return 2;
    uint32_t hd[2];
    float range;
    std::memcpy(hd, b.data(), 8);
    std::memcpy(&range, b.data() + 8, 4);
    const size_t n = hd[0], nspp = hd[1], cnt = nspp * n * 4;
    if (b.size() != 12 + cnt * sizeof(float)) return 2;
    std::vector<float> s(cnt), o(n * 128);
    std::memcpy(s.data(), b.data() + 12, cnt * sizeof(float));
    if (!halves) {
        if (rmr_probe_vis_fold(s.data(), n, hd[1], range, o.data()) != RMR_OK) return 3;
    } else {
        // two runs of k with the sums stored in between, laid out as the kernels' state: [probe][3][64]
        float D[64][3];
        rmr_probe_vis_dirs(D);
        std::vector<float> state(n * 192, -7.0f);
        const size_t cut = nspp / 2;
        for (int pass = 0; pass < 2; pass++) {
            const size_t k0 = pass ? cut : 0, k1 = pass ? nspp : cut;
            for (size_t i = 0; i < n; i++)
                for (int j = 0; j < 64; j++) {
                    float* st = state.data() + i * 192 + j;
                    rmr::VisAcc a{0.0f, 0.0f, 0.0f};
                    if (pass) a = rmr::VisAcc{st[0], st[64], st[128]};
                    for (size_t k = k0; k < k1; k++) {
                        const float* v = s.data() + 4 * (k * n + i);
                        if (!rmr::vis_sample_used(v[3])) continue;
                        rmr::vis_fold_one(a, D[j], v[0], v[1], v[2], rmr::vis_sample_r(v[3], range));
                    }
                    st[0] = a.A; st[64] = a.M1; st[128] = a.M2;
                    if (pass) rmr::vis_resolve(a, range, o[i * 128 + 2 * j], o[i * 128 + 2 * j + 1]);
                }
        }
    }
    if (!write_all(out, o.data(), o.size() * sizeof(float))) return 4;
    std::printf("probe_vis_test %s ok\n", halves ? "fold2" : "fold");
    return 0;
}

int file_lookup(const char* in, const char* out) {
    std::vector<unsigned char> b;
    rmr_volume_desc d;
    uint32_t n;
    float bias;
    if (!read_all(in, b) || b.size() < sizeof d + 8) return 2;
    std::memcpy(&d, b.data(), sizeof d);
    std::memcpy(&n, b.data() + sizeof d, 4);
    std::memcpy(&bias, b.data() + sizeof d + 4, 4);
    if (rmr_check_volume(&d, nullptr) != RMR_OK) return 2;
    const size_t np = (size_t)d.n[0] * d.n[1] * d.n[2];
    if (b.size() != sizeof d + 8 + (np * (28 + 128) + (size_t)n * 6) * sizeof(float)) return 2;
    std::vector<float> sh(np * 28), vis(np * 128), q((size_t)n * 3), nr((size_t)n * 3), o((size_t)n * 4);
    const unsigned char* p = b.data() + sizeof d + 8;
    std::memcpy(sh.data(), p, sh.size() * sizeof(float));
    p += sh.size() * sizeof(float);
    std::memcpy(vis.data(), p, vis.size() * sizeof(float));
    p += vis.size() * sizeof(float);
    std::memcpy(q.data(), p, q.size() * sizeof(float));
    p += q.size() * sizeof(float);
    std::memcpy(nr.data(), p, nr.size() * sizeof(float));
    size_t bad = 0;
    (void)rmr_probe_irradiance_vis_host(&d, sh.data(), vis.data(), q.data(), nr.data(), n, bias, o.data(), &bad);
    const uint32_t bad32 = (uint32_t)bad;
    if (!write_all(out, o.data(), o.size() * sizeof(float), &bad32, 4)) return 4;
    std::printf("probe_vis_test lookup ok\n");
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "texel") return file_texel(argv[2], argv[3]);
    if (argc == 4 && std::string(argv[1]) == "fold") return file_fold(argv[2], argv[3], false);
    if (argc == 4 && std::string(argv[1]) == "fold2") return file_fold(argv[2], argv[3], true);
    if (argc == 4 && std::string(argv[1]) == "lookup") return file_lookup(argv[2], argv[3]);
    check_dirs();
    check_fold();
    check_lookup();
    if (failures) {
        std::printf("probe_vis_test: %d checks failed\n", failures);
        return 1;
    }
    std::printf("probe_vis_test ok\n");
    return 0;
}
