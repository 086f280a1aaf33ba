// probe_test.cpp — stand-alone CPU check of the irradiance probes' host functions (probe.cpp, rmr_probe_rule.h):
// the parameter ranges, the basis, the fold's edge cases and the lookup's. tests/test_probes_cpu.py builds and
// runs it, plain and under the sanitizers.
//   probe_test                  the checks
//   probe_test fold IN OUT      rmr_probe_fold of a file: uint32 n, nspp, then L [nspp][n][3], dirs [nspp][n][3];
//                               OUT: sh [n][28]
//   probe_test lookup IN OUT    rmr_probe_irradiance_host of a file: rmr_volume_desc, uint32 n, then sh [points][28],
//                               points [n][3], normals [n][3]; OUT: rgba [n][4], then uint32 first_bad
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "rmr_probe_rule.h"

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
    rmr_probe_params p;
    std::memset(&p, 0xff, sizeof p);
    rmr_default_probe_params(&p);
    CHECK(p.clearance == 0.0f && p.origin_extent == 0.0f && p.first_index == 0);
    static_assert(sizeof(rmr_probe_params) == 16, "rmr_probe_params is 16 bytes");
    CHECK(rmr_check_probe_params(&p) == RMR_OK);
    CHECK(rmr_check_probe_params(nullptr) == RMR_E_INVALID);
    for (float cl : {kNaN, kInf, -kInf, -0.001f}) {
        rmr_probe_params q = p;
        q.clearance = cl;
        CHECK(rmr_check_probe_params(&q) == RMR_E_INVALID);
    }
    rmr_probe_params q = p;
    q.clearance = 0.25f;
    q.origin_extent = kNaN;   // (not looked at)
    CHECK(rmr_check_probe_params(&q) == RMR_OK);
    q.first_index = (uint64_t)1 << 36;
    CHECK(rmr_check_probe_params(&q) == RMR_OK);
    q.first_index = ((uint64_t)1 << 36) + 1;
    CHECK(rmr_check_probe_params(&q) == RMR_E_INVALID);
    // the reject and buried rules
    const float a[3] = {1.0f, -2.0f, 3.0f}, b[3] = {1.0f, kNaN, 3.0f}, c[3] = {kInf, 0.0f, 0.0f};
    CHECK(rmr::probe_point_ok(a, kInf) && rmr::probe_point_ok(a, 3.0f) && !rmr::probe_point_ok(a, 2.9999998f));
    CHECK(!rmr::probe_point_ok(b, kInf) && !rmr::probe_point_ok(c, kInf));
    CHECK(!rmr::probe_buried(0.0f, 0.0f) && rmr::probe_buried(-1e-6f, 0.0f) && rmr::probe_buried(kNaN, 0.0f));
    CHECK(!rmr::probe_buried(0.25f, 0.25f) && rmr::probe_buried(0.24999999f, 0.25f));
}

void check_basis() {
    const float d[4][3] = {{0, 0, 1}, {0, 1, 0}, {1, 0, 0}, {0.6f, 0.0f, 0.8f}};
    float Y[4][9];
    CHECK(rmr_sh_basis(&d[0][0], 4, &Y[0][0]) == RMR_OK);
    CHECK(rmr_sh_basis(nullptr, 1, &Y[0][0]) == RMR_E_INVALID && rmr_sh_basis(nullptr, 0, nullptr) == RMR_OK);
    for (int i = 0; i < 4; i++) CHECK(Y[i][0] == 0.282095f);
    CHECK(Y[0][2] == 0.488603f && Y[0][1] == 0.0f && Y[0][3] == 0.0f && Y[0][6] == 0.315392f * 2.0f);
    CHECK(Y[1][1] == 0.488603f && Y[1][8] == -0.546274f && Y[1][6] == -0.315392f);
    CHECK(Y[2][3] == 0.488603f && Y[2][8] == 0.546274f);
    CHECK(Y[3][7] == 1.092548f * (0.6f * 0.8f) && Y[3][4] == 0.0f);
}

void check_fold() {
    // 3 samples of 3 probes: all used; one sample NaN; every sample non-finite
    const size_t n = 3;
    const uint32_t nspp = 3;
    std::vector<float> L(nspp * n * 3, 1.0f), D(nspp * n * 3, 0.0f), out(n * 28, -1.0f);
    for (size_t u = 0; u < nspp * n; u++) D[3 * u + 2] = 1.0f;   // d = +z
    L[3 * (1 * n + 1) + 0] = kNaN;
    for (uint32_t k = 0; k < nspp; k++) L[3 * (k * n + 2) + 1] = k == 1 ? -kInf : kInf;
    CHECK(rmr_probe_fold(L.data(), D.data(), n, nspp, out.data()) == RMR_OK);
    CHECK(out[27] == 3.0f && out[28 + 27] == 2.0f && out[56 + 27] == 0.0f);
    const float y0 = 0.282095f;
    const float s3 = (((y0 + y0) + y0) * 12.566371f) / 3.0f, s2 = ((y0 + y0) * 12.566371f) / 2.0f;
    for (int c = 0; c < 3; c++) {
        CHECK(out[c] == s3 && out[28 + c] == s2);
        CHECK(out[3 * 1 + c] == 0.0f && out[3 * 3 + c] == 0.0f);   // Y1, Y3 of +z
    }
    for (int j = 0; j < 28; j++) CHECK(out[56 + j] == 0.0f);
    CHECK(rmr_probe_fold(L.data(), D.data(), n, 0, out.data()) == RMR_E_INVALID);
    CHECK(rmr_probe_fold(L.data(), D.data(), n, (1u << 24) + 1, out.data()) == RMR_E_INVALID);
    CHECK(rmr_probe_fold(nullptr, D.data(), n, nspp, out.data()) == RMR_E_INVALID);
    CHECK(rmr_probe_fold(nullptr, nullptr, 0, nspp, nullptr) == RMR_OK);
}

void check_lookup() {
    // a 2 x 2 x 2 field under a constant radiance: sh0 = L / Y0 (so that B0 Y0 = L), every other coefficient 0
    rmr_volume_desc d{{-1.0f, 0.0f, 2.0f}, 0.5f, {2, 2, 2}};
    std::vector<float> sh(8 * 28, 0.0f);
    for (int k = 0; k < 8; k++) {
        for (int c = 0; c < 3; c++) sh[28 * k + c] = (float)(c + 1);
        sh[28 * k + 27] = 16.0f;
    }
    const float q[5][3] = {{-0.75f, 0.25f, 2.25f}, {-1.0f, 0.0f, 2.0f}, {9.0f, -9.0f, 2.5f}, {kNaN, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    const float nr[5][3] = {{0, 1, 0}, {0, 0, 1}, {1, 0, 0}, {0, 1, 0}, {0, 2, 0}};
    float out[5][4];
    size_t bad = 99;
    CHECK(rmr_probe_irradiance_host(&d, sh.data(), &q[0][0], &nr[0][0], 3, &out[0][0], &bad) == RMR_OK && bad == 3);
    for (int i = 0; i < 3; i++) {
        CHECK(out[i][3] == 1.0f);
        for (int c = 0; c < 3; c++) CHECK(out[i][c] == (float)(c + 1) * 0.282095f);
    }
    CHECK(rmr_probe_irradiance_host(&d, sh.data(), &q[0][0], &nr[0][0], 5, &out[0][0], &bad) == RMR_E_INVALID && bad == 3);
    for (int i = 3; i < 5; i++)
        for (int c = 0; c < 4; c++) CHECK(out[i][c] == 0.0f);
    CHECK(out[0][3] == 1.0f);
    // invalid corners drop out and the rest is renormalised; none valid: 0
    sh[28 * 1 + 27] = 0.0f;
    sh[28 * 1 + 0] = 1000.0f;
    CHECK(rmr_probe_irradiance_host(&d, sh.data(), &q[0][0], &nr[0][0], 1, &out[0][0], nullptr) == RMR_OK);
    CHECK(out[0][3] == 0.875f && out[0][0] == (0.875f * 0.282095f) / 0.875f);
    for (int k = 0; k < 8; k++) sh[28 * k + 27] = 0.0f;
    CHECK(rmr_probe_irradiance_host(&d, sh.data(), &q[0][0], &nr[0][0], 1, &out[0][0], nullptr) == RMR_OK);
    for (int c = 0; c < 4; c++) CHECK(out[0][c] == 0.0f);
    d.n[0] = 1;
    CHECK(rmr_probe_irradiance_host(&d, sh.data(), &q[0][0], &nr[0][0], 1, &out[0][0], nullptr) == RMR_E_INVALID);
    CHECK(rmr_probe_irradiance_host(nullptr, sh.data(), &q[0][0], &nr[0][0], 1, &out[0][0], nullptr) == RMR_E_INVALID);
    // the cell rule: clamped outside, the upper boundary belongs to the last cell with w = 1
    int c;
    float w;
    rmr::probe_cell(1.0f, 0.0f, 0.5f, 3, c, w);
    CHECK(c == 1 && w == 1.0f);
    rmr::probe_cell(0.75f, 0.0f, 0.5f, 3, c, w);
    CHECK(c == 1 && w == 0.5f);
    rmr::probe_cell(-3.0f, 0.0f, 0.5f, 3, c, w);
    CHECK(c == 0 && w == 0.0f);
    rmr::probe_cell(3.4e38f, -3.4e38f, 1e-30f, 3, c, w);
    CHECK(c == 1 && w == 1.0f);
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

int file_fold(const char* in, const char* out) {
    std::vector<unsigned char> b;
    if (!read_all(in, b) || b.size() < 8) return 2;
    uint32_t hd[2];
    std::memcpy(hd, b.data(), 8);
    const size_t n = hd[0], cnt = (size_t)hd[1] * n * 3;
    if (b.size() != 8 + 2 * cnt * sizeof(float)) return 2;
    std::vector<float> L(cnt), D(cnt), o(n * 28);
    std::memcpy(L.data(), b.data() + 8, cnt * sizeof(float));
    std::memcpy(D.data(), b.data() + 8 + cnt * sizeof(float), cnt * sizeof(float));
    if (rmr_probe_fold(L.data(), D.data(), n, hd[1], o.data()) != RMR_OK) return 3;
    if (!write_all(out, o.data(), o.size() * sizeof(float))) return 4;
    std::printf("probe_test fold ok\n");
    return 0;
}

int file_lookup(const char* in, const char* out) {
    std::vector<unsigned char> b;
    rmr_volume_desc d;
    uint32_t n;
    if (!read_all(in, b) || b.size() < sizeof d + 4) return 2;
    std::memcpy(&d, b.data(), sizeof d);
    std::memcpy(&n, b.data() + sizeof d, 4);
    if (rmr_check_volume(&d, nullptr) != RMR_OK) return 2;
    const size_t np = (size_t)d.n[0] * d.n[1] * d.n[2];
    if (b.size() != sizeof d + 4 + (np * 28 + (size_t)n * 6) * sizeof(float)) return 2;
    std::vector<float> sh(np * 28), q((size_t)n * 3), nr((size_t)n * 3), o((size_t)n * 4);
    const unsigned char* p = b.data() + sizeof d + 4;
    std::memcpy(sh.data(), p, sh.size() * sizeof(float));
    std::memcpy(q.data(), p + sh.size() * sizeof(float), q.size() * sizeof(float));
    std::memcpy(nr.data(), p + (sh.size() + q.size()) * sizeof(float), nr.size() * sizeof(float));
    size_t bad = 0;
    (void)rmr_probe_irradiance_host(&d, sh.data(), q.data(), nr.data(), n, o.data(), &bad);
    const uint32_t bad32 = (uint32_t)bad;
    if (!write_all(out, o.data(), o.size() * sizeof(float), &bad32, 4)) return 4;
    std::printf("probe_test lookup ok\n");
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "fold") return file_fold(argv[2], argv[3]);
    if (argc == 4 && std::string(argv[1]) == "lookup") return file_lookup(argv[2], argv[3]);
    check_params();
    check_basis();
    check_fold();
    check_lookup();
    if (failures) {
        std::printf("probe_test: %d checks failed\n", failures);
        return 1;
    }
    std::printf("probe_test ok\n");
    return 0;
}
