// aov_test.cpp — stand-alone CPU checks of aov.cpp (no HIP, no Python), run plain and under the address
// and undefined-behaviour sanitizers by tests/test_aov_cpu.py: the initial state, the hand case of the slot
// rule, the edge states of the resolve, the order property, the 2^24 limit and the argument checks, all on
// exactly sized heap arrays.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rmr_aov_rule.h"

namespace {
int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

const float kInf = std::numeric_limits<float>::infinity();

rmr_hit hit(float id, float t, float nx = 0.0f, float ny = 0.0f, float nz = 1.0f, float px = 0.0f, float py = 0.0f,
            float pz = 0.0f) {
    rmr_hit h;
    h.pos[0] = px; h.pos[1] = py; h.pos[2] = pz; h.t = t;
    h.n[0] = nx; h.n[1] = ny; h.n[2] = nz; h.id = id;
    return h;
}
rmr_hit miss(float t = 1000.0f) { return hit(-1.0f, t, 0.0f, 0.0f, 0.0f); }

// plane p of pixel i of an n_px state or resolved array
const float* at(const std::vector<float>& a, size_t n_px, int p, size_t i) { return &a[((size_t)p * n_px + i) * 4]; }
bool is4(const float* v, float a, float b, float c, float d) { return v[0] == a && v[1] == b && v[2] == c && v[3] == d; }

void check_init() {
    static_assert(sizeof(rmr_hit) == 32, "rmr_hit is 32 bytes");
    const size_t n = 3;
    std::vector<float> s(20 * n, 7.0f);
    CHECK(rmr_aov_init(s.data(), n) == RMR_OK);
    for (size_t i = 0; i < n; i++) {
        CHECK(is4(at(s, n, RMR_AOV_STATS, i), 0.0f, 0.0f, 0.0f, kInf));
        CHECK(is4(at(s, n, RMR_AOV_NORMAL, i), 0.0f, 0.0f, 0.0f, 0.0f));
        CHECK(is4(at(s, n, RMR_AOV_POSITION, i), 0.0f, 0.0f, 0.0f, 0.0f));
        CHECK(is4(at(s, n, RMR_AOV_IDS01, i), -1.0f, 0.0f, -1.0f, 0.0f));
        CHECK(is4(at(s, n, RMR_AOV_IDS23, i), -1.0f, 0.0f, -1.0f, 0.0f));
    }
    CHECK(rmr_aov_init(nullptr, 0) == RMR_OK);
    CHECK(rmr_aov_init(nullptr, 1) == RMR_E_INVALID);
    CHECK(rmr_aov_fold(nullptr, nullptr, 1, 1) == RMR_E_INVALID);
    CHECK(rmr_aov_fold(s.data(), nullptr, n, 1) == RMR_E_INVALID);
    CHECK(rmr_aov_fold(s.data(), nullptr, n, 0) == RMR_OK);
    CHECK(rmr_aov_resolve(s.data(), n, 10.0f, nullptr) == RMR_E_INVALID);
    CHECK(rmr_aov_resolve(nullptr, 0, 10.0f, nullptr) == RMR_OK);
}

// ids 3, 1, 4, 1, 5, 9, 2, 6, all hits: slots (3,1) (1,2) (4,1) (5,1), other 3; sequential float32 sums
void check_hand_case() {
    const float ids[8] = {3, 1, 4, 1, 5, 9, 2, 6};
    std::vector<rmr_hit> h;
    float st = 0.0f, mn = kInf, sn[3] = {0, 0, 0}, sp[3] = {0, 0, 0};
    for (int k = 0; k < 8; k++) {
        const float t = 1.1f + 0.37f * (float)k * (float)k, nx = 0.1f * (float)(k + 1), ny = -0.3f + 0.01f * (float)k,
                    nz = 1.0f / (float)(k + 3);
        const float px = 1e3f + (float)k * 0.7f, py = -2.5f * (float)k, pz = 1e-3f * (float)(k + 1);
        h.push_back(hit(ids[k], t, nx, ny, nz, px, py, pz));
        st = st + t;
        mn = t < mn ? t : mn;
        sn[0] = sn[0] + nx; sn[1] = sn[1] + ny; sn[2] = sn[2] + nz;
        sp[0] = sp[0] + px; sp[1] = sp[1] + py; sp[2] = sp[2] + pz;
    }
    std::vector<float> s(20), r(20);
    CHECK(rmr_aov_init(s.data(), 1) == RMR_OK);
    CHECK(rmr_aov_fold(s.data(), h.data(), 1, 8) == RMR_OK);
    CHECK(is4(at(s, 1, RMR_AOV_STATS, 0), 8.0f, 8.0f, st, mn));
    CHECK(is4(at(s, 1, RMR_AOV_NORMAL, 0), sn[0], sn[1], sn[2], 3.0f));
    CHECK(is4(at(s, 1, RMR_AOV_POSITION, 0), sp[0], sp[1], sp[2], 0.0f));
    CHECK(is4(at(s, 1, RMR_AOV_IDS01, 0), 3.0f, 1.0f, 1.0f, 2.0f));
    CHECK(is4(at(s, 1, RMR_AOV_IDS23, 0), 4.0f, 1.0f, 5.0f, 1.0f));
    CHECK(rmr_aov_resolve(s.data(), 1, 1000.0f, r.data()) == RMR_OK);
    CHECK(is4(at(r, 1, RMR_AOV_R_IDS01, 0), 1.0f, 2.0f / 8.0f, 3.0f, 1.0f / 8.0f));
    CHECK(is4(at(r, 1, RMR_AOV_R_IDS23, 0), 4.0f, 1.0f / 8.0f, 5.0f, 1.0f / 8.0f));
    CHECK(is4(at(r, 1, RMR_AOV_R_DEPTH, 0), st / 8.0f, mn, 1.0f, 8.0f));
    CHECK(at(r, 1, RMR_AOV_R_POSITION, 0)[3] == 8.0f && at(r, 1, RMR_AOV_R_POSITION, 0)[0] == sp[0] / 8.0f);
    const float* nn = at(r, 1, RMR_AOV_R_NORMAL, 0);
    CHECK(std::fabs(std::sqrt((double)nn[0] * nn[0] + (double)nn[1] * nn[1] + (double)nn[2] * nn[2]) - 1.0) < 1e-6);
    CHECK(nn[3] == 1.0f);
}

void check_edges() {
    // pixel 0 and 1: misses only; pixel 2: a count tie (7 twice, 2 twice, 9 once) and a miss; pixel 3: normals
    // that cancel; s1, the untouched initial state, is the n = 0 case
    const size_t n = 4;
    std::vector<float> s(20 * n), r(20 * n);
    CHECK(rmr_aov_init(s.data(), n) == RMR_OK);
    std::vector<rmr_hit> h(6 * n, miss());
    const float seq[6] = {7, 2, 9, -1, 2, 7};
    for (int k = 0; k < 6; k++) {
        if (seq[k] >= 0.0f) h[(size_t)k * n + 2] = hit(seq[k], 2.0f + (float)k);
        h[(size_t)k * n + 3] = hit(0.0f, 1.0f, (k & 1) ? 1.0f : -1.0f, 0.0f, 0.0f);
    }
    std::vector<float> s1(s);
    CHECK(rmr_aov_fold(s.data(), h.data(), n, 6) == RMR_OK);
    CHECK(rmr_aov_resolve(s.data(), n, 500.0f, r.data()) == RMR_OK);
    CHECK(is4(at(s, n, RMR_AOV_STATS, 0), 6.0f, 0.0f, 0.0f, kInf));
    CHECK(is4(at(r, n, RMR_AOV_R_DEPTH, 0), 500.0f, 500.0f, 0.0f, 6.0f));
    CHECK(is4(at(r, n, RMR_AOV_R_NORMAL, 0), 0.0f, 0.0f, 0.0f, 0.0f));
    CHECK(is4(at(r, n, RMR_AOV_R_POSITION, 0), 0.0f, 0.0f, 0.0f, 0.0f));
    CHECK(is4(at(r, n, RMR_AOV_R_IDS01, 0), -1.0f, 0.0f, -1.0f, 0.0f));
    CHECK(is4(at(r, n, RMR_AOV_R_IDS23, 0), -1.0f, 0.0f, -1.0f, 0.0f));
    // the tie: (2, 2) before (7, 2), then (9, 1), then the empty slot; 5 hits of 6 samples
    CHECK(is4(at(s, n, RMR_AOV_IDS01, 2), 7.0f, 2.0f, 2.0f, 2.0f));
    CHECK(is4(at(r, n, RMR_AOV_R_IDS01, 2), 2.0f, 2.0f / 6.0f, 7.0f, 2.0f / 6.0f));
    CHECK(is4(at(r, n, RMR_AOV_R_IDS23, 2), 9.0f, 1.0f / 6.0f, -1.0f, 0.0f));
    CHECK(at(r, n, RMR_AOV_R_DEPTH, 2)[2] == 5.0f / 6.0f && at(r, n, RMR_AOV_R_DEPTH, 2)[1] == 2.0f);
    // cancelling normals: length 0 gives the zero normal, alpha stays
    CHECK(is4(at(r, n, RMR_AOV_R_NORMAL, 3), 0.0f, 0.0f, 0.0f, 1.0f));
    // n = 0: no NaN anywhere
    CHECK(rmr_aov_resolve(s1.data(), n, 500.0f, r.data()) == RMR_OK);
    for (float v : r) CHECK(v == v);
    CHECK(is4(at(r, n, RMR_AOV_R_DEPTH, 1), 500.0f, 500.0f, 0.0f, 0.0f));
    CHECK(is4(at(r, n, RMR_AOV_R_IDS01, 1), -1.0f, 0.0f, -1.0f, 0.0f));
}

void check_order_and_limit() {
    // [A; B] in one call equals A then B; B then A differs (the slots are in first-seen order, the sums round
    // in sequence)
    std::vector<rmr_hit> A = {hit(1, 1.0f, 1e8f), hit(2, 3.0f, 1.0f)}, B = {hit(3, 0.5f, -1e8f), hit(1, 2.0f, 1.0f)};
    std::vector<rmr_hit> AB(A);
    AB.insert(AB.end(), B.begin(), B.end());
    std::vector<float> one(20), two(20), rev(20);
    rmr_aov_init(one.data(), 1);
    rmr_aov_init(two.data(), 1);
    rmr_aov_init(rev.data(), 1);
    CHECK(rmr_aov_fold(one.data(), AB.data(), 1, 4) == RMR_OK);
    CHECK(rmr_aov_fold(two.data(), A.data(), 1, 2) == RMR_OK && rmr_aov_fold(two.data(), B.data(), 1, 2) == RMR_OK);
    CHECK(rmr_aov_fold(rev.data(), B.data(), 1, 2) == RMR_OK && rmr_aov_fold(rev.data(), A.data(), 1, 2) == RMR_OK);
    CHECK(std::memcmp(one.data(), two.data(), 80) == 0);
    CHECK(std::memcmp(one.data(), rev.data(), 80) != 0);
    CHECK(at(one, 1, RMR_AOV_IDS01, 0)[0] == 1.0f && at(rev, 1, RMR_AOV_IDS01, 0)[0] == 3.0f);
    // the 2^24 limit: nothing is written by the refused call
    std::vector<float> s(40);
    rmr_aov_init(s.data(), 2);
    s[4] = 16777215.0f;   // pixel 1's n
    std::vector<rmr_hit> h(4, hit(1, 1.0f));
    const std::vector<float> before(s);
    CHECK(rmr_aov_fold(s.data(), h.data(), 2, 2) == RMR_E_INVALID);
    CHECK(std::memcmp(s.data(), before.data(), s.size() * sizeof(float)) == 0);
    CHECK(rmr_aov_fold(s.data(), h.data(), 2, 1) == RMR_OK);
    CHECK(s[4] == 16777216.0f && s[0] == 1.0f);
}
}  // namespace

int main() {
    check_init();
    check_hand_case();
    check_edges();
    check_order_and_limit();
    if (failures) {
        std::printf("aov_test: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("aov_test ok\n");
    return 0;
}
