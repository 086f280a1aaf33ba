// adaptive_test.cpp — stand-alone CPU checks of adaptive.cpp (no HIP, no Python), run plain and under
// the address and undefined-behaviour sanitizers by tests/test_adaptive_cpu.py: the decision rule against
// a brute-force statement on exactly sized heap buffers (ragged block edges, +inf / NaN / 0 entries), the
// tile list of the open blocks, the parameter ranges.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "adaptive.hpp"

namespace {
int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

uint32_t rng_state = 12345u;
float rnd() {   // xorshift, [0, 1)
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

void check_select(int tx, int ty, int bt) {
    const int bx = rmr::adaptive_blocks(tx, bt), by = rmr::adaptive_blocks(ty, bt);
    std::vector<uint8_t> open((size_t)bx * by, 1), want((size_t)bx * by, 1);
    const float thr = 0.25f;
    for (int call = 0; call < 4; call++) {
        std::vector<float> err((size_t)tx * ty);
        for (float& e : err) {
            const float u = rnd();
            e = u < 0.1f ? 0.0f : u < 0.2f ? std::numeric_limits<float>::infinity()
              : u < 0.25f ? std::numeric_limits<float>::quiet_NaN() : 0.5f * rnd();
        }
        int n_want = 0;
        std::vector<float> m((size_t)bx * by, -std::numeric_limits<float>::infinity());   // block maxima, NaN ignored
        for (int y = 0; y < ty; y++)
            for (int x = 0; x < tx; x++) {
                float& b = m[(size_t)(y / bt) * bx + x / bt];
                if (err[(size_t)y * tx + x] > b) b = err[(size_t)y * tx + x];
            }
        for (size_t i = 0; i < want.size(); i++) {
            want[i] = (want[i] && m[i] > thr) ? 1 : 0;
            n_want += want[i];
        }
        const int n = rmr::adaptive_select(err.data(), tx, ty, bt, thr, open.data());
        CHECK(n == n_want);
        CHECK(open == want);
        CHECK(rmr_adaptive_select(err.data(), tx, ty, bt, thr, open.data()) == n);   // idempotent on the same map
        // the tile list: every tile of an open block once, inside the lattice, row-major
        const std::vector<int32_t> t = rmr::adaptive_tiles(open.data(), tx, ty, bt);
        size_t k = 0;
        for (int y = 0; y < ty; y++)
            for (int x = 0; x < tx; x++)
                if (open[(size_t)(y / bt) * bx + x / bt]) {
                    CHECK(k + 1 < t.size() && t[k] == 8 * x && t[k + 1] == 8 * y);
                    k += 2;
                }
        CHECK(k == t.size());
    }
}
}  // namespace

int main() {
    for (int bt = 1; bt <= 8; bt++) {
        check_select(6, 5, bt);
        check_select(1, 1, bt);
        check_select(17, 3, bt);
        check_select(240, 135, bt);
    }
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> e(6, 1.0f);
    std::vector<uint8_t> o(6, 1);
    CHECK(rmr_adaptive_select(nullptr, 3, 2, 1, 0.5f, o.data()) == RMR_E_INVALID);
    CHECK(rmr_adaptive_select(e.data(), 3, 2, 1, 0.5f, nullptr) == RMR_E_INVALID);
    CHECK(rmr_adaptive_select(e.data(), 0, 2, 1, 0.5f, o.data()) == RMR_E_INVALID);
    CHECK(rmr_adaptive_select(e.data(), 3, 2, 0, 0.5f, o.data()) == RMR_E_INVALID);
    CHECK(rmr_adaptive_select(e.data(), 3, 2, 9, 0.5f, o.data()) == RMR_E_INVALID);
    CHECK(rmr_adaptive_select(e.data(), 3, 2, 1, nan, o.data()) == RMR_E_INVALID);
    CHECK(rmr_adaptive_select(e.data(), 3, 2, 1, -1.0f, o.data()) == RMR_E_INVALID);
    CHECK(rmr_adaptive_select(e.data(), 3, 2, 1, 0.5f, o.data()) == 6);

    rmr_adaptive_params p;
    rmr_default_adaptive_params(&p);
    CHECK(p.threshold == 0.1f && p.offset == 1e-4f && p.min_samples == 16 && p.pass_samples == 16 &&
          p.max_samples == 0 && p.block_tiles == 2);
    CHECK(rmr_check_adaptive_params(&p) == RMR_E_INVALID);   // max_samples has no default
    p.max_samples = 64;
    CHECK(rmr_check_adaptive_params(&p) == RMR_OK);
    CHECK(rmr_check_adaptive_params(nullptr) == RMR_E_INVALID);
    rmr_adaptive_params q = p;
    q.threshold = nan; CHECK(!rmr::adaptive_params_ok(q)); q = p;
    q.threshold = inf; CHECK(!rmr::adaptive_params_ok(q)); q = p;
    q.threshold = -0.1f; CHECK(!rmr::adaptive_params_ok(q)); q = p;
    q.threshold = 0.0f; CHECK(rmr::adaptive_params_ok(q)); q = p;
    q.offset = 0.0f; CHECK(!rmr::adaptive_params_ok(q)); q = p;
    q.offset = inf; CHECK(!rmr::adaptive_params_ok(q)); q = p;
    q.min_samples = 1; CHECK(!rmr::adaptive_params_ok(q)); q = p;
    q.pass_samples = 0; CHECK(!rmr::adaptive_params_ok(q)); q = p;
    q.max_samples = 15; CHECK(!rmr::adaptive_params_ok(q)); q = p;
    q.max_samples = 16; CHECK(rmr::adaptive_params_ok(q)); q = p;
    q.block_tiles = 0; CHECK(!rmr::adaptive_params_ok(q)); q = p;
    q.block_tiles = 9; CHECK(!rmr::adaptive_params_ok(q)); q = p;
    q.block_tiles = 8; CHECK(rmr::adaptive_params_ok(q));
    if (failures) {
        std::printf("adaptive_test: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("adaptive_test ok\n");
    return 0;
}
