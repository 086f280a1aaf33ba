// bloom.cpp — see bloom.hpp. No HIP: built into librmr.so and, with bloom_test.cpp, into a stand-alone
// CPU check (plain and under the sanitizers). rmr_bloom_pixels runs the same header the kernels compile
// (rmr_bloom_rule.h), level by level as the kernels do.
#include "bloom.hpp"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace rmr {

bool bloom_params_ok(const rmr_bloom_params& p) {
    return p.levels >= 1 && p.levels <= kBloomMaxLevels && std::isfinite(p.threshold) && p.threshold >= 0.0f &&
           std::isfinite(p.clamp) && p.clamp >= 0.0f && p.scatter >= 0.0f && p.scatter <= 1.0f &&
           std::isfinite(p.intensity) && p.intensity >= 0.0f && p.reserved[0] == 0 && p.reserved[1] == 0 &&
           p.reserved[2] == 0;
}

BloomLevels bloom_levels(int W, int H, int levels) {
    BloomLevels L{};
    L.w[0] = W;
    L.h[0] = H;
    size_t at = 0;
    for (int k = 1; k <= kBloomMaxLevels; k++) {
        L.w[k] = bloom_half(L.w[k - 1]);
        L.h[k] = bloom_half(L.h[k - 1]);
        L.off[k] = at;
        if (k <= levels) at += (size_t)L.w[k] * L.h[k];
    }
    L.total = at;
    return L;
}

namespace {
using Img = std::vector<Bloom3>;

// down along x of every row, then along y of the result
void down2(const Img& a, int w, int h, Img& tmp, Img& out) {
    const int w2 = bloom_half(w), h2 = bloom_half(h);
    tmp.resize((size_t)w2 * h);
    for (int y = 0; y < h; y++) {
        const Bloom3* row = &a[(size_t)y * w];
        for (int j = 0; j < w2; j++) {
            const int i = 2 * j;
            tmp[(size_t)y * w2 + j] = bloom_down3(row[bloom_cl(i - 1, w)], row[bloom_cl(i, w)], row[bloom_cl(i + 1, w)],
                                                  row[bloom_cl(i + 2, w)]);
        }
    }
    out.resize((size_t)w2 * h2);
    for (int j = 0; j < h2; j++) {
        const int i = 2 * j;
        const Bloom3 *rm = &tmp[(size_t)bloom_cl(i - 1, h) * w2], *r0 = &tmp[(size_t)bloom_cl(i, h) * w2],
                     *r1 = &tmp[(size_t)bloom_cl(i + 1, h) * w2], *r2 = &tmp[(size_t)bloom_cl(i + 2, h) * w2];
        for (int x = 0; x < w2; x++) out[(size_t)j * w2 + x] = bloom_down3(rm[x], r0[x], r1[x], r2[x]);
    }
}

// one value of up(b) at (x, y) of the w x h target, b being mw x mh: along x in the near and the far
// row, then along y
Bloom3 up_at(const Img& b, int mw, int mh, int x, int y) {
    const int jx = x >> 1, fx = bloom_up_far(x, mw), jy = y >> 1, fy = bloom_up_far(y, mh);
    const Bloom3 near = bloom_up3(b[(size_t)jy * mw + jx], b[(size_t)jy * mw + fx]);
    const Bloom3 far = bloom_up3(b[(size_t)fy * mw + jx], b[(size_t)fy * mw + fx]);
    return bloom_up3(near, far);
}
}  // namespace

}  // namespace rmr

extern "C" {

void rmr_default_bloom_params(rmr_bloom_params* p) {
    if (!p) return;
    p->levels = 5;
    p->threshold = 1.0f;
    p->clamp = 0.0f;
    p->scatter = 0.7f;
    p->intensity = 0.2f;
    p->reserved[0] = p->reserved[1] = p->reserved[2] = 0;
}

int rmr_check_bloom_params(const rmr_bloom_params* p) { return p && rmr::bloom_params_ok(*p) ? RMR_OK : RMR_E_INVALID; }

int rmr_bloom_pixels(const rmr_bloom_params* p, const float* rgba, int w, int h, float* out) {
    using namespace rmr;
    if (!rgba || !out || w < 1 || h < 1) return RMR_E_INVALID;
    rmr_bloom_params q;
    rmr_default_bloom_params(&q);
    if (p) q = *p;
    if (!bloom_params_ok(q)) return RMR_E_INVALID;
    try {
        const int N = q.levels;
        std::vector<Img> B((size_t)N + 1);
        Img tmp;
        int lw[kBloomMaxLevels + 1], lh[kBloomMaxLevels + 1];
        lw[0] = w;
        lh[0] = h;
        B[0].resize((size_t)w * h);
        for (size_t i = 0; i < (size_t)w * h; i++)
            B[0][i] = bloom_bright(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3], q.threshold, q.clamp);
        for (int k = 1; k <= N; k++) {
            down2(B[k - 1], lw[k - 1], lh[k - 1], tmp, B[k]);
            lw[k] = bloom_half(lw[k - 1]);
            lh[k] = bloom_half(lh[k - 1]);
            if (k == 1) Img().swap(B[0]);
        }
        for (int k = N - 1; k >= 1; k--)
            for (int y = 0; y < lh[k]; y++)
                for (int x = 0; x < lw[k]; x++) {
                    const Bloom3 u = up_at(B[k + 1], lw[k + 1], lh[k + 1], x, y);
                    Bloom3& b = B[k][(size_t)y * lw[k] + x];
                    b.x = bloom_mad(b.x, q.scatter, u.x);
                    b.y = bloom_mad(b.y, q.scatter, u.y);
                    b.z = bloom_mad(b.z, q.scatter, u.z);
                }
        const float gain = bloom_gain(q.intensity, q.scatter, N);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t i = (size_t)y * w + x;
                const float* s = rgba + 4 * i;
                float* o = out + 4 * i;
                if (bloom_invalid(s[0], s[1], s[2], s[3])) {
                    std::memcpy(o, s, 4 * sizeof(float));
                    continue;
                }
                const Bloom3 g = up_at(B[1], lw[1], lh[1], x, y);
                o[0] = bloom_mad(s[0], gain, g.x);
                o[1] = bloom_mad(s[1], gain, g.y);
                o[2] = bloom_mad(s[2], gain, g.z);
                std::memcpy(o + 3, s + 3, sizeof(float));
            }
    } catch (const std::bad_alloc&) {
        return RMR_E_NOMEM;
    }
    return RMR_OK;
}

}  // extern "C"
