// rmr_probe_vis_rule.h — the parts of the probes' visibility rule (include/rmr.h rmr_bake_probe_visibility /
// rmr_probe_irradiance_vis) that the host (probe_vis.cpp) and the device (rmr_probe_vis.hip)
// share: a texel's direction and a direction's texel under the octahedral map, a sample's distance, the fold of
// a probe's samples onto a texel's two moments, the resolve, and the lookup: rmr_probe_rule.h's probe_lookup
// with a back-face and a Chebyshev visibility weight per corner.
// Plain C++ and HIP: float32 sums, products, quotients and square roots, no fma, every select a comparison, so
// both sides run the same operations and NumPy reproduces them (tests/probe_vis_ref.py).
#pragma once
#include "rmr_probe_rule.h"

namespace rmr {

constexpr int kVisRes = 8;                          // texels per side of a probe's map
constexpr int kVisTexels = kVisRes * kVisRes;       // one wave
constexpr int kVisFloats = 2 * kVisTexels;          // a probe's output: vis[64][2] = (m1, m2) per texel
constexpr int kVisStateFloats = 3 * kVisTexels;     // a probe's running state: A, M1, M2 per texel

constexpr float kVisBackFloor = 0.2f;    // the back-face weight's floor
constexpr float kVisFloor = 0.05f;       // the visibility weight's floor

// The running sums of one texel.
struct VisAcc {
    float A, M1, M2;
};

RMR_PROBE_HD float vis_abs(float x) { return x < 0.0f ? -x : x; }
RMR_PROBE_HD float vis_sgn(float x) { return x >= 0.0f ? 1.0f : -1.0f; }

// D_j: the octahedral decode of texel j's centre (j = iy * 8 + ix), normalised.
RMR_PROBE_HD void vis_texel_dir(int j, float D[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int ix = j & (kVisRes - 1), iy = j >> 3;
    const float u = (((float)ix + 0.5f) / (float)kVisRes) * 2.0f - 1.0f;
    const float v = (((float)iy + 0.5f) / (float)kVisRes) * 2.0f - 1.0f;
    float x = u, y = v;
    const float z = (1.0f - vis_abs(u)) - vis_abs(v);
    if (z < 0.0f) {
        const float fx = (1.0f - vis_abs(y)) * vis_sgn(x);
        const float fy = (1.0f - vis_abs(x)) * vis_sgn(y);
        x = fx;
        y = fy;
    }
    const float xx = x * x, yy = y * y, zz = z * z;
    const float len = __builtin_sqrtf((xx + yy) + zz);
    D[0] = x / len;
    D[1] = y / len;
    D[2] = z / len;
}

// One axis of the texel: floor(((o * 0.5) + 0.5) * 8) kept in [0, 7]; a NaN coordinate gives 0.
RMR_PROBE_HD int vis_texel_axis(float o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float h = o * 0.5f;
    const float s = h + 0.5f;
    float f = __builtin_floorf(s * (float)kVisRes);
    f = f > 0.0f ? f : 0.0f;
    f = f < (float)(kVisRes - 1) ? f : (float)(kVisRes - 1);
    return (int)f;
}

// The texel of a direction (not normalised): the nearest one under the octahedral encode.
RMR_PROBE_HD int vis_texel_of(float x, float y, float z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float s = (vis_abs(x) + vis_abs(y)) + vis_abs(z);
    float ox = x / s, oy = y / s;
    if (z < 0.0f) {
        const float fx = (1.0f - vis_abs(oy)) * vis_sgn(x);
        const float fy = (1.0f - vis_abs(ox)) * vis_sgn(y);
        ox = fx;
        oy = fy;
    }
    return vis_texel_axis(oy) * kVisRes + vis_texel_axis(ox);
}

// A sample's distance from the march's t: r = t < range ? t : range; a t that is not finite: no sample.
RMR_PROBE_HD bool vis_sample_used(float t) { return __builtin_isfinite(t); }
RMR_PROBE_HD float vis_sample_r(float t, float range) { return t < range ? t : range; }

// One sample (d, r) met by the texel of direction D.
RMR_PROBE_HD void vis_fold_one(VisAcc& s, const float D[3], float dx, float dy, float dz, float r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float cx = D[0] * dx, cy = D[1] * dy, cz = D[2] * dz;
    const float c = (cx + cy) + cz;
    if (!(c > 0.0f)) return;
    const float c2 = c * c;
    const float c4 = c2 * c2;
    const float c8 = c4 * c4;
    const float c16 = c8 * c8;
    const float w = c16 * c16;
    const float wr = w * r;
    const float rr = r * r;
    const float wrr = w * rr;
    s.A = s.A + w;
    s.M1 = s.M1 + wr;
    s.M2 = s.M2 + wrr;
}

// (m1, m2) of a texel: the sums over A, or (range, range * range) for a texel no sample touched.
RMR_PROBE_HD void vis_resolve(const VisAcc& s, float range, float& m1, float& m2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float q1 = s.M1 / s.A, q2 = s.M2 / s.A;
    const float far2 = range * range;
    m1 = s.A > 0.0f ? q1 : range;
    m2 = s.A > 0.0f ? q2 : far2;
}

RMR_PROBE_HD bool vis_range_ok(float range) { return __builtin_isfinite(range) && range > 0.0f; }
RMR_PROBE_HD bool vis_bias_ok(float bias) { return __builtin_isfinite(bias) && bias >= 0.0f; }

// The two weights of one corner: the probe at P with the map `vis` (its 128 floats), seen from qb with the
// normal nrm. wb: the back-face weight, wv: the visibility weight.
RMR_PROBE_HD void vis_corner_weights(const float* vis, const float P[3], const float qb[3], const float nrm[3], float& wb,
                                     float& wv) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float vx = qb[0] - P[0], vy = qb[1] - P[1], vz = qb[2] - P[2];
    const float xx = vx * vx, yy = vy * vy, zz = vz * vz;
    const float r = __builtin_sqrtf((xx + yy) + zz);
    if (r == 0.0f) {
        wb = 1.0f;
        wv = 1.0f;
        return;
    }
    const float nx = vx * nrm[0], ny = vy * nrm[1], nz = vz * nrm[2];
    const float dn = (nx + ny) + nz;
    const float b = -dn / r;
    const float h = (b + 1.0f) * 0.5f;
    wb = (h * h) + kVisBackFloor;
    const float dx = vx / r, dy = vy / r, dz = vz / r;
    const int j = vis_texel_of(dx, dy, dz);
    const float m1 = vis[2 * j], m2 = vis[2 * j + 1];
    const float mm = m1 * m1;
    const float df = m2 - mm;
    const float var = vis_abs(df);
    const float dl = r - m1;
    const float dd = dl * dl;
    const float ch = var / (var + dd);
    float w = (ch * ch) * ch;
    w = w < kVisFloor ? kVisFloor : w;
    wv = r <= m1 ? 1.0f : w;
}

// out_rgba of one query (which the reject rule has passed) over the field sh[n_points][28] and its visibility
// vis[n_points][128]: probe_lookup with g = (g0 * wb) * wv per valid corner.
RMR_PROBE_HD void probe_lookup_vis(const rmr_volume_desc& d, const float* sh, const float* vis, const float q[3],
                                   const float nrm[3], float bias, float out[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int c[3];
    float w[3];
    for (int a = 0; a < 3; a++) probe_cell(q[a], d.origin[a], d.spacing, d.n[a], c[a], w[a]);
    const size_t sy = (size_t)d.n[0], sz = (size_t)d.n[0] * (size_t)d.n[1];
    const size_t base = (size_t)c[0] + sy * (size_t)c[1] + sz * (size_t)c[2];
    float qb[3];
    for (int a = 0; a < 3; a++) {
        const float t = bias * nrm[a];
        qb[a] = q[a] + t;
    }
    float B[kProbeFloats - 1];
    for (int j = 0; j < kProbeFloats - 1; j++) B[j] = 0.0f;
    float W = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int k = 0; k < 8; k++) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
        const size_t pi = base + (size_t)dx + (size_t)dy * sy + (size_t)dz * sz;
        const float* p = sh + pi * kProbeFloats;
        const float ux = dx ? w[0] : 1.0f - w[0], uy = dy ? w[1] : 1.0f - w[1], uz = dz ? w[2] : 1.0f - w[2];
        const float uxy = ux * uy;
        const float g0 = uxy * uz;
        float g = 0.0f;
        if (p[kProbeFloats - 1] > 0.0f) {   // (a probe is valid iff n_used > 0)
            float P[3];
            P[0] = lattice_coord(d.origin[0], c[0] + dx, d.spacing);
            P[1] = lattice_coord(d.origin[1], c[1] + dy, d.spacing);
            P[2] = lattice_coord(d.origin[2], c[2] + dz, d.spacing);
            float wb, wv;
            vis_corner_weights(vis + pi * kVisFloats, P, qb, nrm, wb, wv);
            const float gb = g0 * wb;
            g = gb * wv;
        }
        W = W + g;
        for (int j = 0; j < kProbeFloats - 1; j++) {
            const float t = g * p[j];
            B[j] = B[j] + t;
        }
    }
    float Y[kProbeSH];
    sh_basis(nrm[0], nrm[1], nrm[2], Y);
    for (int ch = 0; ch < 3; ch++) {
        float t[kProbeSH];
        for (int m = 0; m < kProbeSH; m++) t[m] = B[3 * m + ch] * Y[m];
        const float t0 = t[0];
        const float t1 = ((t[1] + t[2]) + t[3]) * kLobe1;
        const float t2 = ((((t[4] + t[5]) + t[6]) + t[7]) + t[8]) * kLobe2;
        const float e = (t0 + t1) + t2;
        const float v = e / W;
        out[ch] = W > 0.0f ? (v > 0.0f ? v : 0.0f) : 0.0f;
    }
    out[3] = W;
}

}  // namespace rmr
