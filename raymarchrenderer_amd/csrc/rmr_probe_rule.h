// rmr_probe_rule.h — the parts of the irradiance probes' rule (include/rmr.h rmr_bake_probes /
// rmr_probe_irradiance) that the host (probe.cpp) and the device (rmr_probe.hip) share: a
// probe's reject rule, the nine basis functions, the fold of a probe's samples onto its coefficients, the
// resolve, and the lookup: a query's cell and weights, the eight-corner gather and the clamped-cosine resolve.
// Plain C++ and HIP: float32 sums, products and quotients, no fma, every select a comparison, so both sides
// run the same operations and NumPy reproduces them (tests/probe_ref.py).
#pragma once
#include <stdint.h>
#include "rmr_bake_rule.h"
#include "rmr_mesh_rule.h"

#if defined(__HIP__)
#define RMR_PROBE_HD __host__ __device__ inline
#else
#define RMR_PROBE_HD inline
#endif

namespace rmr {

constexpr int kProbeSH = 9;        // basis functions
constexpr int kProbeFloats = 28;   // a probe's output and running state: sh[9][3], then n_used

// the basis' constants and the resolves' factors, written once (tests/probe_ref.py copies the literals)
constexpr float kY0 = 0.282095f;
constexpr float kY1 = 0.488603f;
constexpr float kY2 = 1.092548f;
constexpr float kY6 = 0.315392f;
constexpr float kY8 = 0.546274f;
constexpr float kFourPi = 12.566371f;
constexpr float kLobe1 = 0.6666667f;   // the clamped-cosine lobe's band factors over pi: 1, 2/3, 1/4
constexpr float kLobe2 = 0.25f;

// What every probe kernel reads of the call. points == nullptr: the probes are the lattice's points, probe j
// the point of linear index j (rmr_mesh_rule.h lattice_coord).
struct ProbeList {
    const float* points;    // [n][3], or nullptr
    float origin[3];
    float spacing;
    int32_t nx, ny;
    uint64_t n;
    uint64_t first_index;
    const float* times;     // [nspp], device
    uint32_t nspp;
    float clearance;
    float extent;           // the caller's bound on |p coordinate| (+inf: none)
};

// probe i's position
RMR_PROBE_HD void probe_point(const ProbeList& B, uint64_t i, float p[3]) {
    if (B.points) {
        for (int a = 0; a < 3; a++) p[a] = B.points[3 * i + a];
        return;
    }
    const uint32_t k = (uint32_t)i;
    const uint32_t row = k / (uint32_t)B.nx;
    const int ix = (int)(k - row * (uint32_t)B.nx);
    const int iz = (int)(row / (uint32_t)B.ny);
    const int iy = (int)(row - (uint32_t)iz * (uint32_t)B.ny);
    p[0] = lattice_coord(B.origin[0], ix, B.spacing);
    p[1] = lattice_coord(B.origin[1], iy, B.spacing);
    p[2] = lattice_coord(B.origin[2], iz, B.spacing);
}

// A probe is rejected iff a coordinate is not finite or exceeds the caller's bound.
RMR_PROBE_HD bool probe_point_ok(const float p[3], float extent) {
    bool ok = true;
    for (int a = 0; a < 3; a++) ok = ok && __builtin_isfinite(p[a]) && (p[a] < 0.0f ? -p[a] : p[a]) <= extent;
    return ok;
}

// A probe is buried iff !(map(p).x >= clearance): a NaN distance buries it.
RMR_PROBE_HD bool probe_buried(float dist, float clearance) { return !(dist >= clearance); }

// Y_0 .. Y_8 of a unit vector
RMR_PROBE_HD void sh_basis(float x, float y, float z, float Y[kProbeSH]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float xy = x * y, yz = y * z, zz = z * z, xz = x * z, xx = x * x, yy = y * y;
    const float z3 = 3.0f * zz;
    Y[0] = kY0;
    Y[1] = kY1 * y;
    Y[2] = kY1 * z;
    Y[3] = kY1 * x;
    Y[4] = kY2 * xy;
    Y[5] = kY2 * yz;
    Y[6] = kY6 * (z3 - 1.0f);
    Y[7] = kY2 * xz;
    Y[8] = kY8 * (xx - yy);
}

// a sample with a non-finite component of L is skipped
RMR_PROBE_HD bool probe_sample_used(float lr, float lg, float lb) {
    return __builtin_isfinite(lr) && __builtin_isfinite(lg) && __builtin_isfinite(lb);
}

// S[c] = S[c] + (L[c] * Y) for one basis function: the product rounded, then the sum
RMR_PROBE_HD void probe_fold_one(float s[3], float lr, float lg, float lb, float Y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float pr = lr * Y, pg = lg * Y, pb = lb * Y;
    s[0] = s[0] + pr;
    s[1] = s[1] + pg;
    s[2] = s[2] + pb;
}

// sh = (S * 4 pi) / n_used; n_used == 0: 0
RMR_PROBE_HD float probe_resolve_one(float s, float n_used) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float t = s * kFourPi;
    return n_used > 0.0f ? t / n_used : 0.0f;
}

// ---- the lookup ----------------------------------------------------------------------------------------
// The cell of a query coordinate on one axis: f = (q - origin) / spacing, c = floor(f) clamped to [0, n - 2],
// w = f - (float)c clamped to [0, 1] (a point outside the box takes the boundary's value).
RMR_PROBE_HD void probe_cell(float q, float origin, float spacing, int n, int& c, float& w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float rel = q - origin;
    const float f = rel / spacing;
    float fl = __builtin_floorf(f);
    const float hi = (float)(n - 2);
    fl = fl < 0.0f ? 0.0f : fl;
    fl = fl > hi ? hi : fl;
    c = (int)fl;
    float t = f - fl;
    t = t < 0.0f ? 0.0f : t;
    t = t > 1.0f ? 1.0f : t;
    w = t;
}

// out_rgba of one query (which the reject rule has passed) over the field sh[n_points][28]
RMR_PROBE_HD void probe_lookup(const rmr_volume_desc& d, const float* sh, const float q[3], const float nrm[3], float out[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int c[3];
    float w[3];
    for (int a = 0; a < 3; a++) probe_cell(q[a], d.origin[a], d.spacing, d.n[a], c[a], w[a]);
    const size_t sy = (size_t)d.n[0], sz = (size_t)d.n[0] * (size_t)d.n[1];
    const size_t base = (size_t)c[0] + sy * (size_t)c[1] + sz * (size_t)c[2];
    float B[kProbeFloats - 1];
    for (int j = 0; j < kProbeFloats - 1; j++) B[j] = 0.0f;
    float W = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
        const float* p = sh + (base + (size_t)dx + (size_t)dy * sy + (size_t)dz * sz) * kProbeFloats;
        const float ux = dx ? w[0] : 1.0f - w[0], uy = dy ? w[1] : 1.0f - w[1], uz = dz ? w[2] : 1.0f - w[2];
        const float uxy = ux * uy;
        const float g0 = uxy * uz;
        const float g = p[kProbeFloats - 1] > 0.0f ? g0 : 0.0f;   // (a probe is valid iff n_used > 0)
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
