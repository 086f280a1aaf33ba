// rmr_atrous.h — device functions the a-trous passes share (rmr_denoise.hip, rmr_denoise_var.hip): the
// liveness test, the guide weight of a tap, the B3-spline kernel and the weighted sum. Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include "rmr_internal.h"

namespace rmr {
namespace {

__device__ __forceinline__ bool live(float4 c, float4 n) {
    return n.w >= 0.0f && c.w != 0.0f && __builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z);
}

// 1 / (sigma_z step max(t_p, FLT_MIN)) of a live centre, kept finite: a zero distance then weighs
// exp(-0 x FLT_MAX) = 1 and any other exp(-inf) = 0, as the unbounded quotient would
__device__ __forceinline__ float inv_depth_scale(const DenoisePass& A, float4 hp) {
    return fminf(1.0f / (A.sigma_z_step * fmaxf(hp.w, FLT_MIN)), FLT_MAX);
}

// w_q of a tap q != p whose pixel is live and on the image (the callers zero every other tap);
// products are fused where the statement leaves the rounding open (the library builds with
// -ffp-contract=off, so only these explicit fmaf fuse)
__device__ __forceinline__ float tap_weight(const DenoisePass& A, float4 cp, float4 hp, float4 np, float inv_z,
                                            float4 cq, float4 hq, float4 nq) {
    float w = fmaxf(0.0f, fmaf(np.x, nq.x, fmaf(np.y, nq.y, np.z * nq.z)));
    for (int k = 0; k < A.normal_pow2; k++) w *= w;
    const float dz = fabsf(fmaf(np.x, hq.x - hp.x, fmaf(np.y, hq.y - hp.y, np.z * (hq.z - hp.z))));
    w *= __expf(-dz * inv_z);
    if (A.inv_sigma_c2 > 0.0f) {   // (uniform)
        const float dx = cq.x - cp.x, dy = cq.y - cp.y, dw = cq.z - cp.z;
        w *= __expf(-fmaf(dx, dx, fmaf(dy, dy, dw * dw)) * A.inv_sigma_c2);
    }
    return nq.w == np.w ? w : 0.0f;
}

__device__ __forceinline__ float kern(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

struct Acc { float r, g, b, w; };
// c finite (a live tap, or one staged as zeros)
__device__ __forceinline__ void add_tap(Acc& s, float kw, float4 c) {
    s.r = fmaf(kw, c.x, s.r); s.g = fmaf(kw, c.y, s.g); s.b = fmaf(kw, c.z, s.b); s.w += kw;
}

}  // namespace
}  // namespace rmr
