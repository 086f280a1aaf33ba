// rmr_camera.hip — k_camera_rays: the ray records of a launch's units for the context's camera model
// (include/rmr.h rmr_camera_model states each model operation by operation; camera_ray of rmr_camera_ray.h is
// that statement, shared with rmr_aov.hip).
// One thread per unit, in the sample planes' [nspp][n_tiles][64] order; the ray-source trace kernels
// (rmr_trace.h RAYS, rmr_trace_rays.hip) read the records back. Same float semantics as the trace
// kernels: -ffp-contract=off, sqrt_cr, det_sin / det_cos, rand_step for every random number.
#include <hip/hip_runtime.h>
#include "rmr_camera_ray.h"

namespace rmr {

static_assert(kRayRecord * sizeof(float4) == kRayRecordBytes, "the host sizes the ray buffer with kRayRecordBytes");

__global__ __launch_bounds__(256) void k_camera_rays(KParams P, CamParams C, float4* rays) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n_units) return;
    const uint32_t un = (uint32_t)i;
    float4* rec = rays + (size_t)un * kRayRecord;
    int px, py;
    float time;
    if (!unit_pixel(P, un, px, py, time)) {   // no ray: the NaN mark (rmr_trace.h ray_record)
        rec[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        rec[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        rec[2] = make_float4(0.0f, 0.0f, __builtin_nanf(""), 0.0f);
        return;
    }
    const float gxt = (float)px + time, gyt = (float)py + time;
    V3 o, d;
    float rc;
    camera_ray(P, C, px, py, time, o, d, rc);
    rec[0] = make_float4(o.x, o.y, o.z, time);
    rec[1] = make_float4(d.x, d.y, d.z, rc);
    rec[2] = make_float4(gxt, gyt, 0.0f, 0.0f);
}

hipError_t launch_camera_rays(const KParams& P, const CamParams& C, float4* rays, hipStream_t s) {
    k_camera_rays<<<(unsigned)((P.n_units + 255) / 256), 256, 0, s>>>(P, C, rays);
    return hipGetLastError();
}

}  // namespace rmr
