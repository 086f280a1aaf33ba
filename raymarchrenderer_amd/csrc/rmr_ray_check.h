// rmr_ray_check.h — the rule a caller's ray must pass (include/rmr.h rmr_check_rays), written once for
// the host (camera.cpp first_bad_ray) and the device (rmr_query.hip: the device forms of the queries
// cannot validate on the host, so the kernels apply it and mark what fails as rejected).
// Plain C++ and HIP: no library call, so both sides run the same operations.
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif
#include "../../include/rmr.h"

#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define RMR_HD __host__ __device__ inline
#else
#define RMR_HD inline
#endif

namespace rmr {

RMR_HD bool finite_f(float x) { return __builtin_isfinite(x); }

// every float finite, |d.d - 1| <= 1e-5 and 0 <= gx, gy < 2^24. The length test is in double, each
// product and sum rounded on its own (contraction off: a fused d.d would move the verdict of a ray at
// the bound between the host and the device)
RMR_HD bool ray_ok(const rmr_ray& r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    bool ok = finite_f(r.time) && finite_f(r.rc);
    for (int k = 0; k < 3; k++) ok = ok && finite_f(r.o[k]) && finite_f(r.d[k]);
    const double x = (double)r.d[0], y = (double)r.d[1], z = (double)r.d[2];
    const double xx = x * x, yy = y * y, zz = z * z;
    const double dd = (xx + yy) + zz;
    const double e = dd - 1.0;
    ok = ok && (e < 0.0 ? -e : e) <= 1e-5;
    ok = ok && r.gx >= 0 && r.gy >= 0 && r.gx < (1 << 24) && r.gy < (1 << 24);
    return ok;
}

// rmr_trace_rays_device's origin_extent: a finite, non-negative bound ...
RMR_HD bool extent_ok(float extent) { return finite_f(extent) && extent >= 0.0f; }
// ... that no origin coordinate exceeds (|o_k| == extent is inside; a NaN coordinate is outside)
RMR_HD bool origin_within(const rmr_ray& r, float extent) {
    bool in = true;
    for (int k = 0; k < 3; k++) in = in && (r.o[k] < 0.0f ? -r.o[k] : r.o[k]) <= extent;
    return in;
}

}  // namespace rmr
