// rmr_trace_rays.hip — the ahead-of-time ray-source trace kernels k_trace_rays<VARIANT, NP, PERSIST,
// PROG>: rmr_kernels.hip's k_trace with the primary rays read from a device ray buffer (rmr_trace.h
// RAYS; the buffer is the second kernel argument, KParams is unchanged), and their host launchers.
// Camera models other than the view's own and rmr_trace_rays run these (rmr_api.cpp render_tiles).
#include <hip/hip_runtime.h>
#include "rmr_trace.h"

namespace rmr {

template <int VAR, int NP, bool PERSIST, bool PROG>
__global__ __launch_bounds__(256, (trace_waves<VAR, (NP == -1), PROG>())) void k_trace_rays(KParams P, const float4* rays) {
    trace_main<VAR, TableMap<NP>, PERSIST, PROG, TableMats, true>(P, rays);
}

#define RMR_RAYS_SWITCH(V, NPV, PERS, PRG, CALL)         \
    switch (NPV) {                                          \
    case 4: CALL(V, 4, PERS, PRG); break;                   \
    case 8: CALL(V, 8, PERS, PRG); break;                   \
    case 0: CALL(V, 0, PERS, PRG); break;                   \
    case -2: CALL(V, -2, PERS, PRG); break;                 \
    default: CALL(V, -1, PERS, PRG); break;                 \
    }
#define RMR_LAUNCH_RAYS(V, NPV, PERS, PRG) k_trace_rays<V, NPV, PERS, PRG><<<g, block, 0, s>>>(P, rays)

hipError_t launch_trace_rays(const KParams& P, const float4* rays, int variant, int np, bool prog, bool persistent,
                             int grid, hipStream_t s) {
    dim3 block(256);
    unsigned g = (unsigned)grid;
    if (persistent) {
        switch (variant) {
        case RMR_VARIANT_RM1:
            if (prog) { RMR_RAYS_SWITCH(RMR_VARIANT_RM1, np, true, true, RMR_LAUNCH_RAYS); }
            else { RMR_RAYS_SWITCH(RMR_VARIANT_RM1, np, true, false, RMR_LAUNCH_RAYS); }
            break;
        case RMR_VARIANT_RM2: RMR_RAYS_SWITCH(RMR_VARIANT_RM2, np, true, false, RMR_LAUNCH_RAYS); break;
        default: RMR_RAYS_SWITCH(RMR_VARIANT_RM3, np, true, false, RMR_LAUNCH_RAYS); break;
        }
    } else {
        g = (unsigned)((P.n_units + 255) / 256);
        switch (variant) {
        case RMR_VARIANT_RM1: RMR_LAUNCH_RAYS(RMR_VARIANT_RM1, -1, false, true); break;
        case RMR_VARIANT_RM2: RMR_LAUNCH_RAYS(RMR_VARIANT_RM2, -1, false, false); break;
        default: RMR_LAUNCH_RAYS(RMR_VARIANT_RM3, -1, false, false); break;
        }
    }
    return hipGetLastError();
}
#define RMR_OCC_RAYS(V, NPV, PERS, PRG) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_trace_rays<V, NPV, PERS, PRG>, 256, 0)
int trace_rays_occupancy(int variant, int np, bool prog, int* blocks_per_cu) {
    int b = 0;
    hipError_t e = hipSuccess;
    switch (variant) {
    case RMR_VARIANT_RM1:
        if (prog) { RMR_RAYS_SWITCH(RMR_VARIANT_RM1, np, true, true, RMR_OCC_RAYS); }
        else { RMR_RAYS_SWITCH(RMR_VARIANT_RM1, np, true, false, RMR_OCC_RAYS); }
        break;
    case RMR_VARIANT_RM2: RMR_RAYS_SWITCH(RMR_VARIANT_RM2, np, true, false, RMR_OCC_RAYS); break;
    default: RMR_RAYS_SWITCH(RMR_VARIANT_RM3, np, true, false, RMR_OCC_RAYS); break;
    }
    *blocks_per_cu = b;
    return e == hipSuccess ? 0 : -1;
}
}  // namespace rmr
