// rmr_aov.hip — sampled AOVs (rmr_render_aov): per pixel, the first hits of the beauty
// samples' own primary rays folded into coverage, depth, normal, position and material-id mattes.
//   k_aov<NP>       one thread per pixel of the rect: the pixel's state from memory, then per sample the
//                   camera model's ray (rmr_camera_ray.h, k_camera_rays' statement), march and getNormal
//                   (rmr_cast.h, k_cast_rays' statement) and the rule's fold (rmr_aov_rule.h), in sample
//                   order; the state back to memory once. No atomics, no LDS, no buffer of hit records.
//   k_aov_resolve   the rule's resolve, one thread per pixel
//   k_aov_init      the initial state
// Like the guide pass and the queries: the scene's table-driven map class, no escape bound, no approximate
// map, so every class gives the oracle's bits.
#include <hip/hip_runtime.h>
#include "rmr_aov_rule.h"
#include "rmr_camera_ray.h"
#include "rmr_cast.h"

static_assert(sizeof(rmr::AovState) == 80, "the sampled AOVs' state is five float4 per pixel");
static_assert(sizeof(rmr::Aov4) == sizeof(float4), "a state plane is a float4 plane");

namespace rmr {

namespace {
RMR_D Aov4 ld4(const float4* p) {
    const float4 v = *p;
    return Aov4{v.x, v.y, v.z, v.w};
}
RMR_D void st4(float4* p, const Aov4& v) { *p = make_float4(v.x, v.y, v.z, v.w); }
}  // namespace

// A wave = one 8x8 tile of the rect's tile grid, as in k_guides, so a wave's rays stay coherent. state: the
// five planes, W x H float4 each, one after the other. Touches only pixels inside [x0, x1) x [y0, y1).
// restart: the rect's pixels start from the initial state instead of what memory holds.
template <int NP>
__global__ __launch_bounds__(256) void k_aov(KParams P, CamParams C, float4* state, int restart) {
    using MAP = TableMap<NP>;
    const int tx0 = P.x0 & ~7, ty0 = P.y0 & ~7;
    const int ntx = (P.x1 - tx0 + 7) >> 3, nty = (P.y1 - ty0 + 7) >> 3;
    const int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (tile >= ntx * nty) return;   // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    const int px = tx0 + 8 * (tile % ntx) + (lane & 7);
    const int py = ty0 + 8 * (tile / ntx) + (lane >> 3);
    const bool valid = !(px < P.x0 || py < P.y0 || px >= P.x1 || py >= P.y1);
    const size_t plane = (size_t)P.W * (size_t)P.H;
    float4* sp = state + ((size_t)py * (size_t)P.W + (size_t)px);   // (dereferenced by valid lanes only)

    AovState S = aov_initial();
    if (valid && !restart) {
        S.stats = ld4(sp);
        S.nrm = ld4(sp + plane);
        S.pos = ld4(sp + 2 * plane);
        S.ids01 = ld4(sp + 3 * plane);
        S.ids23 = ld4(sp + 4 * plane);
    }
#pragma unroll 1
    for (uint32_t k = 0; k < P.nspp; k++) {
        const float time = P.nspp == 1u ? P.time1 : P.times[k];
        V3 o, d;
        float rc;
        camera_ray(P, C, px, py, time, o, d, rc);
        float t, id;
        const bool is_hit = march_first_hit<MAP>(P, valid, o, d, t, id);
        const V3 pos = vfma(d, t, o);
        const V3 n = hit_normal<MAP>(P, is_hit, pos);
        if (valid) aov_fold1(S, pos.x, pos.y, pos.z, t, n.x, n.y, n.z, id);
    }
    if (valid) {
        st4(sp, S.stats);
        st4(sp + plane, S.nrm);
        st4(sp + 2 * plane, S.pos);
        st4(sp + 3 * plane, S.ids01);
        st4(sp + 4 * plane, S.ids23);
    }
}

__global__ __launch_bounds__(256) void k_aov_init(float4* state, size_t n_px) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_px) return;
    const AovState S = aov_initial();
    st4(state + i, S.stats);
    st4(state + n_px + i, S.nrm);
    st4(state + 2 * n_px + i, S.pos);
    st4(state + 3 * n_px + i, S.ids01);
    st4(state + 4 * n_px + i, S.ids23);
}

__global__ __launch_bounds__(256) void k_aov_resolve(const float4* state, size_t n_px, float max_dist, float4* out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_px) return;
    AovState S;
    S.stats = ld4(state + i);
    S.nrm = ld4(state + n_px + i);
    S.pos = ld4(state + 2 * n_px + i);
    S.ids01 = ld4(state + 3 * n_px + i);
    S.ids23 = ld4(state + 4 * n_px + i);
    const AovResolved R = aov_resolve1(S, max_dist);
    st4(out + i, R.depth);
    st4(out + n_px + i, R.nrm);
    st4(out + 2 * n_px + i, R.pos);
    st4(out + 3 * n_px + i, R.ids01);
    st4(out + 4 * n_px + i, R.ids23);
}

// P: the launch parameters of the context's scene and view with the rect in x0..y1 (already clamped to the
// image and non-empty), the launch's samples in nspp / times / time1; np: the scene's table-driven map class.
hipError_t launch_aov(const KParams& P, const CamParams& C, int np, float4* state, bool restart, hipStream_t s) {
    const int tx0 = P.x0 & ~7, ty0 = P.y0 & ~7;
    const long long tiles = (long long)((P.x1 - tx0 + 7) >> 3) * ((P.y1 - ty0 + 7) >> 3);
    const unsigned g = (unsigned)((tiles + 3) / 4);
    const int rs = restart ? 1 : 0;
    switch (np) {
    case 4: k_aov<4><<<g, 256, 0, s>>>(P, C, state, rs); break;
    case 8: k_aov<8><<<g, 256, 0, s>>>(P, C, state, rs); break;
    case 0: k_aov<0><<<g, 256, 0, s>>>(P, C, state, rs); break;
    case -2: k_aov<-2><<<g, 256, 0, s>>>(P, C, state, rs); break;
    default: k_aov<-1><<<g, 256, 0, s>>>(P, C, state, rs); break;
    }
    return hipGetLastError();
}

hipError_t launch_aov_init(float4* state, size_t n_px, hipStream_t s) {
    k_aov_init<<<(unsigned)((n_px + 255) / 256), 256, 0, s>>>(state, n_px);
    return hipGetLastError();
}

hipError_t launch_aov_resolve(const float4* state, size_t n_px, float max_dist, float4* out, hipStream_t s) {
    k_aov_resolve<<<(unsigned)((n_px + 255) / 256), 256, 0, s>>>(state, n_px, max_dist, out);
    return hipGetLastError();
}

}  // namespace rmr
