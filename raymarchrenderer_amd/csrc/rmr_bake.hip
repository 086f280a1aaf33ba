// rmr_bake.hip — light baking at surface points (include/rmr.h rmr_bake_points):
//   k_bake_rays      a third ray source beside k_camera_rays and k_pack_rays: (point, normal, sample) -> the
//                    ray-source trace kernels' 48-byte record (rmr_trace.h ray_record), with the sample's
//                    cosine in the record's spare word
//   k_bake_ray_list  the same rays as an rmr_ray list (rmr_bake_rays_device)
//   k_bake_ao<NP>    direction and march of one (point, sample) per thread through the table-driven map
//                    class, no record: (c, c v) into the launch's plane
//   k_bake_fold<AO>  one thread per point: its launch's samples in ascending k onto the point's running state
// The work of a bake is a 1-D image of points: a tile is 64 consecutive points, a sample is k, and tile t's
// sample k is "tile-sample" t nspp + k. A launch covers a run [s0, s0 + cnt) of tile-samples, 64 units each,
// so a cut may fall inside a point's sample set and inside the point list alike; each point still meets its
// samples in ascending k, launch after launch.
// Same float semantics as the trace kernels: -ffp-contract=off, hemisphere() and rand_step() of rmr_trace.h.
#include <hip/hip_runtime.h>
#include "rmr_cast.h"
#include "rmr_bake_rule.h"

static_assert(sizeof(rmr_ray) == 40, "rmr_ray is 40 bytes");

namespace rmr {

struct BakeRay {
    V3 o, d;
    float c, time, gxt, gyt;
    int32_t gx, gy;
};

// Sample k of point i: false for a rejected point (the rule's, or an origin beyond the caller's bound).
RMR_D bool bake_ray(const BakeList& B, uint64_t i, uint32_t k, BakeRay& r) {
    float p[3], n[3];
    for (int a = 0; a < 3; a++) {
        p[a] = B.points[3 * i + a];
        n[a] = B.normals[3 * i + a];
    }
    const uint64_t idx = B.first_index + i;
    r.gx = bake_gx(idx);
    r.gy = bake_gy(idx);
    r.time = B.times[k];
    r.gxt = (float)r.gx + r.time;
    r.gyt = (float)r.gy + r.time;
    if (!bake_point_ok(p, n)) return false;
    Lane L;
    L.gxt = r.gxt;
    L.gyt = r.gyt;
    L.rc = 0.0f;   // a fresh chain, started as main() starts a pixel's: its first jitter call. (From rc = 0 the
                   // co of randHemisphere's first rand(), (p.x, p.y), would not depend on the seed: every sample
                   // of a point would get the same theta)
    (void)lrand(L, v2(L.gxt, L.gyt));
    const bool deg = bake_degenerate(n);
    const V3 m = deg ? v3(0.0f, 1.0f, 0.0f) : v3(n[0], n[1], n[2]);
    V3 d = hemisphere(L, v2(p[0], p[1]), v2(p[2], p[0]), m);
    if (deg && n[1] < 0.0f) d.y = -d.y;
    float o[3];
    bake_origin(p, n, B.bias, o);
    for (int a = 0; a < 3; a++)
        if (!((o[a] < 0.0f ? -o[a] : o[a]) <= B.extent)) return false;   // (the escape bound's boxes assume the bound)
    const float dd[3] = {d.x, d.y, d.z};
    r.o = v3(o[0], o[1], o[2]);
    r.d = d;
    r.c = bake_cosine(n, dd);
    return true;
}

// A wave's rejected points, counted once per point (at its sample 0): one add per wave that saw one.
RMR_D void note_bake_rejects(bool rejected, unsigned long long* rejects) {
    const uint64_t rj = __ballot(rejected);
    if (rejects && rejected && (int)(threadIdx.x & 63u) == __ffsll((unsigned long long)rj) - 1)
        atomicAdd(rejects, (unsigned long long)__popcll(rj));
}

// Records [0, 64 cnt) of a launch over tile-samples [s0, s0 + cnt): (o, time), (d, 0), (gx + time, gy + time,
// mark, c). The padding of the last tile and every rejected point get the NaN mark ("no ray").
__global__ __launch_bounds__(256) void k_bake_rays(BakeList B, uint64_t s0, uint32_t cnt, float4* rec,
                                                   unsigned long long* rejects) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    const bool in_launch = u < cnt * 64u;
    const uint64_t ts = s0 + (u >> 6);
    const uint64_t t = ts / B.nspp;
    const uint32_t k = (uint32_t)(ts - t * B.nspp);
    const uint64_t i = t * 64u + (u & 63u);
    const bool have = in_launch && i < B.n;
    BakeRay r;
    const bool ok = have && bake_ray(B, i, k, r);
    note_bake_rejects(have && !ok && k == 0u, rejects);
    if (!in_launch) return;
    float4* q = rec + (size_t)u * kRayRecord;
    if (ok) {
        q[0] = make_float4(r.o.x, r.o.y, r.o.z, r.time);
        q[1] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);   // the trace's own chain starts fresh as well
        q[2] = make_float4(r.gxt, r.gyt, 0.0f, r.c);
    } else {
        q[0] = q[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        q[2] = make_float4(0.0f, 0.0f, __builtin_nanf(""), 0.0f);
    }
}

// out[k][i] of every sample of every point. A rejected point's rays: gx = -1 (no query accepts them), the
// sample's seed, everything else 0.
__global__ __launch_bounds__(256) void k_bake_ray_list(BakeList B, rmr_ray* out, unsigned long long* rejects) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool have = g < B.n * B.nspp;
    const uint32_t k = (uint32_t)(g / B.n);
    const uint64_t i = g - (uint64_t)k * B.n;
    BakeRay r;
    const bool ok = have && bake_ray(B, i, k, r);
    note_bake_rejects(have && !ok && k == 0u, rejects);
    if (!have) return;
    rmr_ray y{};
    y.time = r.time;
    y.gx = -1;
    if (ok) {
        y.o[0] = r.o.x; y.o[1] = r.o.y; y.o[2] = r.o.z;
        y.d[0] = r.d.x; y.d[1] = r.d.y; y.d[2] = r.d.z;
        y.gx = r.gx;
        y.gy = r.gy;
    }
    out[g] = y;
}

// (c, c v) of the launch's units into `plane`; a rejected point: (NaN, 0); padding is not written. One unit
// per thread, strided over the grid by whole waves (the march's loop exits are wave-uniform).
template <int NP>
__global__ __launch_bounds__(256) void k_bake_ao(KParams P, BakeList B, float ao_distance, uint64_t s0, uint32_t cnt,
                                                 float2* plane, unsigned long long* rejects) {
    using MAP = TableMap<NP>;
    const uint32_t units = cnt * 64u;
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; (u & ~63u) < units; u += stride) {
        const uint64_t ts = s0 + (u >> 6);
        const uint64_t t = ts / B.nspp;
        const uint32_t k = (uint32_t)(ts - t * B.nspp);
        const uint64_t i = t * 64u + (u & 63u);
        const bool have = i < B.n;
        BakeRay r;
        r.o = r.d = v3(0.0f, 0.0f, 0.0f);
        r.c = 0.0f;
        const bool ok = have && bake_ray(B, i, k, r);
        note_bake_rejects(have && !ok && k == 0u, rejects);
        float th, id;
        const bool is_hit = march_first_hit<MAP>(P, ok, r.o, r.d, th, id);
        const bool blocked = is_hit && th < ao_distance;
        if (have) plane[u] = ok ? make_float2(r.c, blocked ? 0.0f : r.c) : make_float2(__builtin_nanf(""), 0.0f);
    }
}

// The fold of a launch over tile-samples [s0, s0 + cnt): thread j of the launch's point tiles takes point
// i = 64 (s0 / nspp) + j and its tile-samples inside the launch in ascending k. A point whose sample 0 is in
// the launch starts from the initial state; one whose last sample is in it gets its result, and the others
// leave their state in `state` (float4 per point: S.rgb and n_used, or sum c, sum c v) for the next launch.
//   radiance: L from the trace's plane `samp`, c and the mark from the records; out_rgba[i] = (2 S / n_used, n_used)
//   AO:       (c, c v) from the plane, c NaN = a rejected point; out_ao[i] = sum c v / sum c
// A rejected point's result is 0 (alpha included).
template <bool AO>
__global__ __launch_bounds__(256) void k_bake_fold(const void* plane, const float4* rec, float4* state, uint64_t n,
                                                   uint32_t nspp, uint64_t s0, uint32_t cnt, float* out) {
    const uint64_t t = s0 / nspp + ((blockIdx.x * 256u + threadIdx.x) >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = t * 64u + lane;
    const uint64_t t_begin = t * nspp, t_end = t_begin + nspp, s1 = s0 + cnt;
    if (i >= n || t_begin >= s1) return;
    const uint64_t a = t_begin > s0 ? t_begin : s0, b = t_end < s1 ? t_end : s1;
    BakeState st;
    bake_state_init(st);
    if (a > t_begin) {
        const float4 v = state[i];
        if (AO) { st.sum_c = v.x; st.sum_cv = v.y; }
        else { st.s[0] = v.x; st.s[1] = v.y; st.s[2] = v.z; st.n_used = v.w; }
    }
    bool rejected = false;
    for (uint64_t ts = a; ts < b; ts++) {
        const size_t u = (size_t)(ts - s0) * 64u + lane;
        if (AO) {
            const float2 cv = ((const float2*)plane)[u];
            if (cv.x == cv.x) bake_fold_ao(st, cv.x, cv.y);
            else rejected = true;
        } else {
            const float4 m = rec[u * kRayRecord + 2];
            if (m.z == m.z) {
                const float4 L = ((const float4*)plane)[u];
                bake_fold_radiance(st, L.x, L.y, L.z, m.w);
            } else {
                rejected = true;   // ("no ray": the trace stored nothing for the unit)
            }
        }
    }
    if (b < t_end) {
        state[i] = AO ? make_float4(st.sum_c, st.sum_cv, 0.0f, 0.0f) : make_float4(st.s[0], st.s[1], st.s[2], st.n_used);
        return;
    }
    if (AO) {
        out[i] = rejected ? 0.0f : bake_resolve_ao(st);
    } else {
        float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!rejected) bake_resolve_radiance(st, r);
        float* o = out + (size_t)i * 4;
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3];
    }
}

#define RMR_BAKE_SWITCH(NPV, CALL)       \
    switch (NPV) {                       \
    case 4: CALL(4); break;              \
    case 8: CALL(8); break;              \
    case 0: CALL(0); break;              \
    case -2: CALL(-2); break;            \
    default: CALL(-1); break;            \
    }

hipError_t launch_bake_rays(const BakeList& B, uint64_t s0, uint32_t cnt, float4* rec, unsigned long long* rejects,
                            hipStream_t s) {
    if (cnt == 0) return hipSuccess;
    k_bake_rays<<<(cnt * 64u + 255u) / 256u, 256, 0, s>>>(B, s0, cnt, rec, rejects);
    return hipGetLastError();
}

hipError_t launch_bake_ray_list(const BakeList& B, rmr_ray* out, unsigned long long* rejects, hipStream_t s) {
    const uint64_t total = B.n * B.nspp;
    if (total == 0) return hipSuccess;
    k_bake_ray_list<<<(unsigned)((total + 255u) / 256u), 256, 0, s>>>(B, out, rejects);
    return hipGetLastError();
}

// P: the launch parameters of the context's scene and params; np: the scene's table-driven map class;
// grid_cap: rmr_set_query_grid (0: one thread per unit).
hipError_t launch_bake_ao(const KParams& P, int np, const BakeList& B, float ao_distance, uint64_t s0, uint32_t cnt,
                          float2* plane, unsigned long long* rejects, int grid_cap, hipStream_t s) {
    if (cnt == 0) return hipSuccess;
    unsigned g = (cnt * 64u + 255u) / 256u;
    if (grid_cap > 0 && g > (unsigned)grid_cap) g = (unsigned)grid_cap;
#define RMR_BAKE_AO_CALL(NPV) k_bake_ao<NPV><<<g, 256, 0, s>>>(P, B, ao_distance, s0, cnt, plane, rejects)
    RMR_BAKE_SWITCH(np, RMR_BAKE_AO_CALL);
#undef RMR_BAKE_AO_CALL
    return hipGetLastError();
}

hipError_t launch_bake_fold(bool ao, const void* plane, const float4* rec, float4* state, uint64_t n, uint32_t nspp,
                            uint64_t s0, uint32_t cnt, float* out, hipStream_t s) {
    if (cnt == 0) return hipSuccess;
    const uint64_t tiles = (s0 + cnt - 1) / nspp - s0 / nspp + 1;
    const unsigned g = (unsigned)((tiles * 64u + 255u) / 256u);
    if (ao) k_bake_fold<true><<<g, 256, 0, s>>>(plane, rec, state, n, nspp, s0, cnt, out);
    else k_bake_fold<false><<<g, 256, 0, s>>>(plane, rec, state, n, nspp, s0, cnt, out);
    return hipGetLastError();
}

}  // namespace rmr
