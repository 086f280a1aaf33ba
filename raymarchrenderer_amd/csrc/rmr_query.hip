// rmr_query.hip — geometry queries for a caller's rays and points, and the device-resident ray list
// (include/rmr.h "first-hit and distance queries"):
//   k_cast_rays<NP, NORMALS>  march() and getNormal of rmr_guides.hip's k_guides with the ray's origin
//                             where the guide pass has the eye: rmr_ray in, rmr_hit out, no records
//   k_eval_map<NP>            map(p) of a point list
//   k_pack_rays               rmr_ray (40 B) -> the ray-source kernels' 48-byte record (rmr_trace.h
//                             ray_record), validated on the GPU (rmr_ray_check.h)
//   k_unpack_rgba             a launch's sample planes -> the caller's RGBA buffer
// Like the guide pass: the scene's table-driven map class, no RNG, no escape bound, no approximate map,
// so every class gives the oracle's march / getNormal / map bits.
#include <hip/hip_runtime.h>
#include "rmr_cast.h"
#include "rmr_ray_check.h"

static_assert(sizeof(rmr_hit) == 32, "rmr_hit is the guide planes' HIT and NORMAL of one ray: 32 bytes");
static_assert(sizeof(rmr_ray) == 40, "rmr_ray is 40 bytes");

namespace rmr {

// A wave's rejected rays: one add per wave that saw one (by its first rejected lane, whose index is the
// wave's smallest), and the list's first rejected index (the host forms name it in their error).
RMR_D void note_rejects(bool rejected, uint64_t i, unsigned long long* rejects, unsigned long long* first_bad) {
    const uint64_t rj = __ballot(rejected);
    if (rejected && (int)(threadIdx.x & 63u) == __ffsll((unsigned long long)rj) - 1) {
        atomicAdd(rejects, (unsigned long long)__popcll(rj));
        atomicMin(first_bad, (unsigned long long)i);
    }
}

RMR_D void store_rejected(rmr_hit* out) {
    rmr_hit h;
    h.pos[0] = h.pos[1] = h.pos[2] = 0.0f;
    h.t = -1.0f;
    h.n[0] = h.n[1] = h.n[2] = 0.0f;
    h.id = -2.0f;
    *out = h;
}

// One ray per thread, strided over the grid by whole waves (a wave's trip count is uniform). A ray the
// rule rejects gets (0, 0, 0, -1, 0, 0, 0, -2) and is counted.
template <int NP, bool NORMALS>
__global__ __launch_bounds__(256) void k_cast_rays(KParams P, const rmr_ray* rays, uint64_t n, rmr_hit* out,
                                                   unsigned long long* rejects, unsigned long long* first_bad) {
    using MAP = TableMap<NP>;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint64_t i = base + lane;
        const bool have = i < n;
        rmr_ray r{};
        if (have) r = rays[i];
        const bool ok = have && ray_ok(r);
        note_rejects(have && !ok, i, rejects, first_bad);
        const V3 o = v3(r.o[0], r.o[1], r.o[2]), dir = v3(r.d[0], r.d[1], r.d[2]);

        float t, id;
        const bool is_hit = march_first_hit<MAP>(P, ok, o, dir, t, id);
        const V3 pos = vfma(dir, t, o);
        V3 nn = v3(0.0f, 0.0f, 0.0f);
        if constexpr (NORMALS) nn = hit_normal<MAP>(P, is_hit, pos);
        if (ok) {
            rmr_hit h;
            h.pos[0] = pos.x; h.pos[1] = pos.y; h.pos[2] = pos.z; h.t = t;
            h.n[0] = nn.x; h.n[1] = nn.y; h.n[2] = nn.z; h.id = id;
            out[i] = h;
        } else if (have) {
            store_rejected(out + i);
        }
    }
}

// map(p) of each point as (distance, id): 12 bytes in, 8 bytes out, straight from and to the caller's
// buffers. Points are not checked.
struct F3 { float x, y, z; };
struct F2 { float x, y; };
template <int NP>
__global__ __launch_bounds__(256) void k_eval_map(KParams P, const F3* xyz, uint64_t n, F2* out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
        const F3 p = xyz[i];
        const V2 m = TableMap<NP>::eval(P, v3(p.x, p.y, p.z));
        out[i] = F2{m.x, m.y};
    }
}

// Records [0, units) of a launch from list rays [u0, u0 + units): (o, time), (d, rc), (gx + time,
// gy + time, mark, 0). The padding of the last tile (u0 + k >= n) and every rejected ray get the NaN
// mark ("no ray"); rejected: the rule of rmr_ray_check.h, or an origin beyond `extent`.
__global__ __launch_bounds__(256) void k_pack_rays(const rmr_ray* rays, uint64_t n, uint64_t u0, uint32_t units,
                                                   float extent, float4* rec, unsigned long long* rejects,
                                                   unsigned long long* first_bad) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const bool in_launch = k < units;
    const uint64_t i = u0 + k;
    const bool have = in_launch && i < n;
    rmr_ray r{};
    if (have) r = rays[i];
    const bool ok = have && ray_ok(r) && origin_within(r, extent);
    note_rejects(have && !ok, i, rejects, first_bad);
    if (!in_launch) return;
    float4* q = rec + (size_t)k * kRayRecord;
    if (ok) {
        q[0] = make_float4(r.o[0], r.o[1], r.o[2], r.time);
        q[1] = make_float4(r.d[0], r.d[1], r.d[2], r.rc);
        q[2] = make_float4((float)r.gx + r.time, (float)r.gy + r.time, 0.0f, 0.0f);   // gid + time, one rounding
    } else {
        q[0] = q[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        q[2] = make_float4(0.0f, 0.0f, __builtin_nanf(""), 0.0f);
    }
}

// The planes of a launch's first cnt units to the caller's buffer. A "no ray" unit stored nothing (its
// plane slot is stale), so a rejected ray's result is written here: (0, 0, 0, 0).
__global__ __launch_bounds__(256) void k_unpack_rgba(const float4* samp, const float4* rec, float* out, uint32_t cnt) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= cnt) return;
    const float mark = rec[(size_t)k * kRayRecord + 2].z;
    const float4 v = (mark == mark) ? samp[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float* o = out + (size_t)k * 4;
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}

namespace {
unsigned query_grid(uint64_t n, int cap) {
    const uint64_t blocks = std::max<uint64_t>(1, (n + 255) / 256);
    const uint64_t lim = cap > 0 ? (uint64_t)cap : (uint64_t)0x7fffffff;
    return (unsigned)std::min(blocks, lim);
}
}  // namespace

#define RMR_QUERY_SWITCH(NPV, CALL)      \
    switch (NPV) {                       \
    case 4: CALL(4); break;              \
    case 8: CALL(8); break;              \
    case 0: CALL(0); break;              \
    case -2: CALL(-2); break;            \
    default: CALL(-1); break;            \
    }

// P: the launch parameters of the context's scene and params; np: the scene's table-driven map class;
// grid_cap: rmr_set_query_grid (0: one thread per ray / point).
hipError_t launch_cast_rays(const KParams& P, int np, bool normals, const rmr_ray* rays, uint64_t n, rmr_hit* out,
                            unsigned long long* rejects, unsigned long long* first_bad, int grid_cap, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned g = query_grid(n, grid_cap);
#define RMR_CAST(NPV)                                                                              \
    if (normals) k_cast_rays<NPV, true><<<g, 256, 0, s>>>(P, rays, n, out, rejects, first_bad);   \
    else k_cast_rays<NPV, false><<<g, 256, 0, s>>>(P, rays, n, out, rejects, first_bad)
    RMR_QUERY_SWITCH(np, RMR_CAST);
#undef RMR_CAST
    return hipGetLastError();
}

hipError_t launch_eval_map(const KParams& P, int np, const float* xyz, uint64_t n, float* out, int grid_cap, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned g = query_grid(n, grid_cap);
#define RMR_EVAL(NPV) k_eval_map<NPV><<<g, 256, 0, s>>>(P, (const F3*)xyz, n, (F2*)out)
    RMR_QUERY_SWITCH(np, RMR_EVAL);
#undef RMR_EVAL
    return hipGetLastError();
}

hipError_t launch_pack_rays(const rmr_ray* rays, uint64_t n, uint64_t u0, uint32_t units, float extent, float4* rec,
                            unsigned long long* rejects, unsigned long long* first_bad, hipStream_t s) {
    if (units == 0) return hipSuccess;
    k_pack_rays<<<(units + 255u) / 256u, 256, 0, s>>>(rays, n, u0, units, extent, rec, rejects, first_bad);
    return hipGetLastError();
}

hipError_t launch_unpack_rgba(const float4* samp, const float4* rec, float* out, uint32_t cnt, hipStream_t s) {
    if (cnt == 0) return hipSuccess;
    k_unpack_rgba<<<(cnt + 255u) / 256u, 256, 0, s>>>(samp, rec, out, cnt);
    return hipGetLastError();
}

}  // namespace rmr
