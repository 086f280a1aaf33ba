// rmr_probe.hip — irradiance probes (include/rmr.h rmr_bake_probes / rmr_probe_irradiance):
//   k_probe_rays<NP>      a ray source beside k_bake_rays: (probe, sample) -> the ray-source trace kernels'
//                         48-byte record, a uniform direction on the sphere from the probe itself; the buried
//                         test runs here, through the table-driven map class
//   k_probe_ray_list<NP>  the same rays as an rmr_ray list (rmr_probe_rays_device)
//   k_probe_fold<PAIR>    a launch's tile-samples projected onto nine basis functions and added to the probes'
//                         running state. PAIR: one thread per (probe, basis function),
//                         three channel sums each; a wave is 64 consecutive probes of one basis function, so the
//                         record and plane reads are the bake fold's coalesced ones, nine waves sharing them
//                         through the cache. !PAIR: one thread per probe, 27 sums (RMR_PROBE_FOLD_PER_PROBE
//                         makes it the default; the comparison is DESIGN.md §4.18's)
//   k_probe_lookup        one thread per query: the eight-corner gather of 28 floats each, the basis of the
//                         normal and the resolve
// The work of a probe bake is the light bake's 1-D image of points (rmr_bake.hip): a tile is 64 consecutive
// probes, tile t's sample k is tile-sample t nspp + k, a launch covers a run of tile-samples.
// Same float semantics as the trace kernels: -ffp-contract=off, hemisphere() and rand_step() of rmr_trace.h.
#include <hip/hip_runtime.h>
#include "rmr_probe_ray.h"

#ifndef RMR_PROBE_FOLD_PER_PROBE
#define RMR_PROBE_FOLD_PER_PROBE 0
#endif

namespace rmr {

// Records [0, 64 cnt) of a launch over tile-samples [s0, s0 + cnt), laid out as k_bake_rays lays them out:
// (o, time), (d, 0), (gx + time, gy + time, mark, 0). The padding of the last tile and every rejected or buried
// probe get the NaN mark ("no ray").
template <int NP>
__global__ __launch_bounds__(256) void k_probe_rays(KParams P, ProbeList B, uint64_t s0, uint32_t cnt, float4* rec,
                                                    unsigned long long* rejects) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    const bool in_launch = u < cnt * 64u;
    const uint64_t ts = s0 + (u >> 6);
    const uint64_t t = ts / B.nspp;
    const uint32_t k = (uint32_t)(ts - t * B.nspp);
    const uint64_t i = t * 64u + (u & 63u);
    const bool have = in_launch && i < B.n;
    ProbeRay r;
    const int why = have ? probe_ray<TableMap<NP>>(P, B, i, k, r) : kProbeBuried;
    note_probe_rejects(have && why == kProbeRejected && k == 0u, rejects);
    if (!in_launch) return;
    float4* q = rec + (size_t)u * kRayRecord;
    if (have && why == kProbeUsed) {
        q[0] = make_float4(r.o.x, r.o.y, r.o.z, r.time);
        q[1] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);   // the trace's own chain starts fresh as well
        q[2] = make_float4(r.gxt, r.gyt, 0.0f, 0.0f);
    } else {
        q[0] = q[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        q[2] = make_float4(0.0f, 0.0f, __builtin_nanf(""), 0.0f);
    }
}

// out[k][i] of every sample of every probe. A rejected or buried probe's rays: gx = -1 (no query accepts
// them), the sample's seed, everything else 0.
template <int NP>
__global__ __launch_bounds__(256) void k_probe_ray_list(KParams P, ProbeList B, rmr_ray* out, unsigned long long* rejects) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool have = g < B.n * B.nspp;
    const uint32_t k = (uint32_t)(g / B.n);
    const uint64_t i = g - (uint64_t)k * B.n;
    ProbeRay r;
    const int why = have ? probe_ray<TableMap<NP>>(P, B, i, k, r) : kProbeBuried;
    note_probe_rejects(have && why == kProbeRejected && k == 0u, rejects);
    if (!have) return;
    rmr_ray y{};
    y.time = r.time;
    y.gx = -1;
    if (why == kProbeUsed) {
        y.o[0] = r.o.x; y.o[1] = r.o.y; y.o[2] = r.o.z;
        y.d[0] = r.d.x; y.d[1] = r.d.y; y.d[2] = r.d.z;
        y.gx = r.gx;
        y.gy = r.gy;
    }
    out[g] = y;
}

// The fold of a launch over tile-samples [s0, s0 + cnt). PAIR: wave w of the launch takes probe tile
// s0 / nspp + w / 9 and basis function w % 9, its lane j probe i = 64 tile + j; !PAIR: wave w takes tile
// s0 / nspp + w and all nine. A probe's samples inside the launch are met in ascending k. A probe whose sample
// 0 is in the launch starts from zeros; one whose last sample is in it gets its result, and the others leave
// their sums in `state` for the next launch: a float4 per (probe, basis function), S.rgb and n_used, each pair
// carrying the count itself so that no thread reads what another writes. d and the mark come from the records,
// L from the trace's plane `samp`. A rejected or buried probe has no used sample: its result is 0.
template <bool PAIR>
__global__ __launch_bounds__(256) void k_probe_fold(const float4* samp, const float4* rec, float4* state, uint64_t n,
                                                    uint32_t nspp, uint64_t s0, uint32_t cnt, float* out) {
    constexpr int M = PAIR ? 1 : kProbeSH;
    const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6;
    const uint32_t m0 = PAIR ? w % (uint32_t)kProbeSH : 0u;
    const uint64_t t = s0 / nspp + (PAIR ? w / (uint32_t)kProbeSH : w);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = t * 64u + lane;
    const uint64_t t_begin = t * nspp, t_end = t_begin + nspp, s1 = s0 + cnt;
    if (i >= n || t_begin >= s1) return;
    const uint64_t a = t_begin > s0 ? t_begin : s0, b = t_end < s1 ? t_end : s1;
    float S[M][3];
    float n_used = 0.0f;
    float4* st = state + (size_t)i * kProbeSH + m0;
#pragma unroll
    for (int m = 0; m < M; m++) {
        const float4 v = a > t_begin ? st[m] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        S[m][0] = v.x; S[m][1] = v.y; S[m][2] = v.z;
        n_used = v.w;   // (the same count in every one of a probe's nine)
    }
    for (uint64_t ts = a; ts < b; ts++) {
        const size_t u = (size_t)(ts - s0) * 64u + lane;
        const float4 mk = rec[u * kRayRecord + 2];
        if (!(mk.z == mk.z)) continue;   // ("no ray": the trace stored nothing for the unit)
        const float4 L = samp[u];
        if (!probe_sample_used(L.x, L.y, L.z)) continue;
        const float4 d = rec[u * kRayRecord + 1];
        float Y[kProbeSH];
        sh_basis(d.x, d.y, d.z, Y);
        if (PAIR) {
            // (a select over registers: m0 is wave-uniform, the nine values are a few operations)
            float y = Y[0];
#pragma unroll
            for (int m = 1; m < kProbeSH; m++) y = m0 == (uint32_t)m ? Y[m] : y;
            probe_fold_one(S[0], L.x, L.y, L.z, y);
        } else {
#pragma unroll
            for (int m = 0; m < M; m++) probe_fold_one(S[m], L.x, L.y, L.z, Y[m]);
        }
        n_used = n_used + 1.0f;
    }
    if (b < t_end) {
#pragma unroll
        for (int m = 0; m < M; m++) st[m] = make_float4(S[m][0], S[m][1], S[m][2], n_used);
        return;
    }
    float* o = out + (size_t)i * kProbeFloats;
#pragma unroll
    for (int m = 0; m < M; m++)
        for (int c = 0; c < 3; c++) o[3 * (m0 + m) + c] = probe_resolve_one(S[m][c], n_used);
    if (m0 == 0u) o[kProbeFloats - 1] = n_used;
}

// One thread per query over the field sh[points of d][28]; a rejected query: (0, 0, 0, 0), counted.
__global__ __launch_bounds__(256) void k_probe_lookup(rmr_volume_desc d, const float* sh, const float* points,
                                                      const float* normals, uint64_t n, float* out,
                                                      unsigned long long* rejects) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool have = i < n;
    float q[3] = {0.0f, 0.0f, 0.0f}, nrm[3] = {0.0f, 0.0f, 0.0f};
    if (have)
        for (int a = 0; a < 3; a++) {
            q[a] = points[3 * i + a];
            nrm[a] = normals[3 * i + a];
        }
    const bool ok = have && bake_point_ok(q, nrm);
    note_probe_rejects(have && !ok, rejects);
    if (!have) return;
    float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ok) probe_lookup(d, sh, q, nrm, r);
    float* o = out + (size_t)i * 4;   // (any 4-byte alignment)
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3];
}

// P: the launch parameters of the context's scene and params; np: the scene's table-driven map class.
hipError_t launch_probe_rays(const KParams& P, int np, const ProbeList& B, uint64_t s0, uint32_t cnt, float4* rec,
                             unsigned long long* rejects, hipStream_t s) {
    if (cnt == 0) return hipSuccess;
    const unsigned g = (cnt * 64u + 255u) / 256u;
#define RMR_PROBE_RAYS_CALL(NPV) k_probe_rays<NPV><<<g, 256, 0, s>>>(P, B, s0, cnt, rec, rejects)
    RMR_PROBE_SWITCH(np, RMR_PROBE_RAYS_CALL);
#undef RMR_PROBE_RAYS_CALL
    return hipGetLastError();
}

hipError_t launch_probe_ray_list(const KParams& P, int np, const ProbeList& B, rmr_ray* out, unsigned long long* rejects,
                                 hipStream_t s) {
    const uint64_t total = B.n * B.nspp;
    if (total == 0) return hipSuccess;
    const unsigned g = (unsigned)((total + 255u) / 256u);
#define RMR_PROBE_LIST_CALL(NPV) k_probe_ray_list<NPV><<<g, 256, 0, s>>>(P, B, out, rejects)
    RMR_PROBE_SWITCH(np, RMR_PROBE_LIST_CALL);
#undef RMR_PROBE_LIST_CALL
    return hipGetLastError();
}

// mapping: 0 the build's default, 1 one thread per (probe, basis function), 2 one thread per probe
hipError_t launch_probe_fold(int mapping, const float4* samp, const float4* rec, float4* state, uint64_t n, uint32_t nspp,
                             uint64_t s0, uint32_t cnt, float* out, hipStream_t s) {
    if (cnt == 0) return hipSuccess;
    const uint64_t tiles = (s0 + cnt - 1) / nspp - s0 / nspp + 1;
    const bool pair = mapping == 0 ? !RMR_PROBE_FOLD_PER_PROBE : mapping == 1;
    const uint64_t waves = pair ? tiles * (uint64_t)kProbeSH : tiles;
    const unsigned g = (unsigned)((waves * 64u + 255u) / 256u);
    if (pair) k_probe_fold<true><<<g, 256, 0, s>>>(samp, rec, state, n, nspp, s0, cnt, out);
    else k_probe_fold<false><<<g, 256, 0, s>>>(samp, rec, state, n, nspp, s0, cnt, out);
    return hipGetLastError();
}

hipError_t launch_probe_lookup(const rmr_volume_desc& d, const float* sh, const float* points, const float* normals,
                               uint64_t n, float* out, unsigned long long* rejects, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_probe_lookup<<<(unsigned)((n + 255u) / 256u), 256, 0, s>>>(d, sh, points, normals, n, out, rejects);
    return hipGetLastError();
}

}  // namespace rmr
