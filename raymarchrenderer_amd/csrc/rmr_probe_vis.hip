// rmr_probe_vis.hip — the probes' visibility (include/rmr.h rmr_bake_probe_visibility / rmr_probe_irradiance_vis;
// DESIGN.md §4.19):
//   k_probe_vis_cast<NP>  one thread per (probe, sample) unit in the probe ray source's tile order: the
//                         position, the reject and buried tests and the direction through k_probe_rays' own
//                         function (rmr_probe_ray.h), then the cast's march (rmr_cast.h) over the table-driven
//                         map class, no normal probes; writes a 16-byte record (d.xyz, r)
//   k_probe_vis_fold      one wave per probe, lane j = texel j: the wave walks the probe's records of a launch
//                         in ascending k, eight fetched ahead of the sequential sums; A, M1, M2 per texel are
//                         carried between launches, the launch with a probe's last sample resolves
//   k_probe_lookup_vis    one thread per query: k_probe_lookup plus the per-corner weights, two floats
//                         gathered from each valid corner's map
// The work is the probe bake's 1-D image (rmr_probe.hip): a tile is 64 consecutive probes, tile t's sample k is
// tile-sample t nspp + k, a launch covers a run of tile-samples; unit u of a launch is record u.
// A record's fourth float: r >= 0, or NaN for a sample that is skipped (t not finite, the last tile's padding),
// or -1 for every sample of a probe that is not used (rejected, buried, not valid in the field).
// Same float semantics as the trace kernels: -ffp-contract=off.
#include <hip/hip_runtime.h>
#include "rmr_probe_ray.h"
#include "rmr_probe_vis_rule.h"

namespace rmr {

constexpr float kVisProbeUnused = -1.0f;
constexpr int kVisAhead = 8;   // records fetched ahead of the sums

// valid_sh: the field form's validity (probe i is used iff valid_sh[28 i + 27] > 0, and the buried test is not
// run), or nullptr for the list forms.
template <int NP>
__global__ __launch_bounds__(256) void k_probe_vis_cast(KParams P, ProbeList B, const float* valid_sh, float range,
                                                        uint64_t s0, uint32_t cnt, float4* rec,
                                                        unsigned long long* rejects) {
    using MAP = TableMap<NP>;
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    const bool in_launch = u < cnt * 64u;
    const uint64_t ts = s0 + (u >> 6);
    const uint64_t t = ts / B.nspp;
    const uint32_t k = (uint32_t)(ts - t * B.nspp);
    const uint64_t i = t * 64u + (u & 63u);
    const bool have = in_launch && i < B.n;
    const bool field = valid_sh != nullptr;
    const bool valid = have && (!field || valid_sh[(size_t)i * kProbeFloats + kProbeFloats - 1] > 0.0f);
    ProbeRay r;
    r.o = r.d = v3(0.0f, 0.0f, 0.0f);
    const int why = valid ? probe_ray<MAP>(P, B, i, k, r, !field) : kProbeBuried;
    note_probe_rejects(valid && why == kProbeRejected && k == 0u, rejects);
    const bool ok = valid && why == kProbeUsed;
    float tt, id;
    (void)march_first_hit<MAP>(P, ok, r.o, r.d, tt, id);   // (wave-uniform loop exits: every lane calls it)
    if (!in_launch) return;
    float rr = __builtin_nanf("");
    if (have && !ok) rr = kVisProbeUnused;
    if (ok && vis_sample_used(tt)) rr = vis_sample_r(tt, range);
    rec[u] = make_float4(r.d.x, r.d.y, r.d.z, rr);
}

// The fold of a launch over tile-samples [s0, s0 + cnt): wave w of the launch takes probe 64 (s0 / nspp) + w.
// state: [probe][3][64] floats; out: [probe][64][2].
__global__ __launch_bounds__(256) void k_probe_vis_fold(const float4* rec, float* state, uint64_t n, uint32_t nspp,
                                                        float range, uint64_t s0, uint32_t cnt, float* out) {
    const uint32_t w = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = s0 / nspp + (w >> 6);
    const uint32_t slot = w & 63u;
    const uint64_t i = t * 64u + slot;
    const uint64_t t_begin = t * nspp, t_end = t_begin + nspp, s1 = s0 + cnt;
    if (i >= n || t_begin >= s1) return;
    const uint64_t a = t_begin > s0 ? t_begin : s0, b = t_end < s1 ? t_end : s1;
    float D[3];
    vis_texel_dir((int)lane, D);
    float* st = state + (size_t)i * kVisStateFloats + lane;
    VisAcc S{0.0f, 0.0f, 0.0f};
    if (a > t_begin) {
        S.A = st[0];
        S.M1 = st[kVisTexels];
        S.M2 = st[2 * kVisTexels];
    }
    bool unused = false;
    const float4* q = rec + (size_t)(a - s0) * 64u + slot;   // (wave-uniform: one load per wave and record)
    const uint32_t steps = (uint32_t)(b - a);
    for (uint32_t k0 = 0; k0 < steps; k0 += (uint32_t)kVisAhead) {
        float4 v[kVisAhead];
#pragma unroll
        for (int j = 0; j < kVisAhead; j++)
            v[j] = k0 + (uint32_t)j < steps ? q[(size_t)(k0 + (uint32_t)j) * 64u] : make_float4(0.0f, 0.0f, 0.0f, __builtin_nanf(""));
#pragma unroll
        for (int j = 0; j < kVisAhead; j++) {
            unused = unused || v[j].w < 0.0f;
            if (v[j].w >= 0.0f) vis_fold_one(S, D, v[j].x, v[j].y, v[j].z, v[j].w);
        }
    }
    if (b < t_end) {
        st[0] = S.A;
        st[kVisTexels] = S.M1;
        st[2 * kVisTexels] = S.M2;
        return;
    }
    float m1, m2;
    vis_resolve(S, range, m1, m2);
    if (unused) m1 = m2 = 0.0f;
    float2* o = (float2*)(out + (size_t)i * kVisFloats) + lane;
    *o = make_float2(m1, m2);
}

// One thread per query over the field sh[points of d][28] and vis[points of d][128]; a rejected query:
// (0, 0, 0, 0), counted.
__global__ __launch_bounds__(256) void k_probe_lookup_vis(rmr_volume_desc d, const float* sh, const float* vis,
                                                          const float* points, const float* normals, uint64_t n,
                                                          float bias, float* out, unsigned long long* rejects) {
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
    if (ok) probe_lookup_vis(d, sh, vis, q, nrm, bias, r);
    float* o = out + (size_t)i * 4;   // (any 4-byte alignment)
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3];
}

// P: the launch parameters of the context's scene and params; np: the scene's table-driven map class.
hipError_t launch_probe_vis_cast(const KParams& P, int np, const ProbeList& B, const float* valid_sh, float range,
                                 uint64_t s0, uint32_t cnt, float4* rec, unsigned long long* rejects, hipStream_t s) {
    if (cnt == 0) return hipSuccess;
    const unsigned g = (cnt * 64u + 255u) / 256u;
#define RMR_PROBE_VIS_CAST_CALL(NPV) k_probe_vis_cast<NPV><<<g, 256, 0, s>>>(P, B, valid_sh, range, s0, cnt, rec, rejects)
    RMR_PROBE_SWITCH(np, RMR_PROBE_VIS_CAST_CALL);
#undef RMR_PROBE_VIS_CAST_CALL
    return hipGetLastError();
}

hipError_t launch_probe_vis_fold(const float4* rec, float* state, uint64_t n, uint32_t nspp, float range, uint64_t s0,
                                 uint32_t cnt, float* out, hipStream_t s) {
    if (cnt == 0) return hipSuccess;
    const uint64_t tiles = (s0 + cnt - 1) / nspp - s0 / nspp + 1;
    const unsigned g = (unsigned)((tiles * 64u * 64u + 255u) / 256u);
    k_probe_vis_fold<<<g, 256, 0, s>>>(rec, state, n, nspp, range, s0, cnt, out);
    return hipGetLastError();
}

hipError_t launch_probe_lookup_vis(const rmr_volume_desc& d, const float* sh, const float* vis, const float* points,
                                   const float* normals, uint64_t n, float bias, float* out, unsigned long long* rejects,
                                   hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_probe_lookup_vis<<<(unsigned)((n + 255u) / 256u), 256, 0, s>>>(d, sh, vis, points, normals, n, bias, out, rejects);
    return hipGetLastError();
}

}  // namespace rmr
