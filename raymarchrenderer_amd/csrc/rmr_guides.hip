// rmr_guides.hip — first-hit guide pass (rmr_render_guides): one deterministic
// pixel-centre primary ray per pixel, marched with the reference's march() (RM1:233-257) through the
// table-driven map class the context selected for the scene, then getNormal (RM1:259-268) at the hit.
// No RNG, no escape bound, no approximate map: every map class gives the same bits, so the planes are
// checkable against the oracle's march / getNormal bit for bit.
#include <hip/hip_runtime.h>
#include "rmr_trace.h"

namespace rmr {

// One thread per pixel over the rect's 8x8 tiles (a wave = one tile, as the trace kernel's units).
// Planes (W x H float4, row 0 = top): ray = (dir, 0); hit = (fma(dir, t, eye), t); nrm = (normal, id)
// for a hit (t < maxDist), (0, 0, 0, -1) otherwise. Writes only inside [x0, x1) x [y0, y1).
template <int NP>
__global__ __launch_bounds__(256) void k_guides(KParams P, float4* ray, float4* hit, float4* nrm) {
    using MAP = TableMap<NP>;
    const int tx0 = P.x0 & ~7, ty0 = P.y0 & ~7;
    const int ntx = (P.x1 - tx0 + 7) >> 3, nty = (P.y1 - ty0 + 7) >> 3;
    const int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (tile >= ntx * nty) return;   // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    const int px = tx0 + 8 * (tile % ntx) + (lane & 7);
    const int py = ty0 + 8 * (tile / ntx) + (lane >> 3);
    const bool valid = !(px < P.x0 || py < P.y0 || px >= P.x1 || py >= P.y1);

    // main()'s corner-ray interpolation (primary_dir) with 0.5 for each of its three rand() results
    const float W = P.Wf, H = P.Hf;
    const float u = (float)px / W + 0.5f / W;
    const float v = (float)py / H + 0.5f / H;
    const V3 r00 = v3(P.r00[0], P.r00[1], P.r00[2]), r10 = v3(P.r10[0], P.r10[1], P.r10[2]);
    const V3 d0 = v3(P.dr01[0], P.dr01[1], P.dr01[2]), d1 = v3(P.dr11[0], P.dr11[1], P.dr11[2]);
    const V3 dir = normalize(vmix(vfma(d0, u, r00), vfma(d1, u, r10), v));
    const V3 eye = v3(P.eye[0], P.eye[1], P.eye[2]);

    // march(eye, dir, +1): the hit test comes before the t >= maxDist test, so a step can return a
    // hit at t >= maxDist (a far hit); trace() treats that as its miss, and so does the id below
    float t = 0.0f, id = -1.0f;
    bool done = !valid;
    for (int i = 0; i < P.max_steps; i++) {
        if (!__ballot(!done)) break;
        if (!done) {
            const V2 m = MAP::eval(P, vfma(dir, t, eye));
            if (m.x < 0.001f) {
                id = m.y;
                done = true;
            } else if (t >= P.max_dist) {
                t = P.max_dist;
                done = true;
            } else {
                t = fmaf(m.x, P.step_mult, t);
            }
        }
    }
    if (!done) { t = P.max_dist; id = -1.0f; }   // fell out of the loop: (maxDist, -1)
    const bool is_hit = valid && t < P.max_dist;
    if (!is_hit) id = -1.0f;
    const V3 pos = vfma(dir, t, eye);

    // getNormal: probes +x, -x, +y, -y, +z, -z with probe_point's offsets and signed zeros
    V3 n = v3(0.0f, 0.0f, 0.0f);
    if (__ballot(is_hit)) {
        float plus = 0.0f;
#pragma unroll 1
        for (int c = 0; c < 6; c++) {
            const int ax = c >> 1;
            const bool neg = (c & 1) != 0;
            const float hs = neg ? -0.001f : 0.001f, z0 = neg ? -0.0f : 0.0f;
            if (is_hit) {
                const V3 q = v3(pos.x + (ax == 0 ? hs : z0), pos.y + (ax == 1 ? hs : z0), pos.z + (ax == 2 ? hs : z0));
                const float m = MAP::eval(P, q).x;
                const float dv = plus - m;
                plus = neg ? plus : m;
                n.x = (neg && ax == 0) ? dv : n.x;
                n.y = (neg && ax == 1) ? dv : n.y;
                n.z = (neg && ax == 2) ? dv : n.z;
            }
        }
        if (is_hit) n = normalize(n);
    }
    if (valid) {
        const size_t o = (size_t)py * (size_t)P.W + (size_t)px;
        ray[o] = make_float4(dir.x, dir.y, dir.z, 0.0f);
        hit[o] = make_float4(pos.x, pos.y, pos.z, t);
        nrm[o] = is_hit ? make_float4(n.x, n.y, n.z, id) : make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    }
}

// P: the launch parameters of the context's scene and view with the rect in x0..y1 (already clamped
// to the image and non-empty); np: the scene's table-driven map class (accel.hpp SceneAccel::map_np).
hipError_t launch_guides(const KParams& P, int np, float4* ray, float4* hit, float4* nrm, hipStream_t s) {
    const int tx0 = P.x0 & ~7, ty0 = P.y0 & ~7;
    const long long tiles = (long long)((P.x1 - tx0 + 7) >> 3) * ((P.y1 - ty0 + 7) >> 3);
    const unsigned g = (unsigned)((tiles + 3) / 4);
    switch (np) {
    case 4: k_guides<4><<<g, 256, 0, s>>>(P, ray, hit, nrm); break;
    case 8: k_guides<8><<<g, 256, 0, s>>>(P, ray, hit, nrm); break;
    case 0: k_guides<0><<<g, 256, 0, s>>>(P, ray, hit, nrm); break;
    case -2: k_guides<-2><<<g, 256, 0, s>>>(P, ray, hit, nrm); break;
    default: k_guides<-1><<<g, 256, 0, s>>>(P, ray, hit, nrm); break;
    }
    return hipGetLastError();
}

}  // namespace rmr
