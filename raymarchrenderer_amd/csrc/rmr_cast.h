// rmr_cast.h — the first hit of a ray through a table-driven map class (include/rmr.h rmr_cast_rays states
// it operation by operation): march(o, d, +1) and getNormal at the hit, written once for the kernels that
// cast rays of their own: k_cast_rays (rmr_query.hip) and k_aov (rmr_aov.hip). Like the guide pass: no RNG,
// no escape bound, no approximate map, so every class gives the oracle's march / getNormal bits.
#pragma once
#include "rmr_trace.h"

namespace rmr {

// march(o, dir, +1) of a wave's rays: the hit test comes before the t >= maxDist test (a far hit keeps
// its t). `ok`: the lane has a ray. Returns is_hit (t < maxDist); id is -1 for a miss. Wave-uniform loop
// exits: call it from every lane of the wave.
template <class MAP>
RMR_D bool march_first_hit(const KParams& P, bool ok, V3 o, V3 dir, float& t, float& id) {
    t = 0.0f;
    id = -1.0f;
    bool done = !ok;
    for (int s = 0; s < P.max_steps; s++) {
        if (!__ballot(!done)) break;
        if (!done) {
            const V2 m = MAP::eval(P, vfma(dir, t, o));
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
    const bool is_hit = ok && t < P.max_dist;
    if (!is_hit) id = -1.0f;
    return is_hit;
}

// getNormal at the hits of a wave (k_guides' loop): probes +x, -x, +y, -y, +z, -z with probe_point's
// offsets and signed zeros, then normalize. Wave-uniform outside the per-lane guard.
template <class MAP>
RMR_D V3 hit_normal(const KParams& P, bool is_hit, V3 pos) {
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
    return n;
}

}  // namespace rmr
