// rmr_probe_ray.h — what the probes' ray sources share (rmr_probe.hip, rmr_probe_vis.hip): sample k of probe i
// as a ray, with the reject and buried tests (include/rmr.h rmr_bake_probes), the wave's reject count and the
// switch over the scene's table-driven map class. Device code.
#pragma once
#include "rmr_cast.h"
#include "rmr_probe_rule.h"

namespace rmr {

struct ProbeRay {
    V3 o, d;
    float time, gxt, gyt;
    int32_t gx, gy;
};

enum { kProbeUsed = 0, kProbeBuried = 1, kProbeRejected = 2 };

// Sample k of probe i: kProbeUsed with the ray, or why there is none.
// bury: run the buried test (the visibility's field form takes the field's validity instead).
template <class MAP>
RMR_D int probe_ray(const KParams& P, const ProbeList& B, uint64_t i, uint32_t k, ProbeRay& r, bool bury = true) {
    float p[3];
    probe_point(B, i, p);
    const uint64_t idx = B.first_index + i;
    r.gx = bake_gx(idx);
    r.gy = bake_gy(idx);
    r.time = B.times[k];
    r.gxt = (float)r.gx + r.time;
    r.gyt = (float)r.gy + r.time;
    if (!probe_point_ok(p, B.extent)) return kProbeRejected;
    r.o = v3(p[0], p[1], p[2]);
    if (bury && probe_buried(MAP::eval(P, r.o).x, B.clearance)) return kProbeBuried;
    Lane L;
    L.gxt = r.gxt;
    L.gyt = r.gyt;
    L.rc = 0.0f;   // a fresh chain, started as main() starts a pixel's (rmr_bake.hip bake_ray has the reason)
    (void)lrand(L, v2(L.gxt, L.gyt));
    r.d = hemisphere(L, v2(p[0], p[1]), v2(p[2], p[0]), v3(0.0f, 0.0f, 0.0f));   // zero normal: the whole sphere
    return kProbeUsed;
}

// A wave's rejected probes, counted once per probe (at its sample 0): one add per wave that saw one.
RMR_D void note_probe_rejects(bool rejected, unsigned long long* rejects) {
    const uint64_t rj = __ballot(rejected);
    if (rejects && rejected && (int)(threadIdx.x & 63u) == __ffsll((unsigned long long)rj) - 1)
        atomicAdd(rejects, (unsigned long long)__popcll(rj));
}

#define RMR_PROBE_SWITCH(NPV, CALL)      \
    switch (NPV) {                       \
    case 4: CALL(4); break;              \
    case 8: CALL(8); break;              \
    case 0: CALL(0); break;              \
    case -2: CALL(-2); break;            \
    default: CALL(-1); break;            \
    }

}  // namespace rmr
