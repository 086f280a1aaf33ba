// aov.cpp — the sampled AOVs' host functions (include/rmr.h rmr_aov_fold / rmr_aov_resolve / rmr_aov_init).
// No HIP: built into librmr.so and, with aov_test.cpp, into a stand-alone CPU check (plain and under the
// sanitizers). They run the same header the kernels compile (rmr_aov_rule.h).
#include <cstring>

#include "rmr_aov_rule.h"

static_assert(sizeof(rmr::AovState) == 20 * sizeof(float), "the state is five float4 per pixel");

namespace {
using rmr::Aov4;
using rmr::AovState;

// state and resolved planes: [plane][pixel][4] floats
Aov4 get4(const float* planes, size_t n_px, int plane, size_t i) {
    Aov4 v;
    std::memcpy(&v, planes + ((size_t)plane * n_px + i) * 4, sizeof v);
    return v;
}
void put4(float* planes, size_t n_px, int plane, size_t i, const Aov4& v) {
    std::memcpy(planes + ((size_t)plane * n_px + i) * 4, &v, sizeof v);
}
AovState get_state(const float* state, size_t n_px, size_t i) {
    AovState s;
    s.stats = get4(state, n_px, RMR_AOV_STATS, i);
    s.nrm = get4(state, n_px, RMR_AOV_NORMAL, i);
    s.pos = get4(state, n_px, RMR_AOV_POSITION, i);
    s.ids01 = get4(state, n_px, RMR_AOV_IDS01, i);
    s.ids23 = get4(state, n_px, RMR_AOV_IDS23, i);
    return s;
}
void put_state(float* state, size_t n_px, size_t i, const AovState& s) {
    put4(state, n_px, RMR_AOV_STATS, i, s.stats);
    put4(state, n_px, RMR_AOV_NORMAL, i, s.nrm);
    put4(state, n_px, RMR_AOV_POSITION, i, s.pos);
    put4(state, n_px, RMR_AOV_IDS01, i, s.ids01);
    put4(state, n_px, RMR_AOV_IDS23, i, s.ids23);
}
}  // namespace

extern "C" {

int rmr_aov_init(float* state, size_t n_px) {
    if (!state && n_px) return RMR_E_INVALID;
    const AovState s = rmr::aov_initial();
    for (size_t i = 0; i < n_px; i++) put_state(state, n_px, i, s);
    return RMR_OK;
}

int rmr_aov_fold(float* state, const rmr_hit* hits, size_t n_px, uint32_t nspp) {
    if (n_px && (!state || (nspp && !hits))) return RMR_E_INVALID;
    for (size_t i = 0; i < n_px; i++) {
        AovState s = get_state(state, n_px, i);
        if ((double)s.stats.x + (double)nspp > (double)rmr::kAovMaxSamples) return RMR_E_INVALID;   // (nothing written from here on)
    }
    for (size_t i = 0; i < n_px; i++) {
        AovState s = get_state(state, n_px, i);
        for (uint32_t k = 0; k < nspp; k++) {
            const rmr_hit& h = hits[(size_t)k * n_px + i];
            rmr::aov_fold1(s, h.pos[0], h.pos[1], h.pos[2], h.t, h.n[0], h.n[1], h.n[2], h.id);
        }
        put_state(state, n_px, i, s);
    }
    return RMR_OK;
}

int rmr_aov_resolve(const float* state, size_t n_px, float max_dist, float* out) {
    if (n_px && (!state || !out)) return RMR_E_INVALID;
    for (size_t i = 0; i < n_px; i++) {
        const rmr::AovResolved r = rmr::aov_resolve1(get_state(state, n_px, i), max_dist);
        put4(out, n_px, RMR_AOV_R_DEPTH, i, r.depth);
        put4(out, n_px, RMR_AOV_R_NORMAL, i, r.nrm);
        put4(out, n_px, RMR_AOV_R_POSITION, i, r.pos);
        put4(out, n_px, RMR_AOV_R_IDS01, i, r.ids01);
        put4(out, n_px, RMR_AOV_R_IDS23, i, r.ids23);
    }
    return RMR_OK;
}

}  // extern "C"
