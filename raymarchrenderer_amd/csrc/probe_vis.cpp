// probe_vis.cpp — the probes' visibility: host functions (include/rmr.h rmr_probe_vis_dirs / rmr_probe_vis_fold /
// rmr_probe_irradiance_vis_host). No HIP: built into librmr.so and, with probe_vis_test.cpp, into a stand-alone
// CPU check (plain and under the sanitizers). They run the same header the kernels compile
// (rmr_probe_vis_rule.h).
#include <cmath>
#include <cstring>

#include "rmr_probe_vis_rule.h"

extern "C" {

int rmr_probe_vis_dirs(float out[64][3]) {
    if (!out) return RMR_E_INVALID;
    for (int j = 0; j < rmr::kVisTexels; j++) rmr::vis_texel_dir(j, out[j]);
    return RMR_OK;
}

int rmr_probe_vis_fold(const float* d_and_t, size_t n, uint32_t nspp, float range, float* out) {
    if (nspp == 0 || nspp > (1u << 24) || !rmr::vis_range_ok(range)) return RMR_E_INVALID;
    if (n && (!d_and_t || !out)) return RMR_E_INVALID;
    float D[rmr::kVisTexels][3];
    for (int j = 0; j < rmr::kVisTexels; j++) rmr::vis_texel_dir(j, D[j]);
    for (size_t i = 0; i < n; i++) {
        rmr::VisAcc S[rmr::kVisTexels];
        std::memset(S, 0, sizeof S);
        for (uint32_t k = 0; k < nspp; k++) {
            const float* s = d_and_t + 4 * ((size_t)k * n + i);
            if (!rmr::vis_sample_used(s[3])) continue;
            const float r = rmr::vis_sample_r(s[3], range);
            for (int j = 0; j < rmr::kVisTexels; j++) rmr::vis_fold_one(S[j], D[j], s[0], s[1], s[2], r);
        }
        float* o = out + rmr::kVisFloats * i;
        for (int j = 0; j < rmr::kVisTexels; j++) rmr::vis_resolve(S[j], range, o[2 * j], o[2 * j + 1]);
    }
    return RMR_OK;
}

int rmr_probe_irradiance_vis_host(const rmr_volume_desc* desc, const float* sh, const float* vis, const float* points,
                                  const float* normals, size_t n, float bias, float* out_rgba, size_t* first_bad) {
    if (first_bad) *first_bad = n;
    if (rmr::volume_bad_field(desc) || !sh || !vis || !rmr::vis_bias_ok(bias) || (n && (!points || !normals || !out_rgba)))
        return RMR_E_INVALID;
    int rc = RMR_OK;
    for (size_t i = 0; i < n; i++) {
        float* o = out_rgba + 4 * i;
        if (!rmr::bake_point_ok(points + 3 * i, normals + 3 * i)) {
            o[0] = o[1] = o[2] = o[3] = 0.0f;
            if (rc == RMR_OK && first_bad) *first_bad = i;
            rc = RMR_E_INVALID;
            continue;
        }
        rmr::probe_lookup_vis(*desc, sh, vis, points + 3 * i, normals + 3 * i, bias, o);
    }
    return rc;
}

}  // extern "C"
