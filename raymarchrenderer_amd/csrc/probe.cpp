// probe.cpp — the irradiance probes' host functions (include/rmr.h rmr_default_probe_params /
// rmr_check_probe_params / rmr_sh_basis / rmr_probe_fold / rmr_probe_irradiance_host). No HIP: built into
// librmr.so and, with probe_test.cpp, into a stand-alone CPU check (plain and under the sanitizers). They run
// the same header the kernels compile (rmr_probe_rule.h).
#include <cmath>
#include <cstring>

#include "rmr_probe_rule.h"

static_assert(sizeof(rmr_probe_params) == 16, "rmr_probe_params is 16 bytes");

extern "C" {

void rmr_default_probe_params(rmr_probe_params* p) {
    if (!p) return;
    p->clearance = 0.0f;
    p->origin_extent = 0.0f;
    p->first_index = 0;
}

int rmr_check_probe_params(const rmr_probe_params* p) {
    if (!p) return RMR_E_INVALID;
    if (!(p->clearance - p->clearance == 0.0f) || !(p->clearance >= 0.0f)) return RMR_E_INVALID;
    if (p->first_index > rmr::kBakeMaxIndex) return RMR_E_INVALID;
    return RMR_OK;
}

int rmr_sh_basis(const float* dirs, size_t n, float* out) {
    if (n && (!dirs || !out)) return RMR_E_INVALID;
    for (size_t i = 0; i < n; i++) rmr::sh_basis(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], out + rmr::kProbeSH * i);
    return RMR_OK;
}

int rmr_probe_fold(const float* L_rgb, const float* dirs, size_t n, uint32_t nspp, float* out) {
    if (nspp == 0 || nspp > (1u << 24)) return RMR_E_INVALID;
    if (n && (!L_rgb || !dirs || !out)) return RMR_E_INVALID;
    for (size_t i = 0; i < n; i++) {
        float S[rmr::kProbeSH][3];
        std::memset(S, 0, sizeof S);
        float n_used = 0.0f;
        for (uint32_t k = 0; k < nspp; k++) {
            const float* L = L_rgb + 3 * ((size_t)k * n + i);
            const float* d = dirs + 3 * ((size_t)k * n + i);
            if (!rmr::probe_sample_used(L[0], L[1], L[2])) continue;
            float Y[rmr::kProbeSH];
            rmr::sh_basis(d[0], d[1], d[2], Y);
            for (int m = 0; m < rmr::kProbeSH; m++) rmr::probe_fold_one(S[m], L[0], L[1], L[2], Y[m]);
            n_used = n_used + 1.0f;
        }
        float* o = out + rmr::kProbeFloats * i;
        for (int m = 0; m < rmr::kProbeSH; m++)
            for (int c = 0; c < 3; c++) o[3 * m + c] = rmr::probe_resolve_one(S[m][c], n_used);
        o[rmr::kProbeFloats - 1] = n_used;
    }
    return RMR_OK;
}

int rmr_probe_irradiance_host(const rmr_volume_desc* desc, const float* sh, const float* points, const float* normals,
                              size_t n, float* out_rgba, size_t* first_bad) {
    if (first_bad) *first_bad = n;
    if (rmr::volume_bad_field(desc) || !sh || (n && (!points || !normals || !out_rgba))) return RMR_E_INVALID;
    int rc = RMR_OK;
    for (size_t i = 0; i < n; i++) {
        float* o = out_rgba + 4 * i;
        if (!rmr::bake_point_ok(points + 3 * i, normals + 3 * i)) {
            o[0] = o[1] = o[2] = o[3] = 0.0f;
            if (rc == RMR_OK && first_bad) *first_bad = i;
            rc = RMR_E_INVALID;
            continue;
        }
        rmr::probe_lookup(*desc, sh, points + 3 * i, normals + 3 * i, o);
    }
    return rc;
}

}  // extern "C"
