// bake.cpp — the light bake's host functions (include/rmr.h rmr_default_bake_params / rmr_check_bake_params /
// rmr_bake_check_points / rmr_bake_fold / rmr_srgb8_pixels / rmr_encode_ply_colors). No HIP: built into
// librmr.so and, with bake_test.cpp, into a stand-alone CPU check (plain and under the sanitizers). They run
// the same header the kernels compile (rmr_bake_rule.h).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "rmr_bake_rule.h"

extern "C" {

void rmr_default_bake_params(rmr_bake_params* p) {
    if (!p) return;
    p->flags = RMR_BAKE_RADIANCE;
    p->bias = 0.002f;
    p->ao_distance = INFINITY;
    p->origin_extent = 0.0f;
    p->first_index = 0;
}

int rmr_check_bake_params(const rmr_bake_params* p) {
    if (!p) return RMR_E_INVALID;
    if (p->flags == 0 || (p->flags & ~rmr::kBakeFlags)) return RMR_E_INVALID;
    if (!(p->bias - p->bias == 0.0f)) return RMR_E_INVALID;
    if (!(p->ao_distance > 0.0f)) return RMR_E_INVALID;   // (a NaN fails the comparison; +inf passes)
    if (p->first_index > rmr::kBakeMaxIndex) return RMR_E_INVALID;
    return RMR_OK;
}

int rmr_bake_check_points(const float* points, const float* normals, size_t n, size_t* first_bad) {
    if (n && (!points || !normals)) return RMR_E_INVALID;
    if (first_bad) *first_bad = n;
    for (size_t i = 0; i < n; i++)
        if (!rmr::bake_point_ok(points + 3 * i, normals + 3 * i)) {
            if (first_bad) *first_bad = i;
            return RMR_E_INVALID;
        }
    return RMR_OK;
}

int rmr_bake_fold(const float* L_rgb, const float* c, const float* cv, size_t n, uint32_t nspp, float* out_rgba,
                  float* out_ao) {
    if (nspp == 0 || nspp > (1u << 24)) return RMR_E_INVALID;
    if (n && ((out_rgba && (!L_rgb || !c)) || (out_ao && (!c || !cv)))) return RMR_E_INVALID;
    for (size_t i = 0; i < n; i++) {
        rmr::BakeState st;
        rmr::bake_state_init(st);
        for (uint32_t k = 0; k < nspp; k++) {
            const size_t u = (size_t)k * n + i;
            if (out_rgba) rmr::bake_fold_radiance(st, L_rgb[3 * u], L_rgb[3 * u + 1], L_rgb[3 * u + 2], c[u]);
            if (out_ao) rmr::bake_fold_ao(st, c[u], cv[u]);
        }
        if (out_rgba) rmr::bake_resolve_radiance(st, out_rgba + 4 * i);
        if (out_ao) out_ao[i] = rmr::bake_resolve_ao(st);
    }
    return RMR_OK;
}

// sRGB decision points of Graphics::Display's GL_FRAMEBUFFER_SRGB write: byte(c) = round(255 srgb(c))
// for c in [0, 1] (srgb: 12.92 c below 0.0031308, else 1.055 c^(1/2.4) - 0.055), so byte(c) >= k
// <=> srgb(c) >= (k - 1/2) / 255 <=> c >= linear((k - 1/2) / 255); out[k] is that bound rounded up to
// a float (for a float c the comparison is then exact), out[0] = 0.
int rmr_srgb_thresholds(float out[256]) {
    if (!out) return RMR_E_INVALID;
    out[0] = 0.0f;
    for (int k = 1; k < 256; k++) {
        const double y = (k - 0.5) / 255.0;
        const double lin = (y <= 0.04045) ? y / 12.92 : std::pow((y + 0.055) / 1.055, 2.4);
        float f = (float)lin;
        if ((double)f < lin) f = std::nextafter(f, 2.0f);
        out[k] = f;
    }
    return RMR_OK;
}

int rmr_srgb8_pixels(const float* rgb, size_t n, uint8_t* out) {
    if (n && (!rgb || !out)) return RMR_E_INVALID;
    float thr[256];
    const int r = rmr_srgb_thresholds(thr);
    if (r != RMR_OK) return r;
    for (size_t i = 0; i < 3 * n; i++) {
        // the largest k with thr[k] <= v (thr[0] admits everything that is not a NaN; a NaN: 0)
        int lo = 0, hi = 256;
        while (hi - lo > 1) {
            const int mid = (lo + hi) / 2;
            if (rgb[i] >= thr[mid]) lo = mid;
            else hi = mid;
        }
        out[i] = (uint8_t)lo;
    }
    return RMR_OK;
}

int rmr_encode_ply_colors(const char* path, const float* vertices, const float* normals, const float* ids,
                          const uint8_t* rgb8, size_t n_vertices, const uint32_t* quads, size_t n_quads) {
    if (!rgb8) return rmr_encode_ply(path, vertices, normals, ids, n_vertices, quads, n_quads);
    if (!path || (n_vertices && !vertices) || (n_quads && !quads)) return RMR_E_INVALID;
    for (size_t i = 0; i < 4 * n_quads; i++)
        if (quads[i] >= n_vertices) return RMR_E_INVALID;
    const uint16_t one = 1;
    unsigned char first;
    std::memcpy(&first, &one, 1);
    if (first != 1) return RMR_E_UNSUPPORTED;   // (the arrays are written as they lie in memory: little-endian hosts)
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return RMR_E_IO;
    std::fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\n", n_vertices);
    std::fprintf(f, "property float x\nproperty float y\nproperty float z\n");
    if (normals) std::fprintf(f, "property float nx\nproperty float ny\nproperty float nz\n");
    if (ids) std::fprintf(f, "property float material\n");
    std::fprintf(f, "property uchar red\nproperty uchar green\nproperty uchar blue\n");
    std::fprintf(f, "element face %zu\nproperty list uchar uint vertex_indices\nend_header\n", n_quads);
    for (size_t i = 0; i < n_vertices; i++) {
        std::fwrite(vertices + 3 * i, sizeof(float), 3, f);
        if (normals) std::fwrite(normals + 3 * i, sizeof(float), 3, f);
        if (ids) std::fwrite(ids + i, sizeof(float), 1, f);
        std::fwrite(rgb8 + 3 * i, 1, 3, f);
    }
    const unsigned char four = 4;
    for (size_t i = 0; i < n_quads; i++) {
        std::fwrite(&four, 1, 1, f);
        std::fwrite(quads + 4 * i, sizeof(uint32_t), 4, f);
    }
    const bool bad = std::ferror(f) != 0;
    const bool closed = std::fclose(f) == 0;
    return !bad && closed ? RMR_OK : RMR_E_IO;
}

}  // extern "C"
