// mesh.cpp — the lattice's and the mesh's host functions (include/rmr.h rmr_check_volume / rmr_surface_nets /
// rmr_encode_obj / rmr_encode_ply). No HIP: built into librmr.so and, with mesh_test.cpp, into a stand-alone
// CPU check (plain and under the sanitizers). They run the same header the kernels compile (rmr_mesh_rule.h).
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "rmr_mesh_rule.h"

namespace {
using rmr::kMeshActive;
using rmr::kMeshEdgeX;
using rmr::kMeshLowerInside;

bool finite(float v) { return v - v == 0.0f; }

struct File {
    std::FILE* f;
    explicit File(const char* path) : f(path ? std::fopen(path, "wb") : nullptr) {}
    ~File() { if (f) std::fclose(f); }
    // flush and close: false if anything failed since the file was opened
    bool done() {
        if (!f) return false;
        const bool bad = std::ferror(f) != 0;
        const bool closed = std::fclose(f) == 0;
        f = nullptr;
        return !bad && closed;
    }
};

bool indices_ok(const uint32_t* quads, size_t n_quads, size_t n_vertices) {
    for (size_t i = 0; i < 4 * n_quads; i++)
        if (quads[i] >= n_vertices) return false;
    return true;
}
}  // namespace

extern "C" {

int rmr_check_volume(const rmr_volume_desc* desc, const char** bad_field) {
    const char* bad = rmr::volume_bad_field(desc);
    if (bad_field) *bad_field = bad;
    return bad ? RMR_E_INVALID : RMR_OK;
}

int rmr_surface_nets(const float* dist, const rmr_volume_desc* desc, float iso, float* vertices, size_t vertex_cap,
                     uint32_t* quads, size_t quad_cap, rmr_mesh_info* info) {
    if (!dist || !info || rmr::volume_bad_field(desc) || !finite(iso) || ((vertices == nullptr) != (quads == nullptr)))
        return RMR_E_INVALID;
    const int nx = desc->n[0], ny = desc->n[1], nz = desc->n[2];
    const size_t sy = (size_t)nx, sz = (size_t)nx * (size_t)ny, n_points = sz * (size_t)nz;
    std::vector<uint8_t> flags;
    std::vector<uint32_t> cell_vertex;
    try {
        flags.assign(n_points, 0);
        if (vertices) cell_vertex.assign(n_points, 0);
    } catch (const std::bad_alloc&) {
        return RMR_E_NOMEM;
    }
    // the count pass: a flag byte per point, as k_mesh_classify
    uint64_t n_vertices = 0, n_quads = 0;
    for (int iz = 0; iz + 1 < nz; iz++)
        for (int iy = 0; iy + 1 < ny; iy++)
            for (int ix = 0; ix + 1 < nx; ix++) {
                const size_t k = (size_t)ix + sy * (size_t)iy + sz * (size_t)iz;
                float d[8];
                for (int c = 0; c < 8; c++) d[c] = dist[k + (size_t)(c & 1) + (size_t)((c >> 1) & 1) * sy + (size_t)(c >> 2) * sz];
                const uint32_t f = rmr::mesh_point_flags(d, iso, ix, iy, iz, nx, ny, nz);
                flags[k] = (uint8_t)f;
                n_vertices += f & kMeshActive;
                n_quads += (f >> 1 & 1u) + (f >> 2 & 1u) + (f >> 3 & 1u);
            }
    info->n_vertices = n_vertices;
    info->n_quads = n_quads;
    if (!vertices) return RMR_OK;
    if (n_vertices > vertex_cap || n_quads > quad_cap) return RMR_E_INVALID;
    // the fill passes: vertices in point order, then quads in point order
    uint32_t v = 0;
    for (size_t k = 0; k < n_points; k++) {
        if (!(flags[k] & kMeshActive)) continue;
        const int ix = (int)(k % sy), iy = (int)(k / sy % (size_t)ny), iz = (int)(k / sz);
        float d[8];
        for (int c = 0; c < 8; c++) d[c] = dist[k + (size_t)(c & 1) + (size_t)((c >> 1) & 1) * sy + (size_t)(c >> 2) * sz];
        rmr::mesh_cell_vertex(d, iso, rmr::lattice_coord(desc->origin[0], ix, desc->spacing),
                              rmr::lattice_coord(desc->origin[1], iy, desc->spacing),
                              rmr::lattice_coord(desc->origin[2], iz, desc->spacing), desc->spacing, vertices + 3 * (size_t)v);
        cell_vertex[k] = v++;
    }
    const uint32_t stride[3] = {1u, (uint32_t)sy, (uint32_t)sz};
    size_t q = 0;
    for (size_t k = 0; k < n_points; k++) {
        const uint32_t f = flags[k];
        for (int ax = 0; ax < 3; ax++) {
            if (!(f & (kMeshEdgeX << ax))) continue;
            uint32_t c[4];
            rmr::mesh_quad_cells((uint32_t)k, ax, stride, c);
            const bool lower_in = (f & kMeshLowerInside) != 0u;
            for (int j = 0; j < 4; j++) quads[4 * q + (size_t)j] = cell_vertex[c[lower_in ? j : 3 - j]];
            q++;
        }
    }
    return RMR_OK;
}

int rmr_encode_obj(const char* path, const float* vertices, const float* normals, size_t n_vertices, const uint32_t* quads,
                   size_t n_quads) {
    if (!path || (n_vertices && !vertices) || (n_quads && !quads)) return RMR_E_INVALID;
    if (!indices_ok(quads, n_quads, n_vertices)) return RMR_E_INVALID;
    File out(path);
    if (!out.f) return RMR_E_IO;
    std::fprintf(out.f, "# %zu vertices, %zu quads\n", n_vertices, n_quads);
    for (size_t i = 0; i < n_vertices; i++)
        std::fprintf(out.f, "v %.9g %.9g %.9g\n", (double)vertices[3 * i], (double)vertices[3 * i + 1], (double)vertices[3 * i + 2]);
    if (normals)
        for (size_t i = 0; i < n_vertices; i++)
            std::fprintf(out.f, "vn %.9g %.9g %.9g\n", (double)normals[3 * i], (double)normals[3 * i + 1], (double)normals[3 * i + 2]);
    for (size_t i = 0; i < n_quads; i++) {
        const unsigned long a = (unsigned long)quads[4 * i] + 1, b = (unsigned long)quads[4 * i + 1] + 1,
                            c = (unsigned long)quads[4 * i + 2] + 1, d = (unsigned long)quads[4 * i + 3] + 1;
        if (normals) std::fprintf(out.f, "f %lu//%lu %lu//%lu %lu//%lu %lu//%lu\n", a, a, b, b, c, c, d, d);
        else std::fprintf(out.f, "f %lu %lu %lu %lu\n", a, b, c, d);
    }
    return out.done() ? RMR_OK : RMR_E_IO;
}

int rmr_encode_ply(const char* path, const float* vertices, const float* normals, const float* ids, size_t n_vertices,
                   const uint32_t* quads, size_t n_quads) {
    if (!path || (n_vertices && !vertices) || (n_quads && !quads)) return RMR_E_INVALID;
    if (!indices_ok(quads, n_quads, n_vertices)) return RMR_E_INVALID;
    const uint16_t one = 1;
    unsigned char first;
    std::memcpy(&first, &one, 1);
    if (first != 1) return RMR_E_UNSUPPORTED;   // (the arrays are written as they lie in memory: little-endian hosts)
    File out(path);
    if (!out.f) return RMR_E_IO;
    std::fprintf(out.f, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\n", n_vertices);
    std::fprintf(out.f, "property float x\nproperty float y\nproperty float z\n");
    if (normals) std::fprintf(out.f, "property float nx\nproperty float ny\nproperty float nz\n");
    if (ids) std::fprintf(out.f, "property float material\n");
    std::fprintf(out.f, "element face %zu\nproperty list uchar uint vertex_indices\nend_header\n", n_quads);
    for (size_t i = 0; i < n_vertices; i++) {
        std::fwrite(vertices + 3 * i, sizeof(float), 3, out.f);
        if (normals) std::fwrite(normals + 3 * i, sizeof(float), 3, out.f);
        if (ids) std::fwrite(ids + i, sizeof(float), 1, out.f);
    }
    const unsigned char four = 4;
    for (size_t i = 0; i < n_quads; i++) {
        std::fwrite(&four, 1, 1, out.f);
        std::fwrite(quads + 4 * i, sizeof(uint32_t), 4, out.f);
    }
    return out.done() ? RMR_OK : RMR_E_IO;
}

}  // extern "C"
