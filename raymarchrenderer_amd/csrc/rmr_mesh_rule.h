// rmr_mesh_rule.h — the lattice and the surface-nets rule (include/rmr.h rmr_sample_volume /
// rmr_extract_mesh), written once for the host (mesh.cpp) and the device (rmr_volume.hip):
// a point's coordinates, the inside test, a cell's mask and vertex, and a point's emitting edges.
// Plain C++ and HIP: float32 sums, products and quotients only, no fused multiply-add, every select a
// comparison, so both sides run the same operations and NumPy reproduces them (tests/mesh_ref.py).
#pragma once
#include <stdint.h>
#include "../../include/rmr.h"

#if defined(__HIP__)
#define RMR_MESH_HD __host__ __device__ inline
#else
#define RMR_MESH_HD inline
#endif

namespace rmr {

constexpr int kVolumeMaxAxis = 4096;
constexpr uint64_t kVolumeMaxPoints = (uint64_t)1 << 30;

// what a point's flag byte holds (rmr_volume.hip k_mesh_classify)
constexpr uint32_t kMeshActive = 1u;       // the cell whose lower corner the point is has a vertex
constexpr uint32_t kMeshEdgeX = 2u;        // the interior edge from the point along x emits a quad (y: 4, z: 8)
constexpr uint32_t kMeshLowerInside = 16u; // the point itself is inside

// origin + (float)i * spacing: the product rounded, then the sum
RMR_MESH_HD float lattice_coord(float origin, int i, float spacing) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float step = (float)i * spacing;
    return origin + step;
}

// a NaN is outside, dist == iso is outside
RMR_MESH_HD bool mesh_inside(float dist, float iso) { return dist < iso; }

// the crossing of an edge from d0 (lower end) to d1; 0.5 unless it is a number in [0, 1]
RMR_MESH_HD float mesh_crossing(float d0, float d1, float iso) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float t = (iso - d0) / (d1 - d0);
    return (t >= 0.0f && t <= 1.0f) ? t : 0.5f;
}

// bit k: corner k is inside; corner k is at offsets (k & 1, k >> 1 & 1, k >> 2) on (x, y, z)
RMR_MESH_HD uint32_t mesh_cell_mask(const float d[8], float iso) {
    uint32_t m = 0;
    for (int k = 0; k < 8; k++) m |= mesh_inside(d[k], iso) ? (1u << k) : 0u;
    return m;
}
RMR_MESH_HD bool mesh_cell_active(uint32_t mask) { return mask != 0u && mask != 0xffu; }

// The vertex of an active cell whose lower corner is at (cx, cy, cz) = lattice_coord of its cell coordinates:
// the 12 edges in the order axis a = x, y, z, then (ou, ov) = (0, 0), (1, 0), (0, 1), (1, 1) on u = a + 1,
// v = a + 2 (cyclic); sequential float32 sums per axis; corner + spacing * (sum / count).
RMR_MESH_HD void mesh_cell_vertex(const float d[8], float iso, float cx, float cy, float cz, float spacing, float out[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float s[3] = {0.0f, 0.0f, 0.0f};
    int count = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int e = 0; e < 12; e++) {
        const int a = e >> 2, u = (a + 1) % 3, v = (a + 2) % 3;
        const int ou = e & 1, ov = (e >> 1) & 1;
        const int k0 = (ou << u) | (ov << v), k1 = k0 | (1 << a);
        const float d0 = d[k0], d1 = d[k1];
        if (mesh_inside(d0, iso) != mesh_inside(d1, iso)) {
            float c[3];
            c[a] = mesh_crossing(d0, d1, iso);
            c[u] = (float)ou;
            c[v] = (float)ov;
            s[0] = s[0] + c[0];
            s[1] = s[1] + c[1];
            s[2] = s[2] + c[2];
            count++;
        }
    }
    const float n = (float)count;
    const float mx = s[0] / n, my = s[1] / n, mz = s[2] / n;
    const float px = spacing * mx, py = spacing * my, pz = spacing * mz;
    out[0] = cx + px;
    out[1] = cy + py;
    out[2] = cz + pz;
}

// The flag byte of point (ix, iy, iz), whose cell exists (every i_a <= n_a - 2), from the cell's corners:
// the cell's activity, the point's inside-ness and which of its three edges emit a quad (interior, ends differ).
RMR_MESH_HD uint32_t mesh_point_flags(const float d[8], float iso, int ix, int iy, int iz, int nx, int ny, int nz) {
    const uint32_t mask = mesh_cell_mask(d, iso);
    uint32_t f = mesh_cell_active(mask) ? kMeshActive : 0u;
    const bool in0 = (mask & 1u) != 0u;
    if (in0) f |= kMeshLowerInside;
    const bool mx = ix >= 1 && ix <= nx - 2, my = iy >= 1 && iy <= ny - 2, mz = iz >= 1 && iz <= nz - 2;
    if (my && mz && in0 != ((mask & 2u) != 0u)) f |= kMeshEdgeX;
    if (mz && mx && in0 != ((mask & 4u) != 0u)) f |= kMeshEdgeX << 1;
    if (mx && my && in0 != ((mask & 16u) != 0u)) f |= kMeshEdgeX << 2;
    return f;
}

// The four cells around the edge from the point of linear index k along axis ax, as point indices of their
// lower corners, in the quad's order for an inside lower end; stride[a]: the linear index step of axis a.
RMR_MESH_HD void mesh_quad_cells(uint32_t k, int ax, const uint32_t stride[3], uint32_t out[4]) {
    const uint32_t su = stride[(ax + 1) % 3], sv = stride[(ax + 2) % 3];
    out[0] = k - su - sv;
    out[1] = k - sv;
    out[2] = k;
    out[3] = k - su;
}

// "origin" / "spacing" / "n" / "points" / "desc", or null for a descriptor that is in range
RMR_MESH_HD const char* volume_bad_field(const rmr_volume_desc* d) {
    if (!d) return "desc";
    for (int a = 0; a < 3; a++)
        if (!(d->origin[a] - d->origin[a] == 0.0f)) return "origin";   // (finite)
    if (!(d->spacing - d->spacing == 0.0f) || !(d->spacing > 0.0f)) return "spacing";
    for (int a = 0; a < 3; a++)
        if (d->n[a] < 2 || d->n[a] > kVolumeMaxAxis) return "n";
    if ((uint64_t)d->n[0] * (uint64_t)d->n[1] * (uint64_t)d->n[2] > kVolumeMaxPoints) return "points";
    return nullptr;
}

}  // namespace rmr
