// rmr_volume.hip — SDF volume sampling and surface-nets extraction (include/rmr.h rmr_sample_volume /
// rmr_extract_mesh). The rule is rmr_mesh_rule.h's; everything here is one thread per
// lattice point, 256 points per block, x fastest, so a wave reads 64 consecutive points of a row.
//   k_sample_volume<NP, IDS>  map() at the lattice's points, which the kernel computes itself: nothing
//                             read but the scene's tables, 4 (8 with IDS) bytes written per point
//   k_mesh_classify           the 8 corners of the point's cell -> a flag byte per point (active cell,
//                             emitting edges, the point's inside-ness) and the block's totals of vertices
//                             and quads by ballot / popcount
//   k_mesh_scan1 / _scan2     exclusive scan of the block totals: kScanGroup totals per workgroup, then
//                             the workgroups' totals by one workgroup of any length; the grand totals
//   k_mesh_vertices           active cells: vertex number = scanned base + rank in the block; the vertex
//                             by the rule, and the number into the cell-index volume
//   k_mesh_quads              emitting edges: place = scanned base + rank; the four cells' numbers
//   k_mesh_attr<NP>           getNormal and map().y at the vertices (rmr_cast.h hit_normal, whole waves)
// The scans alone decide where an element lands: no atomic anywhere, two runs give the same bytes.
#include <hip/hip_runtime.h>
#include "rmr_cast.h"
#include "rmr_mesh_rule.h"

namespace rmr {

constexpr uint32_t kMeshBlock = 256;     // points per block of the classify / emit kernels
constexpr uint32_t kScanGroup = 1024;    // block totals one k_mesh_scan1 workgroup scans (4 per thread)

struct Lattice {
    float ox, oy, oz, spacing;
    int32_t nx, ny, nz;
    uint32_t n_points;
};

namespace {
RMR_D void point_of(const Lattice& L, uint32_t k, int& ix, int& iy, int& iz) {
    const uint32_t row = k / (uint32_t)L.nx;
    ix = (int)(k - row * (uint32_t)L.nx);
    iz = (int)(row / (uint32_t)L.ny);
    iy = (int)(row - (uint32_t)iz * (uint32_t)L.ny);
}

// the 8 corners of the cell whose lower corner is point k (which exists: every i_a <= n_a - 2)
RMR_D void load_corners(const float* dist, const Lattice& L, uint32_t k, float d[8]) {
    const uint32_t sy = (uint32_t)L.nx, sz = (uint32_t)L.nx * (uint32_t)L.ny;
#pragma unroll
    for (int c = 0; c < 8; c++) d[c] = dist[k + (uint32_t)(c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz];
}

// exclusive scan over the wave's 64 lanes (all active); total: the wave's sum
RMR_D uint32_t wave_scan(uint32_t v, uint32_t lane, uint32_t& total) {
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if ((int)lane >= d) inc += o;
    }
    total = __shfl(inc, 63, 64);
    return inc - v;
}

// exclusive scan of (a, b) over a block of 256 threads (all active); the block's totals to ta, tb
RMR_D void block_scan2(uint32_t& a, uint32_t& b, uint32_t& ta, uint32_t& tb, uint32_t (*lds)[2]) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t wa, wb;
    a = wave_scan(a, lane, wa);
    b = wave_scan(b, lane, wb);
    if (lane == 0) { lds[w][0] = wa; lds[w][1] = wb; }
    __syncthreads();
    ta = tb = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        if (i < w) { a += lds[i][0]; b += lds[i][1]; }
        ta += lds[i][0];
        tb += lds[i][1];
    }
    __syncthreads();
}

// a lane's rank among the set bits of a ballot, and the flag byte's quad count
RMR_D uint32_t rank_in(uint64_t ballot, uint32_t lane) { return (uint32_t)__popcll(ballot & (((uint64_t)1 << lane) - 1u)); }
RMR_D uint32_t quads_of(uint32_t f) { return (f >> 1 & 1u) + (f >> 2 & 1u) + (f >> 3 & 1u); }

// (vertices, quads) before thread's element in its block of 256: ranks by ballot / popcount, the waves
// before it through LDS. Every thread of the block calls it.
RMR_D void block_ranks(uint32_t f, uint32_t& vrank, uint32_t& qrank, uint32_t& vtot, uint32_t& qtot, uint32_t (*lds)[2]) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t q = quads_of(f);
    const uint64_t bv = __ballot((f & kMeshActive) != 0u), b0 = __ballot((q & 1u) != 0u), b1 = __ballot((q & 2u) != 0u);
    vrank = rank_in(bv, lane);
    qrank = rank_in(b0, lane) + 2u * rank_in(b1, lane);
    if (lane == 0) {
        lds[w][0] = (uint32_t)__popcll(bv);
        lds[w][1] = (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1);
    }
    __syncthreads();
    vtot = qtot = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        if (i < w) { vrank += lds[i][0]; qrank += lds[i][1]; }
        vtot += lds[i][0];
        qtot += lds[i][1];
    }
}
}  // namespace

// ---- the volume ------------------------------------------------------------------------------------
template <int NP, bool IDS>
__global__ __launch_bounds__(256) void k_sample_volume(KParams P, Lattice L, float* dist, float* id) {
    const uint32_t stride = gridDim.x * 256u;   // (the grid is capped so that this fits)
    for (uint64_t k64 = (uint64_t)blockIdx.x * 256u + threadIdx.x; k64 < L.n_points; k64 += stride) {
        const uint32_t k = (uint32_t)k64;
        int ix, iy, iz;
        point_of(L, k, ix, iy, iz);
        const V3 p = v3(lattice_coord(L.ox, ix, L.spacing), lattice_coord(L.oy, iy, L.spacing),
                        lattice_coord(L.oz, iz, L.spacing));
        const V2 m = TableMap<NP>::eval(P, p);
        dist[k] = m.x;
        if constexpr (IDS) id[k] = m.y;
    }
}

// ---- extraction ------------------------------------------------------------------------------------
// flags[k] for every point, totals[block] = (vertices, quads) of the block's 256 points
__global__ __launch_bounds__(256) void k_mesh_classify(Lattice L, const float* dist, float iso, uint8_t* flags, uint2* totals) {
    __shared__ uint32_t lds[4][2];
    const uint32_t k = blockIdx.x * kMeshBlock + threadIdx.x;
    uint32_t f = 0;
    if (k < L.n_points) {
        int ix, iy, iz;
        point_of(L, k, ix, iy, iz);
        if (ix <= L.nx - 2 && iy <= L.ny - 2 && iz <= L.nz - 2) {
            float d[8];
            load_corners(dist, L, k, d);
            f = mesh_point_flags(d, iso, ix, iy, iz, L.nx, L.ny, L.nz);
        }
        flags[k] = (uint8_t)f;
    }
    uint32_t vr, qr, vt, qt;
    block_ranks(f, vr, qr, vt, qt, lds);
    if (threadIdx.x == 0) totals[blockIdx.x] = make_uint2(vt, qt);
}

// totals[0, n) -> their exclusive scan within each group of kScanGroup, in place; group_totals[g]
__global__ __launch_bounds__(256) void k_mesh_scan1(uint2* totals, uint32_t n, uint2* group_totals) {
    __shared__ uint32_t lds[4][2];
    const uint32_t i0 = blockIdx.x * kScanGroup + threadIdx.x * 4u;
    uint2 v[4];
    uint32_t a = 0, b = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        v[j] = (i0 + j < n) ? totals[i0 + j] : make_uint2(0u, 0u);
        a += v[j].x;
        b += v[j].y;
    }
    uint32_t ta, tb;
    block_scan2(a, b, ta, tb, lds);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        if (i0 + j < n) totals[i0 + j] = make_uint2(a, b);
        a += v[j].x;
        b += v[j].y;
    }
    if (threadIdx.x == 0) group_totals[blockIdx.x] = make_uint2(ta, tb);
}

// group_totals[0, m) -> their exclusive scan as 64-bit bases, by one workgroup: thread t takes the
// ceil(m / 256) consecutive groups from t * per on, so there is one path for every m; counts[0], [1] = the
// mesh's vertices and quads
__global__ __launch_bounds__(256) void k_mesh_scan2(const uint2* group_totals, uint32_t m, unsigned long long* bases,
                                                    unsigned long long* counts) {
    __shared__ unsigned long long sums[256][2];
    const uint32_t per = (m + 255u) / 256u, g0 = threadIdx.x * per;
    unsigned long long a = 0, b = 0;
    for (uint32_t j = 0; j < per && g0 + j < m; j++) { a += group_totals[g0 + j].x; b += group_totals[g0 + j].y; }
    sums[threadIdx.x][0] = a;
    sums[threadIdx.x][1] = b;
    __syncthreads();
    if (threadIdx.x == 0) {   // (256 additions: the scan of the threads' sums, serial)
        unsigned long long ra = 0, rb = 0;
        for (uint32_t t = 0; t < 256u; t++) {
            const unsigned long long xa = sums[t][0], xb = sums[t][1];
            sums[t][0] = ra;
            sums[t][1] = rb;
            ra += xa;
            rb += xb;
        }
        counts[0] = ra;
        counts[1] = rb;
    }
    __syncthreads();
    a = sums[threadIdx.x][0];
    b = sums[threadIdx.x][1];
    for (uint32_t j = 0; j < per && g0 + j < m; j++) {
        bases[2 * (size_t)(g0 + j)] = a;
        bases[2 * (size_t)(g0 + j) + 1] = b;
        a += group_totals[g0 + j].x;
        b += group_totals[g0 + j].y;
    }
}

// The block's base: its group's 64-bit base plus its scanned total inside the group (the sums stay below
// 2^32: rmr_extract_mesh refuses larger counts before this runs).
RMR_D void block_base(const uint2* totals, const unsigned long long* bases, uint32_t& vbase, uint32_t& qbase) {
    const uint2 t = totals[blockIdx.x];
    const uint32_t g = blockIdx.x / kScanGroup;
    vbase = (uint32_t)bases[2 * (size_t)g] + t.x;
    qbase = (uint32_t)bases[2 * (size_t)g + 1] + t.y;
}

__global__ __launch_bounds__(256) void k_mesh_vertices(Lattice L, const float* dist, float iso, const uint8_t* flags,
                                                       const uint2* totals, const unsigned long long* bases,
                                                       uint32_t* cell_vertex, float* vertices) {
    __shared__ uint32_t lds[4][2];
    const uint32_t k = blockIdx.x * kMeshBlock + threadIdx.x;
    const uint32_t f = k < L.n_points ? flags[k] : 0u;
    uint32_t vr, qr, vt, qt, vbase, qbase;
    block_ranks(f, vr, qr, vt, qt, lds);
    if (!(f & kMeshActive)) return;
    block_base(totals, bases, vbase, qbase);
    const uint32_t v = vbase + vr;
    cell_vertex[k] = v;
    int ix, iy, iz;
    point_of(L, k, ix, iy, iz);
    float d[8], out[3];
    load_corners(dist, L, k, d);
    mesh_cell_vertex(d, iso, lattice_coord(L.ox, ix, L.spacing), lattice_coord(L.oy, iy, L.spacing),
                     lattice_coord(L.oz, iz, L.spacing), L.spacing, out);
    float* o = vertices + 3 * (size_t)v;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}

__global__ __launch_bounds__(256) void k_mesh_quads(Lattice L, const uint8_t* flags, const uint2* totals,
                                                    const unsigned long long* bases, const uint32_t* cell_vertex, uint4* quads) {
    __shared__ uint32_t lds[4][2];
    const uint32_t k = blockIdx.x * kMeshBlock + threadIdx.x;
    const uint32_t f = k < L.n_points ? flags[k] : 0u;
    uint32_t vr, qr, vt, qt, vbase, qbase;
    block_ranks(f, vr, qr, vt, qt, lds);
    if (!quads_of(f)) return;
    block_base(totals, bases, vbase, qbase);
    const uint32_t stride[3] = {1u, (uint32_t)L.nx, (uint32_t)L.nx * (uint32_t)L.ny};
    const bool lower_in = (f & kMeshLowerInside) != 0u;
    uint32_t q = qbase + qr;
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        if (!(f & (kMeshEdgeX << ax))) continue;
        uint32_t c[4];
        mesh_quad_cells(k, ax, stride, c);   // (an emitting edge is interior: k - su - sv >= 0, all four cells active)
        const uint32_t v0 = cell_vertex[c[0]], v1 = cell_vertex[c[1]], v2 = cell_vertex[c[2]], v3 = cell_vertex[c[3]];
        quads[q++] = lower_in ? make_uint4(v0, v1, v2, v3) : make_uint4(v3, v2, v1, v0);
    }
}

// Whole waves: hit_normal's loop exits are wave-uniform, lanes past the last vertex take part without a vertex.
template <int NP>
__global__ __launch_bounds__(256) void k_mesh_attr(KParams P, const float* vertices, uint32_t n_vertices, float* normals, float* ids) {
    using MAP = TableMap<NP>;
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    const bool have = v < n_vertices;
    V3 pos = v3(0.0f, 0.0f, 0.0f);
    if (have) pos = v3(vertices[3 * (size_t)v], vertices[3 * (size_t)v + 1], vertices[3 * (size_t)v + 2]);
    if (normals) {   // (a kernel argument: uniform)
        const V3 n = hit_normal<MAP>(P, have, pos);
        if (have) { normals[3 * (size_t)v] = n.x; normals[3 * (size_t)v + 1] = n.y; normals[3 * (size_t)v + 2] = n.z; }
    }
    if (ids && have) ids[v] = MAP::eval(P, pos).y;
}

// ---- launches --------------------------------------------------------------------------------------
namespace {
Lattice lattice_of(const rmr_volume_desc& d) {
    Lattice L;
    L.ox = d.origin[0]; L.oy = d.origin[1]; L.oz = d.origin[2]; L.spacing = d.spacing;
    L.nx = d.n[0]; L.ny = d.n[1]; L.nz = d.n[2];
    L.n_points = (uint32_t)((uint64_t)d.n[0] * (uint64_t)d.n[1] * (uint64_t)d.n[2]);   // (<= 2^30: rmr_check_volume)
    return L;
}
}  // namespace

#define RMR_VOLUME_SWITCH(NPV, CALL)     \
    switch (NPV) {                       \
    case 4: CALL(4); break;              \
    case 8: CALL(8); break;              \
    case 0: CALL(0); break;              \
    case -2: CALL(-2); break;            \
    default: CALL(-1); break;            \
    }

uint32_t mesh_blocks(const rmr_volume_desc& d) { return (lattice_of(d).n_points + kMeshBlock - 1u) / kMeshBlock; }
uint32_t mesh_scan_groups(uint32_t blocks) { return (blocks + kScanGroup - 1u) / kScanGroup; }

// d: a descriptor rmr_check_volume accepts; grid_cap: rmr_set_query_grid (0: one thread per point)
hipError_t launch_sample_volume(const KParams& P, int np, const rmr_volume_desc& d, float* dist, float* id, int grid_cap,
                                hipStream_t s) {
    const Lattice L = lattice_of(d);
    unsigned g = mesh_blocks(d);   // (<= 2^22 blocks)
    if (grid_cap > 0 && (unsigned)grid_cap < g) g = (unsigned)grid_cap;
#define RMR_SAMPLE(NPV)                                                    \
    if (id) k_sample_volume<NPV, true><<<g, 256, 0, s>>>(P, L, dist, id);  \
    else k_sample_volume<NPV, false><<<g, 256, 0, s>>>(P, L, dist, id)
    RMR_VOLUME_SWITCH(np, RMR_SAMPLE);
#undef RMR_SAMPLE
    return hipGetLastError();
}

// flags: n_points bytes; totals: mesh_blocks() uint2; group_totals: mesh_scan_groups() uint2; bases: 2 words
// per group; counts: 2 words
hipError_t launch_mesh_count(const rmr_volume_desc& d, const float* dist, float iso, uint8_t* flags, uint2* totals,
                             uint2* group_totals, unsigned long long* bases, unsigned long long* counts, hipStream_t s) {
    const Lattice L = lattice_of(d);
    const uint32_t blocks = mesh_blocks(d), groups = mesh_scan_groups(blocks);
    k_mesh_classify<<<blocks, 256, 0, s>>>(L, dist, iso, flags, totals);
    k_mesh_scan1<<<groups, 256, 0, s>>>(totals, blocks, group_totals);
    k_mesh_scan2<<<1, 256, 0, s>>>(group_totals, groups, bases, counts);
    return hipGetLastError();
}

// vertices: 3 floats per vertex, quads: 4 indices per quad, as counted; cell_vertex: n_points words
hipError_t launch_mesh_emit(const rmr_volume_desc& d, const float* dist, float iso, const uint8_t* flags, const uint2* totals,
                            const unsigned long long* bases, uint32_t* cell_vertex, float* vertices, uint32_t* quads,
                            hipStream_t s) {
    const Lattice L = lattice_of(d);
    const uint32_t blocks = mesh_blocks(d);
    k_mesh_vertices<<<blocks, 256, 0, s>>>(L, dist, iso, flags, totals, bases, cell_vertex, vertices);
    if (quads) k_mesh_quads<<<blocks, 256, 0, s>>>(L, flags, totals, bases, cell_vertex, (uint4*)quads);
    return hipGetLastError();
}

// normals and / or ids (null: not asked for) at the n_vertices vertices
hipError_t launch_mesh_attr(const KParams& P, int np, const float* vertices, uint32_t n_vertices, float* normals, float* ids,
                            hipStream_t s) {
    if (n_vertices == 0 || (!normals && !ids)) return hipSuccess;
    const unsigned g = (n_vertices + 255u) / 256u;
#define RMR_ATTR(NPV) k_mesh_attr<NPV><<<g, 256, 0, s>>>(P, vertices, n_vertices, normals, ids)
    RMR_VOLUME_SWITCH(np, RMR_ATTR);
#undef RMR_ATTR
    return hipGetLastError();
}

}  // namespace rmr
