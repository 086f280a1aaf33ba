// accel.cpp — scene acceleration and launch planning on the host (see accel.hpp).
#include "accel.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rmr {

const char* validate_scene(const CompiledScene& s) {
    for (const auto& p : s.prims) {
        if (p.type < RMR_PRIM_SPHERE || p.type > RMR_PRIM_MANDELBULB) return "bad prim type";
        if (p.type == RMR_PRIM_PROGRAM) {
            if (p.prog_begin < 0 || p.prog_end > (int)s.ops.size() || p.prog_begin > p.prog_end)
                return "prim program range out of bounds";
            if (p.dist_var < 0 || p.dist_var >= RMR_MAX_VARS) return "bad dist_var";
        }
    }
    const int nconst = (int)(s.consts.size() / 3);
    for (const auto& o : s.ops) {
        for (int i = 0; i < 7; i++) {
            const int r = o.in[i];
            if (r == RMR_OPND_NONE || r == RMR_OPND_P) continue;
            if (RMR_OPND_IS_CONST(r)) {
                if (RMR_OPND_CONST_INDEX(r) >= nconst) return "constant index out of range";
            } else if (r < 0 || r >= RMR_MAX_VARS) {
                return "var index out of range";
            }
        }
        for (int i = 0; i < 4; i++)
            if (o.out[i] >= RMR_MAX_VARS) return "var index out of range";
    }
    for (const auto& m : s.materials)
        if (m.defined && (m.prog_begin < 0 || m.prog_end > (int)s.ops.size())) return "material program range";
    if (s.variant == RMR_VARIANT_RM2 && (s.v2_begin < 0 || s.v2_end > (int)s.ops.size())) return "v2 program range";
    return nullptr;
}

std::vector<DMat> shading_kinds(const CompiledScene& s) {
    std::vector<DMat> dm(std::max<size_t>(1, s.materials.size()));
    for (size_t i = 0; i < s.materials.size(); i++) {
        const rmr_material& m = s.materials[i];
        DMat d{};
        d.kind = m.defined ? MAT_PROGRAM : MAT_NONE;
        if (m.defined && m.prog_end - m.prog_begin == 1 && m.inside_var < 0 && m.hit_var < 0) {
            const rmr_op& op = s.ops[(size_t)m.prog_begin];
            auto lit = [&](int ref, float* out) {
                if (!RMR_OPND_IS_CONST(ref)) return false;
                const int k = RMR_OPND_CONST_INDEX(ref);
                for (int j = 0; j < 3; j++) out[j] = s.consts[3 * (size_t)k + j];
                return true;
            };
            if (op.code == RMR_OP_M_DIFFUSE && m.color_var == op.out[0] && m.dir_var == op.out[1] &&
                op.out[0] != op.out[1] && lit(op.in[0], d.c))
                d.kind = MAT_DIFFUSE;
            else if (op.code == RMR_OP_M_EMISSION && m.color_var == op.out[0] && m.dir_var < 0 &&
                     lit(op.in[0], d.c) && lit(op.in[1], d.p)) {
                d.kind = MAT_EMISSION;
                // grayscale of p * vec3(1) without separateChannels (rmr_trace.h gray_ch, RM1:306-309):
                // x * 1 is exact, so this is the kernel's ((p.x + p.y) + p.z) / (1 + 1 + 1)
                const float sum = (d.p[0] + d.p[1]) + d.p[2];
                d.gray1 = sum / 3.0f;
            }
        }
        dm[i] = d;
    }
    return dm;
}

bool escape_prim(const rmr_prim& q) {
    if (q.type == RMR_PRIM_SPHERE || q.type == RMR_PRIM_BOX) return true;
    return q.type == RMR_PRIM_MANDELBULB && q.r[1] >= 1.0f && q.r[2] >= 1.5f && std::isfinite(q.r[2]);
}

DPrim pack_prim(const rmr_prim& p, int scene_index) {
    DPrim q{};
    for (int k = 0; k < 3; k++) { q.c[k] = p.c[k]; q.r[k] = p.r[k]; }
    q.type = p.type | (scene_index << 8);
    q.mat_id = p.mat_id;
    return q;
}

namespace {

float escape_halfwidth(const rmr_prim& q, int k) {
    if (q.type == RMR_PRIM_SPHERE) return std::fabs(q.r[0]);
    if (q.type == RMR_PRIM_MANDELBULB) return q.r[2];
    return std::fabs(q.r[k]);
}

// Escape boxes: each primitive's box for scenes of <= max_esc_boxes primitives; for BVH scenes a cut
// of the hierarchy (the always-visited large primitives individually, then the node with the largest
// box split until max_esc_boxes boxes). Their union covers every primitive.
void build_escape_boxes(const CompiledScene& s, SceneAccel& a, size_t kMaxEscBoxes) {
    a.esc_raw.clear();
    if (!a.esc_all || (a.map_np == -1 && s.prims.size() > kMaxEscBoxes)) return;
    auto prim_box = [&](const rmr_prim& q, float* b) {
        for (int k = 0; k < 3; k++) {
            const float h = escape_halfwidth(q, k);
            b[k] = q.c[k] - h;
            b[3 + k] = q.c[k] + h;
        }
    };
    float b[6];
    if (a.map_np != -2 || s.prims.size() <= kMaxEscBoxes) {   // one box per primitive
        for (const rmr_prim& q : s.prims) {
            prim_box(q, b);
            a.esc_raw.insert(a.esc_raw.end(), b, b + 6);
        }
        return;
    }
    // BVH scene: nodes are in pre-order (first child = next node, second child = that node's skip);
    // leaves of the always-visited list have infinite bounds: use their primitives' own boxes
    std::vector<int> cut;
    for (size_t i = 0; i < a.nodes.size();) {
        const BvhNode& nd = a.nodes[i];
        if (nd.lo[0] <= -1e38f) {   // always-visited leaf of large primitives
            for (int k = nd.first; k < nd.first + nd.count; k++) {
                prim_box(s.prims[(size_t)(a.order[(size_t)k])], b);
                a.esc_raw.insert(a.esc_raw.end(), b, b + 6);
            }
            i = (size_t)nd.skip;
            continue;
        }
        cut.push_back((int)i);   // root of the remaining hierarchy
        break;
    }
    while (!cut.empty() && a.esc_raw.size() / 6 + cut.size() < kMaxEscBoxes) {
        // split the internal node of the cut with the largest box
        int best = -1;
        float bestv = -1.0f;
        for (size_t q = 0; q < cut.size(); q++) {
            const BvhNode& nd = a.nodes[(size_t)cut[q]];
            if (nd.count != 0) continue;
            const float v = (nd.hi[0] - nd.lo[0]) * (nd.hi[1] - nd.lo[1]) * (nd.hi[2] - nd.lo[2]);
            if (v > bestv) { bestv = v; best = (int)q; }
        }
        if (best < 0) break;
        const int i = cut[(size_t)best];
        cut[(size_t)best] = i + 1;
        cut.push_back(a.nodes[(size_t)(i + 1)].skip);
    }
    for (int i : cut) {
        const BvhNode& nd = a.nodes[(size_t)i];
        for (int k = 0; k < 3; k++) { b[k] = nd.lo[k]; b[3 + k] = nd.hi[k]; }
        a.esc_raw.insert(a.esc_raw.end(), b, b + 6);
    }
}

// max |c|_inf + |r|_inf over the primitives, the sum rounded to T
template <class T>
T scene_extent(const CompiledScene& s) {
    T E = 0;
    for (const rmr_prim& q : s.prims) {
        const float rr = q.type == RMR_PRIM_SPHERE ? std::fabs(q.r[0])
                                                   : std::max({std::fabs(q.r[0]), std::fabs(q.r[1]), std::fabs(q.r[2])});
        E = std::max(E, (T)std::max({std::fabs(q.c[0]), std::fabs(q.c[1]), std::fabs(q.c[2])}) + (T)rr);
    }
    return E;
}

struct BvhItem {
    float lo[3], hi[3], cen[3];
    int idx;
};

void bvh_build(std::vector<BvhItem>& it, int l, int r, int leaf_size, std::vector<BvhNode>& nodes, std::vector<int>& order) {
    const int me = (int)nodes.size();
    nodes.push_back(BvhNode{});
    BvhNode nd{};
    for (int k = 0; k < 3; k++) { nd.lo[k] = 3.0e38f; nd.hi[k] = -3.0e38f; }
    float clo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, chi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (int i = l; i < r; i++)
        for (int k = 0; k < 3; k++) {
            nd.lo[k] = std::min(nd.lo[k], it[i].lo[k]);
            nd.hi[k] = std::max(nd.hi[k], it[i].hi[k]);
            clo[k] = std::min(clo[k], it[i].cen[k]);
            chi[k] = std::max(chi[k], it[i].cen[k]);
        }
    if (r - l <= leaf_size) {
        std::sort(it.begin() + l, it.begin() + r, [](const BvhItem& a, const BvhItem& b) { return a.idx < b.idx; });
        nd.first = (int)order.size();
        nd.count = r - l;
        for (int i = l; i < r; i++) order.push_back(it[i].idx);
    } else {
        int ax = 0;
        for (int k = 1; k < 3; k++)
            if (chi[k] - clo[k] > chi[ax] - clo[ax]) ax = k;
        const int mid = (l + r) / 2;
        std::nth_element(it.begin() + l, it.begin() + mid, it.begin() + r,
                         [ax](const BvhItem& a, const BvhItem& b) { return a.cen[ax] < b.cen[ax]; });
        nd.first = -1;
        nd.count = 0;
        bvh_build(it, l, mid, leaf_size, nodes, order);
        bvh_build(it, mid, r, leaf_size, nodes, order);
    }
    nd.skip = (int)nodes.size();
    nodes[(size_t)me] = nd;
}

// Bounding boxes of a BVH scene's primitives, and which are "large": primitives much larger than the
// typical one (ground planes, walls) would make every box above them cover the scene, so they go
// first, in an always-visited leaf (infinite bounds), which also gives the running minimum a small
// value early; the candidate grid lists only the others.
std::vector<BvhItem> bvh_items(const CompiledScene& s, std::vector<char>& is_large, float& extent) {
    std::vector<BvhItem> items;
    extent = 0.0f;
    for (size_t i = 0; i < s.prims.size(); i++) {
        const rmr_prim& p = s.prims[i];
        BvhItem b{};
        for (int k = 0; k < 3; k++) {
            const float h = (p.type == RMR_PRIM_SPHERE) ? std::fabs(p.r[0]) : std::fabs(p.r[k]);
            b.lo[k] = p.c[k] - h;
            b.hi[k] = p.c[k] + h;
            b.cen[k] = p.c[k];
            extent = std::max(extent, std::fabs(p.c[k]) + h);
        }
        b.idx = (int)i;
        items.push_back(b);
    }
    std::vector<float> ext;
    for (const auto& b : items) ext.push_back(std::max({b.hi[0] - b.lo[0], b.hi[1] - b.lo[1], b.hi[2] - b.lo[2]}));
    std::vector<float> sorted_ext = ext;
    is_large.assign(items.size(), 0);
    if (items.empty()) return items;
    std::nth_element(sorted_ext.begin(), sorted_ext.begin() + sorted_ext.size() / 2, sorted_ext.end());
    const float big = 8.0f * sorted_ext[sorted_ext.size() / 2];
    for (size_t i = 0; i < items.size(); i++) is_large[i] = ext[i] > big;
    return items;
}

void build_grid(SceneAccel& a, const AccelOptions& opt) {
    a.grid_on = false;
    if (!opt.grid) return;
    CandidateGrid& g = a.grid;
    if (!build_candidate_grid(a.dprims, a.n_large, a.grid_extent, opt.grid_cells, opt.grid_pad, g)) return;
    const size_t ncell = g.cells.size() / 2;
    if (ncell >= ((size_t)1 << 31)) return;   // the kernel's cell index is 32-bit (map_grid_npc)
    a.grid_cells.resize(ncell);
    for (size_t i = 0; i < ncell; i++) {
        const uint32_t x = g.cells[2 * i], off = x & 0xffffffu, cnt = x >> 24;
        uint32_t e[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < 4 && cnt != 255u && k < cnt; k++) e[k] = g.list[off + k];
        a.grid_cells[i] = make_uint4(x, g.cells[2 * i + 1], e[0] | (e[1] << 16), e[2] | (e[3] << 16));
    }
    a.grid_on = true;
}

void build_bvh(const CompiledScene& s, SceneAccel& a, const AccelOptions& opt) {
    std::vector<char> is_large;
    float extent = 0.0f;
    const std::vector<BvhItem> items = bvh_items(s, is_large, extent);
    std::vector<BvhItem> small, large;
    for (size_t i = 0; i < items.size(); i++) (is_large[i] ? large : small).push_back(items[i]);
    std::vector<BvhNode>& nodes = a.nodes;
    std::vector<int>& order = a.order;
    if (!large.empty()) {
        for (size_t at = 0; at < large.size(); at += 4) {  // leaves of <= 4, all always visited
            BvhNode nd{};
            for (int k = 0; k < 3; k++) { nd.lo[k] = -3.0e38f; nd.hi[k] = 3.0e38f; }
            nd.first = (int)order.size();
            nd.count = (int)std::min<size_t>(4, large.size() - at);
            for (int i = 0; i < nd.count; i++) order.push_back(large[at + (size_t)i].idx);
            nd.skip = (int)nodes.size() + 1;
            nodes.push_back(nd);
        }
    }
    if (!small.empty()) bvh_build(small, 0, (int)small.size(), opt.bvh_leaf, nodes, order);
    a.dprims.resize(order.size());
    for (size_t k = 0; k < order.size(); k++) a.dprims[k] = pack_prim(s.prims[(size_t)order[k]], order[k]);
    a.bvh_margin = 1e-4f + extent * 0x1p-16f;
    a.grid_extent = scene_extent<double>(s);
    a.n_large = (int)large.size();   // the always-visited leaves come first (leaf order 0 ..)
    a.small_spheres = true;
    for (const BvhItem& b : small) a.small_spheres = a.small_spheres && s.prims[(size_t)b.idx].type == RMR_PRIM_SPHERE;
    build_grid(a, opt);
}

}  // namespace

SceneAccel build_scene_accel(const CompiledScene& s, const AccelOptions& opt) {
    SceneAccel a;
    a.dmats = shading_kinds(s);
    a.has_prog = false;
    for (const auto& d : a.dmats)
        if (d.kind == MAT_PROGRAM) a.has_prog = true;
    // the map class, and the primitives packed for it
    bool simple = true;   // a sphere/box scene
    for (const auto& p : s.prims) simple = simple && (p.type == RMR_PRIM_SPHERE || p.type == RMR_PRIM_BOX);
    const size_t n = s.prims.size();
    a.map_np = !simple || n == 0 ? -1 : (n <= 4 ? 4 : (n <= 8 ? 8 : (n <= kMaxLoopPrims ? 0 : -2)));
    if (a.map_np == -2) {
        build_bvh(s, a, opt);
    } else {
        a.dprims.assign(std::max<size_t>(n, 8), DPrim{});
        for (size_t i = 0; i < n; i++) a.dprims[i] = pack_prim(s.prims[i], 0);
    }
    a.esc_all = n != 0;
    for (const rmr_prim& q : s.prims) {
        a.esc_all = a.esc_all && escape_prim(q);
        if (!escape_prim(q)) continue;
        for (int k = 0; k < 3; k++)
            a.esc_extent = std::max(a.esc_extent, std::fabs((double)q.c[k]) + (double)escape_halfwidth(q, k));
    }
    build_escape_boxes(s, a, opt.max_esc_boxes);
    a.am_r2 = 2.0f * max_sphere_radius(s);
    a.err_extent = scene_extent<float>(s);   // scale of the float error of a box/sphere distance
    a.npc_eps0 = a.err_extent * 0x1p-17f + 0x1p-60f;
    // rmr_trace.h am_normal_cert: (0.002 + 2R) 2^-20 + 2^-39 + 4 eps + 2 delta with eps the npc_eps
    // bound at |p|_inf <= E + 0.005 (a hit's probes), in double, widened by 2^-20 for the kernel
    // fma's rounding and rounded up to float
    const double eps = ((double)a.err_extent + 0.005) * 0x1p-17 + (double)a.npc_eps0;
    const double k0 = (0.002 + (double)a.am_r2) * 0x1p-20 + 0x1p-39 + 4.0 * eps + 2.0 * 0.0010001;
    a.cert_k = std::nextafter((float)(k0 * (1.0 + 0x1p-20)), INFINITY);
    return a;
}

CacheFacts cache_kernel_facts(const SceneAccel& a, bool grid_built) {
    const bool grid = a.map_np == -2 && grid_built;
    return CacheFacts{grid ? 1 : 2, grid && a.small_spheres};
}

double escape_inflation(const float eye[3], double esc_extent, float max_dist) {
    double e = 0.0;
    for (int k = 0; k < 3; k++) e = std::max(e, std::fabs((double)eye[k]));
    return 0.002 + std::ldexp(e + 2.0 * esc_extent + 3.0 * std::fabs((double)max_dist), -16);
}

float trail_eps_bound(const float org[3], double esc_extent, double infl, float err_extent) {
    double e = 0.0;
    for (int k = 0; k < 3; k++) e = std::max(e, std::fabs((double)org[k]));
    // every corner of an inflated box has |.|_inf <= esc_extent + infl
    const double B = (std::max(e, esc_extent + infl) + 0.01) * (1.0 + 0x1p-15);
    const double eps = std::ldexp(B + 0.002 + (double)err_extent, -17) + 0x1p-60;
    if (!(eps < 0x1p127)) return INFINITY;   // (a NaN or infinite coordinate included)
    return std::nextafter((float)eps, INFINITY);
}

std::vector<float> inflate_escape_boxes(const std::vector<float>& raw, double infl) {
    std::vector<float> bx(raw.size());
    for (size_t i = 0; i < bx.size(); i++)   // outward in double, then to float
        bx[i] = (float)((double)raw[i] + ((i % 6) < 3 ? -infl : infl));
    return bx;
}

SamplePlan plan_samples(size_t plane, uint32_t nspp, size_t samp_budget, int launch_streams, size_t unit_bytes) {
    size_t chunk = std::max<size_t>(1, samp_budget / (plane * unit_bytes));
    chunk = std::min<size_t>(chunk, nspp);
    // the trace kernel indexes units with 32 bits (atomic work counter included): < 2^31 per launch
    chunk = std::max<size_t>(1, std::min<size_t>(chunk, (((size_t)1 << 31) - 1) / plane));
    // slots for launches whose planes fit the budget shared between the slots (larger ones, C4's 34-GB
    // 4K 256-spp frame, run on the context's stream: one plane buffer of them is enough)
    const bool slotted = launch_streams >= 2 && plane * chunk * unit_bytes <= samp_budget / (size_t)launch_streams;
    return SamplePlan{chunk, slotted};
}

// A persistent grid no larger than the launch's work: one work chunk per wave at most (a 256x256 1-spp
// launch (C1) on the full grid: 0.47 ms, almost all of it waves that find no work; the per-path kernel
// takes one wave per 64 units as it is). Waves per block and units per chunk of the kernel that runs.
// A launch with less work than one chunk per wave of the grid (a tile of one sample: the reference's
// Graphics::Render call) takes smaller claims instead, down to small_chunk units, so its paths spread
// over more CUs rather than running after one another in a few waves. 480x270 tiles of one sample, same
// process (r06m_small_chunk.log), 64 against 128 units: Cornell-5 -21%, RM3 -7%, Mandelbulb -18%; 32 /
// 16 slower again. Single-bounce paths are too short for it (C1's 256x256 frame +6%): those launches
// keep the kernel's chunk.
GridPlan plan_grid(uint64_t n_units, int full_grid, int reserve, int waves_per_block, int kernel_chunk,
                   int small_chunk, int max_bounces, int grid_per_cu, int kernel_mode) {
    int grid = full_grid;
    uint32_t chunk_units = 0;
    if (kernel_mode == 0 && grid_per_cu <= 0) {
        const uint64_t wpb = (uint64_t)waves_per_block, kchunk = (uint64_t)kernel_chunk;
        const uint64_t avail = (uint64_t)std::max(1, full_grid - reserve);
        uint64_t ck = kchunk;
        if (small_chunk > 0 && max_bounces >= 2 && n_units < avail * wpb * kchunk)
            ck = std::min(kchunk, std::max<uint64_t>((uint64_t)small_chunk, (n_units + avail * wpb - 1) / (avail * wpb)));
        if (ck < kchunk) chunk_units = (uint32_t)ck;
        const uint64_t want = (n_units + wpb * ck - 1) / (wpb * ck);
        grid = (int)std::max<uint64_t>(1, std::min<uint64_t>(avail, want));
    }
    return GridPlan{grid, chunk_units};
}

std::vector<TileXY> rect_tiles(int x0, int y0, int x1, int y1) {
    std::vector<TileXY> t;
    for (int y = y0; y < y1; y += 8)
        for (int x = x0; x < x1; x += 8) t.push_back(TileXY{x, y});
    return t;
}

std::vector<TileXY> expand_tiles(const int32_t* tiles_xy, int n_tiles, int tile_size, int W, int H) {
    std::vector<TileXY> t;
    t.reserve((size_t)n_tiles * (tile_size / 8) * (tile_size / 8));
    for (int i = 0; i < n_tiles; i++) {
        const int bx = tiles_xy[2 * i] * tile_size, by = tiles_xy[2 * i + 1] * tile_size;
        for (int y = by; y < std::min(by + tile_size, H); y += 8)
            for (int x = bx; x < std::min(bx + tile_size, W); x += 8) t.push_back(TileXY{x, y});
    }
    return t;
}

bool clamp_rect(int W, int H, int& x0, int& y0, int& x1, int& y1) {
    auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
    x0 = clampi(x0, 0, W); x1 = clampi(x1, 0, W);
    y0 = clampi(y0, 0, H); y1 = clampi(y1, 0, H);
    return x1 > x0 && y1 > y0;
}

// Rects holding the same samples (same first index, same seeds) whose union is a rectangle go out as
// one launch over that rectangle (the reference's 4x4 grid, fixed or progressive: the whole grid in one
// launch); any other rect goes out as a launch of its own (a launch clips to one rect: a tile of a rect
// whose edge is off the 8-pixel grid reaches into its neighbour). Bitwise equal to the calls made one by
// one: each pixel gets the same samples with the same seeds in the same order, and the held rects are
// disjoint (rmr_render flushes before an overlapping call).
std::vector<CallLaunch> group_deferred(const std::vector<DeferredCall>& d) {
    std::vector<CallLaunch> out;
    std::vector<char> done(d.size(), 0);
    for (size_t i = 0; i < d.size(); i++) {
        if (done[i]) continue;
        std::vector<size_t> grp;
        int bx0 = d[i].x0, by0 = d[i].y0, bx1 = d[i].x1, by1 = d[i].y1;
        uint64_t area = 0;
        for (size_t j = i; j < d.size(); j++) {
            if (done[j] || d[j].s0 != d[i].s0 || d[j].times.size() != d[i].times.size() ||
                std::memcmp(d[j].times.data(), d[i].times.data(), d[i].times.size() * sizeof(float)) != 0)
                continue;
            grp.push_back(j);
            done[j] = 1;
            bx0 = std::min(bx0, d[j].x0); by0 = std::min(by0, d[j].y0);
            bx1 = std::max(bx1, d[j].x1); by1 = std::max(by1, d[j].y1);
            area += (uint64_t)(d[j].x1 - d[j].x0) * (uint64_t)(d[j].y1 - d[j].y0);
        }
        const uint32_t n = (uint32_t)d[i].times.size();
        if (area == (uint64_t)(bx1 - bx0) * (uint64_t)(by1 - by0)) {   // disjoint rects filling their box
            out.push_back(CallLaunch{bx0, by0, bx1, by1, d[i].s0, d[i].times.data(), n});
            continue;
        }
        for (size_t j : grp) out.push_back(CallLaunch{d[j].x0, d[j].y0, d[j].x1, d[j].y1, d[j].s0, d[j].times.data(), n});
    }
    return out;
}

}  // namespace rmr
