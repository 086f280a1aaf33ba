// accel_test.cpp — CPU checks of the scene acceleration and launch planning (accel.hpp), linked with the
// HIP-free units only (scene.cpp, grid.cpp, accel.cpp). `make accel_test` / `make accel_test_san`
// (address + undefined-behaviour sanitizers); tests/test_accel_cpu.py runs both.
//   accel_test ROOT            check everything against properties stated here and against the record
//                              tests/golden/accel_record.json; exit status 1 on any failure
//   accel_test ROOT --record   print the record of the scenes (kept from the parent's code: the program
//                              must go on reproducing it, so regenerate it only for a deliberate change)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <random>
#include <set>
#include <sstream>
#include <string>
#include <tuple>

#include "accel.hpp"

using namespace rmr;

static int g_fail = 0;
static std::string g_where;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            if (++g_fail <= 40) std::printf("FAIL %s: %s (line %d)\n", g_where.c_str(), #cond, __LINE__); \
        }                                                                                            \
    } while (0)

// ---- sha256 (FIPS 180-4) ----
static std::string sha256(const void* data, size_t len) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
        0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
        0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
        0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
        0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    std::string m((const char*)data, len);
    m.push_back((char)0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int i = 7; i >= 0; i--) m.push_back((char)(((uint64_t)len * 8) >> (8 * i)));
    auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
    for (size_t at = 0; at < m.size(); at += 64) {
        uint32_t w[64];
        for (int i = 0; i < 16; i++)
            w[i] = ((uint32_t)(uint8_t)m[at + 4 * i] << 24) | ((uint32_t)(uint8_t)m[at + 4 * i + 1] << 16) |
                   ((uint32_t)(uint8_t)m[at + 4 * i + 2] << 8) | (uint32_t)(uint8_t)m[at + 4 * i + 3];
        for (int i = 16; i < 64; i++) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; i++) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    char out[65];
    for (int i = 0; i < 8; i++) std::snprintf(out + 8 * i, 9, "%08x", h[i]);
    return out;
}
template <class T>
static std::string digest(const std::vector<T>& v) { return sha256(v.data(), v.size() * sizeof(T)); }

static std::string read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::printf("cannot read %s\n", path.c_str()); std::exit(2); }
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

struct Case { std::string name, path; int variant; };
static std::vector<Case> cases() {
    std::vector<Case> c;
    for (const char* n : {"cornell5", "csg64", "csg256", "csg_nodes", "mandelbulb", "sphere1", "empty"})
        c.push_back({n, std::string("scenes/") + n + ".scene", RMR_VARIANT_RM1});
    for (const char* n : {"default", "glass_test", "multilight"})
        c.push_back({n, std::string("tests/golden/scenes/") + n + ".scene", RMR_VARIANT_RM1});
    c.push_back({"simple", "tests/golden/scenes/simple.scene", RMR_VARIANT_RM2});
    c.push_back({"builtin_rm3", "", RMR_VARIANT_RM3});
    return c;
}
static CompiledScene load(const std::string& root, const Case& c) {
    return c.path.empty() ? builtin_scene(c.variant) : compile_scene(read_file(root + "/" + c.path), c.variant);
}

// ---- the record: digests of the arrays, the scalars as hex floats ----
static std::map<std::string, std::string> record_of(const SceneAccel& a) {
    char buf[64];
    std::map<std::string, std::string> r;
    r["nodes"] = digest(a.nodes);
    r["order"] = digest(a.order);
    r["dprims"] = digest(a.dprims);
    r["dmats"] = digest(a.dmats);
    r["esc_raw"] = digest(a.esc_raw);
    auto num = [&](const char* k, double v) { std::snprintf(buf, sizeof buf, "%a", v); r[k] = buf; };
    num("map_np", a.map_np); num("has_prog", a.has_prog); num("n_large", a.n_large);
    num("n_nodes", (double)a.nodes.size()); num("n_dprims", (double)a.dprims.size());
    num("n_esc", (double)(a.esc_raw.size() / 6)); num("esc_all", a.esc_all); num("small_spheres", a.small_spheres);
    num("bvh_margin", a.bvh_margin); num("esc_extent", a.esc_extent); num("grid_extent", a.grid_extent);
    num("err_extent", a.err_extent); num("am_r2", a.am_r2); num("npc_eps0", a.npc_eps0); num("cert_k", a.cert_k);
    return r;
}

// ---- BVH ----
static float halfwidth(const rmr_prim& p, int k) { return p.type == RMR_PRIM_SPHERE ? std::fabs(p.r[0]) : std::fabs(p.r[k]); }

static void check_subtree(const CompiledScene& s, const SceneAccel& a, int i, std::vector<int>& anc, std::vector<int>& seen_leaf) {
    const auto& N = a.nodes;
    CHECK(i >= 0 && (size_t)i < N.size());
    if (i < 0 || (size_t)i >= N.size()) return;
    const BvhNode& nd = N[(size_t)i];
    anc.push_back(i);
    if (nd.count != 0) {   // leaf
        CHECK(nd.skip == i + 1);
        CHECK(nd.count <= 8 && nd.count >= 1 && nd.first >= 0 && (size_t)(nd.first + nd.count) <= a.order.size());
        seen_leaf.push_back(i);
        for (int k = nd.first; k < nd.first + nd.count && (size_t)k < a.order.size(); k++) {
            if (k > nd.first) CHECK(a.order[(size_t)k] > a.order[(size_t)k - 1]);
            const rmr_prim& p = s.prims[(size_t)a.order[(size_t)k]];
            for (int j : anc)
                for (int ax = 0; ax < 3; ax++) {
                    CHECK(N[(size_t)j].lo[ax] <= p.c[ax] - halfwidth(p, ax));
                    CHECK(N[(size_t)j].hi[ax] >= p.c[ax] + halfwidth(p, ax));
                }
        }
    } else {
        const int c1 = i + 1;
        CHECK((size_t)c1 < N.size());
        if ((size_t)c1 < N.size()) {
            const int c2 = N[(size_t)c1].skip;
            check_subtree(s, a, c1, anc, seen_leaf);
            CHECK(c2 > c1 && (size_t)c2 < N.size());
            if (c2 > c1 && (size_t)c2 < N.size()) {
                check_subtree(s, a, c2, anc, seen_leaf);
                CHECK(N[(size_t)c2].skip == nd.skip);   // skip = the end of the subtree
            }
        }
    }
    anc.pop_back();
}

static void check_bvh(const CompiledScene& s, const SceneAccel& a) {
    const size_t n = s.prims.size();
    CHECK(a.map_np == -2);
    CHECK(a.order.size() == n && a.dprims.size() == n);
    std::vector<int> sorted = a.order;
    std::sort(sorted.begin(), sorted.end());
    for (size_t k = 0; k < sorted.size(); k++) CHECK(sorted[k] == (int)k);   // a permutation
    // the large primitives: wider than 8 x the median width
    std::vector<double> w(n);
    for (size_t i = 0; i < n; i++) w[i] = 2.0 * std::max({halfwidth(s.prims[i], 0), halfwidth(s.prims[i], 1), halfwidth(s.prims[i], 2)});
    std::vector<double> ws = w;
    std::sort(ws.begin(), ws.end());
    int n_large = 0;
    for (size_t i = 0; i < n; i++) n_large += w[i] > 8.0 * ws[n / 2];
    CHECK(a.n_large == n_large);
    // always-visited leaves first
    size_t i = 0;
    int covered = 0;
    for (; i < a.nodes.size() && a.nodes[i].lo[0] <= -1e38f; i++) {
        const BvhNode& nd = a.nodes[i];
        CHECK(nd.count >= 1 && nd.count <= 4 && nd.first == covered && nd.skip == (int)i + 1);
        for (int ax = 0; ax < 3; ax++) CHECK(nd.lo[ax] <= -1e38f && nd.hi[ax] >= 1e38f);
        for (int k = nd.first; k < nd.first + nd.count; k++) CHECK(w[(size_t)a.order[(size_t)k]] > 8.0 * ws[n / 2]);
        covered += nd.count;
    }
    CHECK(covered == n_large);
    for (size_t j = i; j < a.nodes.size(); j++) CHECK(a.nodes[j].lo[0] > -1e38f);   // none later
    std::vector<int> anc, leaves;
    if (i < a.nodes.size()) {
        check_subtree(s, a, (int)i, anc, leaves);
        CHECK(a.nodes[i].skip == (int)a.nodes.size());
        int at = n_large;   // leaves in pre-order take consecutive runs of the leaf order
        for (int l : leaves) { CHECK(a.nodes[(size_t)l].first == at); at += a.nodes[(size_t)l].count; }
        CHECK(at == (int)n);
    } else {
        CHECK(n_large == (int)n);
    }
    for (size_t k = 0; k < a.dprims.size() && k < n; k++) {
        const DPrim& q = a.dprims[k];
        CHECK((q.type >> 8) == a.order[k]);
        const rmr_prim& p = s.prims[(size_t)a.order[k]];
        CHECK((q.type & 0xff) == p.type && q.mat_id == p.mat_id);
        for (int ax = 0; ax < 3; ax++) CHECK(q.c[ax] == p.c[ax] && q.r[ax] == p.r[ax]);
    }
}

// ---- escape boxes ----
static void check_escape(const CompiledScene& s, const SceneAccel& a) {
    CHECK(a.esc_raw.size() % 6 == 0 && a.esc_raw.size() / 6 <= 32);
    bool other = s.prims.empty();
    for (const rmr_prim& p : s.prims)
        other = other || (p.type != RMR_PRIM_SPHERE && p.type != RMR_PRIM_BOX && p.type != RMR_PRIM_MANDELBULB);
    if (other) { CHECK(a.esc_raw.empty()); CHECK(!a.esc_all || s.prims.empty()); return; }
    if (a.esc_raw.empty()) return;
    for (const rmr_prim& p : s.prims) {
        bool in = false;
        for (size_t b = 0; b < a.esc_raw.size() && !in; b += 6) {
            in = true;
            for (int ax = 0; ax < 3; ax++) {
                const float h = p.type == RMR_PRIM_MANDELBULB ? p.r[2] : halfwidth(p, ax);
                in = in && a.esc_raw[b + (size_t)ax] <= p.c[ax] - h && a.esc_raw[b + 3 + (size_t)ax] >= p.c[ax] + h;
            }
        }
        CHECK(in);
    }
}

static void check_inflation(std::mt19937_64& rng) {
    g_where = "escape_inflation";
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (int it = 0; it < 4000; it++) {
        const double scale = std::ldexp(1.0, (int)(u(rng) * 40) - 10);
        float eye[3] = {(float)((u(rng) - 0.5) * scale), (float)((u(rng) - 0.5) * scale), (float)((u(rng) - 0.5) * scale)};
        const double E = u(rng) * scale;
        const float md = (float)(u(rng) * scale);
        const double f0 = escape_inflation(eye, E, md);
        CHECK(f0 >= 0.002);
        float eye2[3] = {eye[0], eye[1], eye[2]};
        const int ax = it % 3;
        eye2[ax] = eye[ax] * 1.5f;   // farther from the origin on one axis
        CHECK(escape_inflation(eye2, E, md) >= f0);
        CHECK(escape_inflation(eye, E * 1.25 + 0.1, md) >= f0);
        CHECK(escape_inflation(eye, E, md * 1.5f + 0.1f) >= f0);
    }
    const float zero[3] = {0, 0, 0};
    CHECK(escape_inflation(zero, 0.0, 0.0f) == 0.002);
    const float e1[3] = {0, -65536.0f, 0};
    CHECK(escape_inflation(e1, 0.0, 0.0f) == 1.002);
    CHECK(escape_inflation(zero, 32768.0, 0.0f) == 1.002);
    const std::vector<float> bx = inflate_escape_boxes({-1, -2, -3, 1, 2, 3}, 0.5);
    CHECK(bx.size() == 6 && bx[0] == -1.5f && bx[1] == -2.5f && bx[2] == -3.5f && bx[3] == 1.5f && bx[4] == 2.5f && bx[5] == 3.5f);
}

// ---- launch plan ----
static void check_samples(size_t plane, uint32_t nspp, size_t budget, int streams) {
    const SamplePlan sp = plan_samples(plane, nspp, budget, streams);
    CHECK(sp.per_launch >= 1);
    if (sp.per_launch < 1) return;
    uint64_t total = 0;
    size_t max_n = 0;
    for (uint64_t k0 = 0; k0 < nspp; k0 += sp.per_launch) {   // the launch loop's partition
        const size_t n = (size_t)std::min<uint64_t>(sp.per_launch, nspp - k0);
        total += n;
        max_n = std::max(max_n, n);
        CHECK((uint64_t)n * plane < ((uint64_t)1 << 31));
        CHECK(n == 1 || (uint64_t)n * plane * 16 <= budget);
    }
    CHECK(total == nspp);
    if (sp.slotted) CHECK(streams >= 2 && (uint64_t)max_n * plane * 16 * (uint64_t)streams <= budget);
}

static void check_grid(uint64_t n_units, int full, int reserve, int wpb, int kchunk, int small, int bounces, int gpc, int mode) {
    const GridPlan g = plan_grid(n_units, full, reserve, wpb, kchunk, small, bounces, gpc, mode);
    if (mode != 0 || gpc > 0) {   // a fixed grid, the kernel's own chunk
        CHECK(g.grid == full && g.chunk_units == 0);
        return;
    }
    const int cap = std::max(1, full - reserve);
    CHECK(g.grid >= 1 && g.grid <= cap);
    CHECK(g.chunk_units == 0 || ((int)g.chunk_units >= small && (int)g.chunk_units < kchunk));
    const uint64_t ck = g.chunk_units ? g.chunk_units : (uint64_t)kchunk;
    if (g.grid < cap) CHECK((uint64_t)g.grid * (uint64_t)wpb * ck >= n_units);
    if (bounces < 2 || small == 0) CHECK(g.chunk_units == 0);
}

static void check_plan(std::mt19937_64& rng) {
    g_where = "launch plan";
    auto ri = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (int it = 0; it < 4000; it++) {
        const size_t plane = 64 * (size_t)ri(1, (it % 4 == 0) ? ((uint64_t)1 << 24) : 40000);
        const uint32_t nspp = (uint32_t)ri(1, (it % 5 == 0) ? 100000 : 300);
        const size_t budget = (size_t)ri(1, 64) << ri(10, 30);
        check_samples(plane, nspp, budget, (int)ri(0, 4));
        const int kchunk = ri(0, 1) ? 128 : 64;
        const int smalls[] = {0, 8, 16, 32, 64, 64, 64};
        check_grid(ri(1, (it % 3 == 0) ? (((uint64_t)1 << 31) - 1) : 1 << 20), (int)ri(1, 4096), (int)ri(0, 3) * 16,
                   (int)(1u << ri(0, 4)), kchunk, smalls[ri(0, 6)], (int)ri(0, 16), it % 7 == 0 ? (int)ri(1, 8) : 0,
                   it % 11 == 0 ? 1 : 0);
    }
    // planes dividing 2^31: the launches stay below it
    check_samples((size_t)1 << 20, 4096, (size_t)48 << 30, 2);
    check_samples((size_t)1 << 30, 3, (size_t)48 << 30, 2);
    // one 8x8 tile x 1 spp: one workgroup, the smallest claim
    check_samples(64, 1, (size_t)48 << 30, 2);
    SamplePlan sp = plan_samples(64, 1, (size_t)48 << 30, 2);
    CHECK(sp.per_launch == 1 && sp.slotted);
    check_grid(64, 1536, 0, 4, 128, 64, 16, 0, 0);
    GridPlan g = plan_grid(64, 1536, 0, 4, 128, 64, 16, 0, 0);
    CHECK(g.grid == 1 && g.chunk_units == 64);
    // 480x270 x 1 spp (60 x 34 tiles) on a 1,536-block grid: 64-unit claims on 510 workgroups of 4 waves
    check_grid(130560, 1536, 0, 4, 128, 64, 16, 0, 0);
    g = plan_grid(130560, 1536, 0, 4, 128, 64, 16, 0, 0);
    CHECK(g.grid == 510 && g.chunk_units == 64);
    g = plan_grid(130560, 1536, 0, 4, 128, 64, 1, 0, 0);   // single-bounce paths keep the kernel's chunk
    CHECK(g.grid == 255 && g.chunk_units == 0);
    g = plan_grid(130560, 1536, 32, 4, 128, 64, 16, 0, 1);   // the per-path kernel: the grid as given
    CHECK(g.grid == 1536 && g.chunk_units == 0);
    // 4K x 256 spp at 48 GiB: 480 x 270 tiles, 34 GB of planes, 2,123,366,400 units: one launch, unslotted
    const size_t plane4k = (size_t)480 * 270 * 64;
    check_samples(plane4k, 256, (size_t)48 << 30, 2);
    sp = plan_samples(plane4k, 256, (size_t)48 << 30, 2);
    CHECK(sp.per_launch == 256 && !sp.slotted);
    check_grid((uint64_t)plane4k * 256, 2048, 0, 4, 128, 64, 16, 0, 0);
    g = plan_grid((uint64_t)plane4k * 256, 2048, 0, 4, 128, 64, 16, 0, 0);
    CHECK(g.grid == 2048 && g.chunk_units == 0);
    // the lane-slot kernels: 6 workgroups per CU (their LDS; rmr_api.cpp takes the count from the loaded
    // code object's occupancy) and 64-unit chunks, so 256 CUs give the same 1,536-block grid
    check_grid((uint64_t)1920 * 1080 * 64, 256 * 6, 0, 4, 64, 64, 4, 0, 0);
    g = plan_grid((uint64_t)1920 * 1080 * 64, 256 * 6, 0, 4, 64, 64, 4, 0, 0);   // C2: the whole grid, whole chunks
    CHECK(g.grid == 1536 && g.chunk_units == 0);
    g = plan_grid(130560, 256 * 6, 0, 4, 64, 64, 16, 0, 0);   // 480x270 x 1 spp: one 64-unit chunk per wave
    CHECK(g.grid == 510 && g.chunk_units == 0);
    g = plan_grid(64 * 64 * 4, 256 * 6, 1 << 20, 4, 64, 64, 4, 0, 0);   // the grid reserved down to one block
    CHECK(g.grid == 1 && g.chunk_units == 0);
    g = plan_grid(64, 256 * 6, 0, 4, 64, 64, 4, 0, 0);   // one tile: a single claim
    CHECK(g.grid == 1 && g.chunk_units == 0);
    // tiles
    std::vector<TileXY> t = rect_tiles(3, 5, 20, 14);
    CHECK(t.size() == 6 && t[0].x == 3 && t[0].y == 5 && t[2].x == 19 && t[3].x == 3 && t[3].y == 13);
    const int32_t txy[] = {0, 0, 1, 1};
    t = expand_tiles(txy, 2, 16, 24, 40);   // the second tile is clipped to the 24-pixel width
    CHECK(t.size() == 6 && t[3].x == 8 && t[3].y == 8 && t[4].x == 16 && t[4].y == 16 && t[5].x == 16 && t[5].y == 24);
    int x0 = -4, y0 = 2, x1 = 100, y1 = 50;
    CHECK(clamp_rect(64, 48, x0, y0, x1, y1) && x0 == 0 && y0 == 2 && x1 == 64 && y1 == 48);
    x0 = 70; x1 = 90; y0 = 0; y1 = 10;
    CHECK(!clamp_rect(64, 48, x0, y0, x1, y1));
}

// ---- deferred grouping ----
// seed of sample `k` in seed family `fam` (rects of one family with the same run hold the same seeds)
static float seed_of(int fam, uint32_t k) { return (float)fam * 1000.0f + (float)k * 0.25f; }
static DeferredCall call(int x0, int y0, int x1, int y1, int fam, uint32_t s0, uint32_t n) {
    DeferredCall d{x0, y0, x1, y1, s0, {}};
    for (uint32_t k = 0; k < n; k++) d.times.push_back(seed_of(fam, s0 + k));
    return d;
}
// every (pixel, sample) of the calls exactly once, with its own seed
static void check_cover(const std::vector<DeferredCall>& d, const std::vector<CallLaunch>& L) {
    std::map<std::tuple<int, int, uint32_t>, float> want;
    for (const auto& e : d)
        for (int y = e.y0; y < e.y1; y++)
            for (int x = e.x0; x < e.x1; x++)
                for (size_t k = 0; k < e.times.size(); k++) want[std::make_tuple(x, y, e.s0 + (uint32_t)k)] = e.times[k];
    size_t got = 0;
    for (const auto& l : L)
        for (int y = l.y0; y < l.y1; y++)
            for (int x = l.x0; x < l.x1; x++)
                for (uint32_t k = 0; k < l.n; k++) {
                    auto it = want.find(std::make_tuple(x, y, l.s0 + k));
                    CHECK(it != want.end());
                    if (it == want.end()) continue;
                    CHECK(it->second == l.times[k]);
                    it->second = NAN;   // (a second visit fails the comparison above)
                    got++;
                }
    CHECK(got == want.size());
}

static void check_grouping(std::mt19937_64& rng) {
    g_where = "deferred grouping";
    auto ri = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    for (int it = 0; it < 300; it++) {
        // disjoint rects: cells of a partition of a 64x48 image by random cut lines, some left out
        std::set<int> cx = {0, 64}, cy = {0, 48};
        for (int k = ri(0, 4); k > 0; k--) cx.insert(ri(1, 63));
        for (int k = ri(0, 3); k > 0; k--) cy.insert(ri(1, 47));
        const std::vector<int> xs(cx.begin(), cx.end()), ys(cy.begin(), cy.end());
        std::vector<DeferredCall> d;
        for (size_t j = 0; j + 1 < ys.size(); j++)
            for (size_t i = 0; i + 1 < xs.size(); i++)
                if (ri(0, 5) != 0) d.push_back(call(xs[i], ys[j], xs[i + 1], ys[j + 1], ri(0, 1), (uint32_t)ri(0, 1), (uint32_t)ri(1, 3)));
        std::shuffle(d.begin(), d.end(), rng);
        const std::vector<CallLaunch> L = group_deferred(d);
        CHECK(L.size() <= d.size());
        check_cover(d, L);
    }
    // the reference's 4x4 grid, every rect holding the same samples: one launch over the frame
    std::vector<DeferredCall> d;
    for (int j = 0; j < 4; j++)
        for (int i = 0; i < 4; i++) d.push_back(call(i * 120, j * 68, (i + 1) * 120, std::min(270, (j + 1) * 68), 0, 5, 2));
    std::vector<CallLaunch> L = group_deferred(d);
    CHECK(L.size() == 1);
    if (L.size() == 1) CHECK(L[0].x0 == 0 && L[0].y0 == 0 && L[0].x1 == 480 && L[0].y1 == 270 && L[0].s0 == 5 && L[0].n == 2);
    check_cover(d, L);
    // one rect a sample ahead: no launch over the frame
    d[6] = call(d[6].x0, d[6].y0, d[6].x1, d[6].y1, 0, 5, 3);
    L = group_deferred(d);
    CHECK(L.size() > 1);
    for (const auto& l : L) CHECK(!(l.x0 == 0 && l.y0 == 0 && l.x1 == 480 && l.y1 == 270));
    check_cover(d, L);
    // rects off the 8-pixel lattice that do not fill their box: one by one
    d = {call(3, 3, 13, 13, 0, 0, 1), call(20, 3, 30, 13, 0, 0, 1), call(3, 20, 13, 30, 0, 0, 1)};
    L = group_deferred(d);
    CHECK(L.size() == 3);
    for (size_t k = 0; k < L.size() && k < 3; k++)
        CHECK(L[k].x0 == d[k].x0 && L[k].y0 == d[k].y0 && L[k].x1 == d[k].x1 && L[k].y1 == d[k].y1 && L[k].times == d[k].times.data());
    check_cover(d, L);
    CHECK(group_deferred({}).empty());
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: accel_test ROOT [--record]\n"); return 2; }
    const std::string root = argv[1];
    const bool write = argc > 2 && std::string(argv[2]) == "--record";
    AccelOptions opt;
    opt.grid = false;   // (the candidate grid has its own test, tests/test_grid_cpu.py; one case below)
    json::Value rec;
    if (!write) rec = json::parse(read_file(root + "/tests/golden/accel_record.json"));
    if (write) std::printf("{\n");
    bool saw_nonescaping = false, first = true;
    for (const Case& c : cases()) {
        g_where = c.name;
        const CompiledScene s = load(root, c);
        CHECK(validate_scene(s) == nullptr);
        const SceneAccel a = build_scene_accel(s, opt);
        const auto r = record_of(a);
        if (write) {
            std::printf("%s  \"%s\": {", first ? "" : ",\n", c.name.c_str());
            bool f2 = true;
            for (const auto& kv : r) { std::printf("%s\n    \"%s\": \"%s\"", f2 ? "" : ",", kv.first.c_str(), kv.second.c_str()); f2 = false; }
            std::printf("\n  }");
            first = false;
            continue;
        }
        const json::Value& want = rec.get(c.name);
        CHECK(want.is_object() && want.size() == r.size());
        for (const auto& kv : r) {
            if (want.get(kv.first).s != kv.second)
                std::printf("record %s.%s: %s, now %s\n", c.name.c_str(), kv.first.c_str(), want.get(kv.first).s.c_str(), kv.second.c_str());
            CHECK(want.get(kv.first).s == kv.second);
        }
        // the map class: sphere/box scenes by size, anything else general
        bool sb = !s.prims.empty();
        for (const rmr_prim& p : s.prims) sb = sb && (p.type == RMR_PRIM_SPHERE || p.type == RMR_PRIM_BOX);
        const size_t n = s.prims.size();
        CHECK(a.map_np == (!sb ? -1 : n <= 4 ? 4 : n <= 8 ? 8 : n <= 32 ? 0 : -2));
        if (c.name == "csg64" || c.name == "csg256") check_bvh(s, a);
        if (a.map_np != -2) {
            CHECK(a.dprims.size() == std::max<size_t>(8, n) && a.nodes.empty() && a.n_large == 0);
            for (size_t k = 0; k < a.dprims.size(); k++) CHECK(a.dprims[k].type == (k < n ? s.prims[k].type : 0));
        }
        check_escape(s, a);
        for (const rmr_prim& p : s.prims) saw_nonescaping = saw_nonescaping || p.type == RMR_PRIM_PROGRAM;
        const CacheFacts f0 = cache_kernel_facts(a, false), f1 = cache_kernel_facts(a, true);
        CHECK(f0.npc_k == 2 && !f0.npc_spheres);
        CHECK(f1.npc_k == (a.map_np == -2 ? 1 : 2));
    }
    if (write) { std::printf("\n}\n"); return 0; }
    g_where = "scenes";
    CHECK(saw_nonescaping);   // (csg_nodes: node-program objects)
    {
        // one non-escaping primitive among spheres and boxes: no escape boxes; a bad table is refused
        g_where = "cornell5 + program primitive";
        CompiledScene s = load(root, cases()[0]);
        CHECK(!build_scene_accel(s, opt).esc_raw.empty());
        s.prims[1].type = RMR_PRIM_PROGRAM;
        s.prims[1].prog_begin = s.prims[1].prog_end = 0;
        s.prims[1].dist_var = 0;
        const SceneAccel a = build_scene_accel(s, opt);
        CHECK(a.esc_raw.empty() && !a.esc_all && a.map_np == -1);
        s.prims[1].prog_end = (int)s.ops.size() + 1;
        CHECK(validate_scene(s) != nullptr);
    }
    {
        // csg64 through a small candidate grid, fewer escape boxes and smaller leaves (the experiments' switches)
        g_where = "csg64 options";
        const CompiledScene s = load(root, cases()[1]);
        AccelOptions o;
        o.grid_cells = 4096.0;
        o.max_esc_boxes = 4;
        o.bvh_leaf = 2;
        const SceneAccel a = build_scene_accel(s, o);
        CHECK(a.grid_on && a.grid_cells.size() == a.grid.cells.size() / 2 && !a.grid_cells.empty());
        CHECK(a.esc_raw.size() / 6 <= 4 && !a.esc_raw.empty());
        for (const BvhNode& nd : a.nodes) CHECK(nd.lo[0] <= -1e38f || nd.count <= 2);
        bool spheres = true;
        for (size_t k = (size_t)a.n_large; k < a.dprims.size(); k++) spheres = spheres && (a.dprims[k].type & 0xff) == RMR_PRIM_SPHERE;
        CHECK(cache_kernel_facts(a, a.grid_on).npc_spheres == spheres);
        check_escape(s, a);
    }
    std::mt19937_64 rng(20240607);
    check_inflation(rng);
    check_plan(rng);
    check_grouping(rng);
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("accel_test ok\n");
    return 0;
}
