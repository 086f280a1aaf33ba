// accel.hpp — what a scene load and a launch work out on the host before any HIP call: the map class,
// the shading kinds, the packed primitives, the BVH, the candidate grid, the escape boxes and the error
// constants the kernels' exactness rests on (SceneAccel), and the launch geometry (sample chunking,
// grid size, grouping of deferred calls, tile lists). Pure functions of their arguments: no HIP runtime
// call, no context, no environment read (the diagnostic library's switches arrive as AccelOptions), so
// all of it runs in a CPU test (accel_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "grid.hpp"
#include "scene.hpp"

namespace rmr {

// Scenes of more than kMaxLoopPrims spheres/boxes use the exact-culling BVH map (map_bvh in
// rmr_trace.h): median-split hierarchy over the primitives' boxes, leaves of <= 8, pre-order with
// skip links; the primitives are stored in leaf order with their scene index (the id tie-break).
constexpr size_t kMaxLoopPrims = 32;

// The experiments' switches (librmr_diag.so reads them from the environment, rmr_api.cpp
// read_switches); the defaults are the release library's values.
struct AccelOptions {
    size_t max_esc_boxes = 32;     // RMR_ESC_BOXES
    // RMR_BVH_LEAF; csg256 4 spp: 2 / 3 / 4 / 6 / 8 / 12 / 16 -> 37.0 / 36.1 / 34.1 / 33.3 / 32.9 / 33.1 / 33.6 ms
    int bvh_leaf = 8;
    bool grid = true;              // RMR_GRID
    // RMR_GRID_CELLS: 2^20 cells (round 3; csg256 1080p 8 spp, same process: 2^18 21.1, 2^19 20.2, 2^20
    // 19.9 ms, flat beyond; 16 MB of cell records, ~0.4 s to build on 16 host threads)
    double grid_cells = 1048576.0;
    double grid_pad = 0.5;         // RMR_GRID_PAD
};

struct SceneAccel {
    // map() specialisation: 4 / 8 unrolled, 0 loop, -2 BVH (sphere/box scenes by size), -1 general
    int map_np = -1;
    std::vector<DMat> dmats;      // shading kind per material id (shading_kinds)
    bool has_prog = true;         // a material needs the generic node interpreter
    // packed primitives: scene order padded to 8, or (BVH) leaf order with the scene index in type >> 8
    std::vector<DPrim> dprims;
    // BVH scenes: nodes in pre-order, leaf order -> scene index, the always-visited large primitives
    // (leaf indices [0, n_large)), the absolute part of the culling margin
    std::vector<BvhNode> nodes;
    std::vector<int> order;
    int n_large = 0;
    float bvh_margin = 1e-4f;
    bool small_spheres = false;   // every primitive past n_large is a sphere
    // candidate grid of the cache's full map() (grid.hpp); grid_cells: the device records (the host
    // record plus the list's first four entries inline, so most full-map lanes read their candidates
    // without a dependent list load)
    bool grid_on = false;
    CandidateGrid grid;
    std::vector<uint4> grid_cells;
    // escape bound (rmr_trace.h ray_exit): <= max_esc_boxes boxes covering every primitive (lo.xyz,
    // hi.xyz), not yet inflated (escape_inflation); empty: none
    std::vector<float> esc_raw;
    bool esc_all = false;         // the scene has primitives and every one takes part (escape_prim)
    // Three scene extents, each with the rounding of what it feeds:
    double esc_extent = 0.0;      // max_k |c_k| + halfwidth_k over escaping primitives (Mandelbulb
                                  // included), in double: escape_inflation
    double grid_extent = 0.0;     // max |c|_inf + |r|_inf, the sum in double: build_candidate_grid's E
    float err_extent = 0.0f;      // max |c|_inf + |r|_inf, the sum in float: npc_eps0 and cert_k
    float am_r2 = 0.0f;           // KParams::am_r2
    float npc_eps0 = 0.0f;        // KParams::npc_eps0
    float cert_k = 0.0f;          // KParams::cert_k
};

// nullptr, or why the tables cannot be run (indices and program ranges out of bounds).
const char* validate_scene(const CompiledScene& s);
// Shading kinds of the RM1 materials: the single-node diffuse / emission materials run the fast
// shading path, every other defined material its node program.
std::vector<DMat> shading_kinds(const CompiledScene& s);
// A Mandelbulb primitive (sd_mandelbulb) takes part in the escape bound when it iterates at least once
// with a bailout >= 1.5: at |p - c| > bailout its loop stops at once with r = |p - c|, dr = 1, so its
// distance is 0.5 log(r) r >= 0.30 — the box c +- bailout then bounds everything within 0.001 of it.
bool escape_prim(const rmr_prim& q);
DPrim pack_prim(const rmr_prim& p, int scene_index);

SceneAccel build_scene_accel(const CompiledScene& s, const AccelOptions& opt = AccelOptions());

// The nearest-primitive cache kernel's class: one cached primitive per lane when the cache's full
// map() runs through the candidate grid (csg256: 21.5 -> 17.4 ms per 4 spp against two), two with the
// BVH full map; sphere-only candidates when every primitive the grid lists is a sphere.
struct CacheFacts { int npc_k; bool npc_spheres; };
CacheFacts cache_kernel_facts(const SceneAccel& a, bool grid_built);

// The launch's escape bound (rmr_trace.h ray_exit): the escape boxes inflated by 0.002 + 2^-16 (|eye| +
// 2E + 3 maxDist) >= 0.001 + 8 x the float error of a distance at any point a march reaches
// (|p| <= |eye| + E + 3 maxDist) + the rounding of the slab parameters
double escape_inflation(const float eye[3], double esc_extent, float max_dist);
std::vector<float> inflate_escape_boxes(const std::vector<float>& raw, double infl);
// KParams::trail_eps_hi of a launch with the escape bound on (rmr_trail_rule.h: the derivation of B): RU(2^-17
// (B + 0.002 + E) + 2^-60) with B = (max(|org|_inf, esc_extent + infl) + 0.01)(1 + 2^-15), E = err_extent;
// +inf where that is not a finite float
float trail_eps_bound(const float org[3], double esc_extent, double infl, float err_extent);

// ---- launch planning ----

// Samples per launch of `nspp` samples over `plane` units each, and whether the launches may go to
// the launch slots.
struct SamplePlan { size_t per_launch; bool slotted; };
// unit_bytes: what a unit of a launch holds in the budget's buffers: its sample (16), and for a
// ray-source launch its ray record as well (rmr_camera.hpp kRayRecordBytes)
SamplePlan plan_samples(size_t plane, uint32_t nspp, size_t samp_budget, int launch_streams, size_t unit_bytes = 16);

// Workgroups of a launch of n_units, and the units a wave claims at a time (0: the kernel's chunk).
struct GridPlan { int grid; uint32_t chunk_units; };
GridPlan plan_grid(uint64_t n_units, int full_grid, int reserve, int waves_per_block, int kernel_chunk,
                   int small_chunk, int max_bounces, int grid_per_cu, int kernel_mode);

// The 8x8 tiles covering [x0, x1) x [y0, y1), row by row from (x0, y0).
std::vector<TileXY> rect_tiles(int x0, int y0, int x1, int y1);
// rmr_render_tiles' list: the 8x8 tiles of each tile_size x tile_size tile, clipped to the image.
std::vector<TileXY> expand_tiles(const int32_t* tiles_xy, int n_tiles, int tile_size, int W, int H);
// Clamp a pixel rect to the image; false when nothing is left.
bool clamp_rect(int W, int H, int& x0, int& y0, int& x1, int& y1);

// Deferred one-sample calls (rmr_render): per pixel rect the consecutive samples requested so far.
struct DeferredCall { int x0, y0, x1, y1; uint32_t s0; std::vector<float> times; };
// One launch: a rect, its first sample index and its seeds (pointing into a DeferredCall's times).
struct CallLaunch { int x0, y0, x1, y1; uint32_t s0; const float* times; uint32_t n; };
std::vector<CallLaunch> group_deferred(const std::vector<DeferredCall>& d);

}  // namespace rmr
