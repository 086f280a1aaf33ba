// rmr_api.cpp — the C ABI of librmr.so (include/rmr.h): the drop-in replacement for the
// reference's static `Graphics` backend (Graphics.h:15-134, Graphics.cpp:215-835).
//
// Ownership: the context owns its HIP stream, the scene tables in HBM, the per-sample radiance
// planes and (unless rmr_bind_accum is used) the RGBA32F accumulator. Host buffers passed in are
// caller-owned and copied. No exception crosses the boundary.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <initializer_list>
#include <new>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/rmr.h"
#include "rmr_internal.h"
#include "accel.hpp"
#include "adaptive.hpp"
#include "rmr_camera.hpp"
#include "rmr_ray_check.h"
#include "rmr_bake_rule.h"
#include "rmr_probe_rule.h"
#include "rmr_probe_vis_rule.h"
#include "rmr_jit.hpp"
#include "rmr_trail_rule.h"
#include "scene.hpp"
#include "temporal.hpp"
#include "tonemap.hpp"
#include "bloom.hpp"
#include "stage_state.hpp"

namespace rmr {
hipError_t launch_trace(const KParams& P, int variant, int np, bool prog, bool persistent, int grid, hipStream_t s);
hipError_t launch_fold(const KParams& P, hipStream_t s);
hipError_t launch_trace_rays(const KParams& P, const float4* rays, int variant, int np, bool prog, bool persistent,
                             int grid, hipStream_t s);
int trace_rays_occupancy(int variant, int np, bool prog, int* blocks_per_cu);
hipError_t launch_camera_rays(const KParams& P, const CamParams& C, float4* rays, hipStream_t s);
hipError_t launch_ray_exit(const KParams& P, const float* rays, float* out, int n, hipStream_t s);
hipError_t launch_display(const float4* accum, int img_w, int img_h, float cx, float cy, float zoom, float min_x,
                          float min_y, float max_x, float max_y, int scr_w, int scr_h, uint32_t* rgba8,
                          const float* thr, hipStream_t s);
int trace_occupancy(int variant, int np, bool prog, int* blocks_per_cu);
hipError_t launch_guides(const KParams& P, int np, float4* ray, float4* hit, float4* nrm, hipStream_t s);
hipError_t launch_atrous(const DenoisePass& A, bool tiled, hipStream_t s);
hipError_t launch_fold_half(const KParams& P, float4* half, hipStream_t s);
hipError_t launch_tile_error(const float4* A, const float4* B, int W, int H, float offset, float* out, hipStream_t s);
hipError_t launch_cast_rays(const KParams& P, int np, bool normals, const rmr_ray* rays, uint64_t n, rmr_hit* out,
                            unsigned long long* rejects, unsigned long long* first_bad, int grid_cap, hipStream_t s);
hipError_t launch_eval_map(const KParams& P, int np, const float* xyz, uint64_t n, float* out, int grid_cap, hipStream_t s);
hipError_t launch_pack_rays(const rmr_ray* rays, uint64_t n, uint64_t u0, uint32_t units, float extent, float4* rec,
                            unsigned long long* rejects, unsigned long long* first_bad, hipStream_t s);
hipError_t launch_unpack_rgba(const float4* samp, const float4* rec, float* out, uint32_t cnt, hipStream_t s);
hipError_t launch_aov(const KParams& P, const CamParams& C, int np, float4* state, bool restart, hipStream_t s);
hipError_t launch_aov_init(float4* state, size_t n_px, hipStream_t s);
hipError_t launch_aov_resolve(const float4* state, size_t n_px, float max_dist, float4* out, hipStream_t s);
uint32_t mesh_blocks(const rmr_volume_desc& d);
uint32_t mesh_scan_groups(uint32_t blocks);
hipError_t launch_sample_volume(const KParams& P, int np, const rmr_volume_desc& d, float* dist, float* id, int grid_cap,
                                hipStream_t s);
hipError_t launch_mesh_count(const rmr_volume_desc& d, const float* dist, float iso, uint8_t* flags, uint2* totals,
                             uint2* group_totals, unsigned long long* bases, unsigned long long* counts, hipStream_t s);
hipError_t launch_mesh_emit(const rmr_volume_desc& d, const float* dist, float iso, const uint8_t* flags, const uint2* totals,
                            const unsigned long long* bases, uint32_t* cell_vertex, float* vertices, uint32_t* quads,
                            hipStream_t s);
hipError_t launch_mesh_attr(const KParams& P, int np, const float* vertices, uint32_t n_vertices, float* normals, float* ids,
                            hipStream_t s);
hipError_t launch_bake_rays(const BakeList& B, uint64_t s0, uint32_t cnt, float4* rec, unsigned long long* rejects,
                            hipStream_t s);
hipError_t launch_bake_ray_list(const BakeList& B, rmr_ray* out, unsigned long long* rejects, hipStream_t s);
hipError_t launch_bake_ao(const KParams& P, int np, const BakeList& B, float ao_distance, uint64_t s0, uint32_t cnt,
                          float2* plane, unsigned long long* rejects, int grid_cap, hipStream_t s);
hipError_t launch_bake_fold(bool ao, const void* plane, const float4* rec, float4* state, uint64_t n, uint32_t nspp,
                            uint64_t s0, uint32_t cnt, float* out, hipStream_t s);
hipError_t launch_probe_rays(const KParams& P, int np, const ProbeList& B, uint64_t s0, uint32_t cnt, float4* rec,
                             unsigned long long* rejects, hipStream_t s);
hipError_t launch_probe_ray_list(const KParams& P, int np, const ProbeList& B, rmr_ray* out, unsigned long long* rejects,
                                 hipStream_t s);
hipError_t launch_probe_fold(int mapping, const float4* samp, const float4* rec, float4* state, uint64_t n, uint32_t nspp,
                             uint64_t s0, uint32_t cnt, float* out, hipStream_t s);
hipError_t launch_probe_lookup(const rmr_volume_desc& d, const float* sh, const float* points, const float* normals,
                               uint64_t n, float* out, unsigned long long* rejects, hipStream_t s);
hipError_t launch_probe_vis_cast(const KParams& P, int np, const ProbeList& B, const float* valid_sh, float range,
                                 uint64_t s0, uint32_t cnt, float4* rec, unsigned long long* rejects, hipStream_t s);
hipError_t launch_probe_vis_fold(const float4* rec, float* state, uint64_t n, uint32_t nspp, float range, uint64_t s0,
                                 uint32_t cnt, float* out, hipStream_t s);
hipError_t launch_probe_lookup_vis(const rmr_volume_desc& d, const float* sh, const float* vis, const float* points,
                                   const float* normals, uint64_t n, float bias, float* out, unsigned long long* rejects,
                                   hipStream_t s);
}  // namespace rmr

using rmr::CompiledScene;
using rmr::KParams;
using rmr::TileXY;

struct EventPair { hipEvent_t a, b, c; };

constexpr int kSlotGridReserve = 32;   // workgroups a slotted launch leaves free for the previous fold
// a-trous passes that run the LDS-tiled form (bit i: step 2^i); DESIGN.md §4.7 has the measurements
constexpr int kDenoiseTiledSteps = 3;
// the same for the variance-guided passes (rmr_denoise_var.hip); DESIGN.md §4.11
constexpr int kDenoiseVarTiledSteps = 3;
// samples per launch of the sampled AOVs' kernel (rmr_set_aov_launch_samples); DESIGN.md §4.15
constexpr int kAovLaunchSamples = 6;

struct rmr_ctx {
    int device = 0;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int W = 1024, H = 1024;               // GUI.cpp:201-208 defaults (Graphics.cpp:6 is overridden)
    int pend_W = 1024, pend_H = 1024;
    rmr_params params{};
    float view[15];
    bool view_set = false;
    CompiledScene scene;
    bool scene_loaded = false;
    // device tables
    rmr_prim* d_prims = nullptr;
    rmr_op* d_ops = nullptr;
    float* d_consts = nullptr;
    rmr_material* d_mats = nullptr;
    rmr_spectral* d_spec = nullptr;
    rmr_rm2_consts* d_rm2 = nullptr;
    rmr::DPrim* d_dprims = nullptr;
    rmr::DMat* d_dmats = nullptr;
    rmr::BvhNode* d_bvh = nullptr;
    // what the host works out per scene (accel.hpp); after the upload without the grid's arrays
    rmr::SceneAccel accel;
    KParams scene_kp{};                   // the launch parameters that only a scene load changes (scene_params)
    // escape bound (rmr_trace.h ray_exit): accel.esc_raw uploaded inflated by esc_infl_dev (which
    // depends on the view and maxDist)
    float* d_esc = nullptr;
    double esc_infl_dev = -1.0;
    float4* d_env = nullptr;              // envTex (rmr_set_env_map)
    float* d_srgb_thr = nullptr;          // rmr_display: sRGB decision points (256 floats)
    uint32_t* d_screen = nullptr;         // rmr_display: staging of a host screen image
    size_t screen_cap = 0;
    int env_w = 0, env_h = 0;
    // candidate grid of the cache's full map() (accel.grid_on; BVH scenes)
    uint4* d_grid = nullptr;
    uint16_t* d_grid_list = nullptr;
    int npc_ksel = 0;   // RMR_NPC_KSEL (experiments): the cache's primitives per lane, 0 = by the kernel class
    // buffers
    float4* d_accum = nullptr;
    bool accum_external = false;
    float4* d_samp = nullptr;
    size_t samp_cap = 0;
    // camera models and caller-supplied rays (rmr_camera.hip, rmr_trace.h RAYS): the
    // model (survives rmr_reload), and the ray buffer of the ray-source launches, kRayRecordBytes per unit
    // next to the sample planes (such launches run on the context's stream only, one after the other)
    rmr_camera_model camera{RMR_CAMERA_VIEW, 0.0f, 1.0f, 1.0f, 1.0f};
    float4* d_rays = nullptr;
    size_t rays_cap = 0;                  // units
    // first-hit and distance queries (rmr_query.hip), allocated at first use: the
    // counters (kQuery* words), and the host forms' device copies of the caller's list and result
    unsigned long long* d_query = nullptr;
    void* d_qin = nullptr;
    void* d_qout = nullptr;
    size_t qin_cap = 0, qout_cap = 0;     // bytes
    int query_grid = 0;                   // rmr_set_query_grid: 0 = one thread per ray / point
    // sampled AOVs (rmr_render_aov, rmr_aov.hip): the five state planes (one allocation,
    // W x H float4 each, at first use) and the five resolved planes (at the first resolve); freed at
    // rmr_reload, a scene load, rmr_set_image_size and rmr_destroy
    float4* d_aov = nullptr;
    float4* d_aov_res = nullptr;
    bool aov_rendered = false;            // an rmr_render_aov since the planes were allocated
    bool aov_res_valid = false;           // d_aov_res is (or is queued to be) the resolve of the current state
    uint64_t aov_samples = 0;             // a bound on every pixel's n: samples since the last whole-image restart
    int aov_launch_samples = kAovLaunchSamples;
    // the extracted mesh (rmr_extract_mesh, rmr_volume.hip): its buffers, sized exactly, and
    // the extraction's working memory (distances, flag bytes, cell numbers: grows only; block totals, group
    // totals, bases and the two counts in one allocation); freed at rmr_mesh_free, rmr_reload and rmr_destroy
    float* d_mesh_v = nullptr;
    float* d_mesh_n = nullptr;
    float* d_mesh_id = nullptr;
    uint32_t* d_mesh_q = nullptr;
    bool mesh_valid = false;
    int mesh_flags = 0;
    uint64_t mesh_nv = 0, mesh_nq = 0;
    void* d_mesh_dist = nullptr;
    void* d_mesh_flag = nullptr;
    void* d_mesh_cell = nullptr;
    void* d_mesh_scan = nullptr;
    size_t mesh_dist_cap = 0, mesh_flag_cap = 0, mesh_cell_cap = 0, mesh_scan_cap = 0;   // bytes
    // light baking (rmr_bake_points, rmr_bake.hip): the per-point state between launches (a
    // float4 per point, grows only, freed at rmr_reload and rmr_destroy); the host form's device copies live
    // in d_qin / d_qout. The mesh's bake (rmr_bake_mesh): colours [V][4] and ao [V], which go with the mesh,
    // whose lattice is kept for the origins' bound
    void* d_bake_state = nullptr;
    size_t bake_state_cap = 0;            // bytes
    float* d_mesh_rgba = nullptr;
    float* d_mesh_ao = nullptr;
    rmr_volume_desc mesh_desc{};
    int mesh_baked = 0;                   // RMR_BAKE_*: what rmr_bake_mesh has (queued) for the current mesh
    // irradiance probes (rmr_bake_probes, rmr_probe.hip): the per-probe state between launches
    // (a float4 per coefficient, grows only) and the field: one lattice and its [points][28] floats. Both are
    // freed by rmr_probe_field_free, rmr_reload and rmr_destroy
    void* d_probe_state = nullptr;
    size_t probe_state_cap = 0;           // bytes
    float* d_probe_field = nullptr;
    rmr_volume_desc probe_desc{};
    bool probe_valid = false;
    // the field's visibility (rmr_bake_probe_field_visibility, rmr_probe_vis.hip): [points][128]
    // floats and the range, dropped with the field and by every new field; the visibility bakes' running sums
    void* d_probe_vis_state = nullptr;
    size_t probe_vis_state_cap = 0;       // bytes
    float* d_probe_vis = nullptr;
    float probe_vis_range = 0.0f;
    bool probe_vis_valid = false;
    int probe_fold_mapping = 0;           // rmr_probe.hip launch_probe_fold (the diagnostic library's switch)
    // which of the output stages' images below are valid: the one place that says so (stage_state.hpp)
    rmr::StageState st;
    // first-hit guides and the preview denoiser (rmr_render_guides / rmr_denoise): three guide planes and
    // two filter images of W x H float4, allocated at first use, freed at rmr_reload / rmr_destroy
    float4* d_guide[3] = {nullptr, nullptr, nullptr};
    float4* d_dn[2] = {nullptr, nullptr};
    int output_source = RMR_OUTPUT_ACCUM; // what rmr_save_bmp / rmr_display* read
    int dn_tiled_steps = kDenoiseTiledSteps;   // bit i: pass i (step 2^i, i < 2) runs the LDS-tiled form
    // variance-guided mode (rmr_denoise_variance): the seed plane and two filter planes of
    // W x H floats, allocated at the first call, freed with the guide planes
    float* d_var[3] = {nullptr, nullptr, nullptr};
    int dnv_tiled_steps = kDenoiseVarTiledSteps;
    // temporal reprojection (rmr_temporal_accumulate): two pairs of history colour (W x H
    // float4) and count (W x H float) that the steps alternate between, and the history's HIT and NORMAL
    // planes; allocated at the first call, freed at rmr_reload / rmr_destroy
    float4* d_tcol[2] = {nullptr, nullptr};
    float* d_tn[2] = {nullptr, nullptr};
    float4* d_tguide[2] = {nullptr, nullptr};
    float t_view[15];                     // the view the history was made with
    bool t_keep = false;                  // diagnostic library (tools/temporal_time.py): a step leaves the history as it is
    // tone mapping and auto-exposure (rmr_tonemap): the tonemapped plane (W x H float4),
    // k_lum_hist's [kToneSlabRows][257] slab, the state and the meter's table of bin centres; allocated
    // at the first call, freed at rmr_reload / rmr_destroy
    float4* d_tm = nullptr;
    uint32_t* d_tm_slab = nullptr;
    rmr::ToneState* d_tm_state = nullptr;
    double* d_tm_lc = nullptr;
    double tm_lc[255];                    // the table's host copy (the source of its queued upload)
    int tm_used = 0;                      // what the last rmr_tonemap used: 0 none, 1 tm_ev / tm_scale, 2 the state
    double tm_ev = 0.0;
    float tm_scale = 1.0f;
    bool tm_fold = false;                 // diagnostic library (tools/tonemap_time.py): k_lum_hist folds equal bins
                                          // inside the wave (measured and not kept: DESIGN.md §4.13, Appendix A)
    // HDR bloom (rmr_bloom): the result plane (W x H float4) and the pyramid, one
    // allocation of eight levels (about a third of a plane); allocated at the first call, both or neither,
    // freed at rmr_reload / rmr_destroy
    float4* d_bl = nullptr;
    float4* d_bl_pyr = nullptr;
    int bl_tail = rmr::kBloomTailDefault; // the most pixels the tail kernel's levels hold together (diagnostic library: 0 = off)
    // per-tile error estimate and adaptive sampling (rmr_estimate.hip, adaptive.hpp)
    bool est_on = false;                  // every launch's fold is k_fold_half (rmr_set_error_estimate)
    bool est_valid = false;               // d_half holds the odd samples of everything in the accumulator
    bool rendered = false;                // something went into the accumulator since the last rmr_reload
    float4* d_half = nullptr;             // the half image B, W x H (allocated while est_on)
    float* d_tile_err = nullptr;          // ceil(H / 8) x ceil(W / 8) tile errors
    std::vector<uint32_t> sample_counts;  // per tile, of the last rmr_render_adaptive since rmr_reload
    // Launch slots (rmr_set_launch_streams): trace launches go round-robin to private streams, each with
    // its own sample planes and work queue, so a launch's drain (its last long paths on a nearly idle
    // chip) overlaps the next launch's start. Every fold stays on the context's stream, after its trace's
    // `done` event, in call order: a sync of the context's stream covers every trace queued before it,
    // and the accumulator sees the same running-mean order. A slot's planes and queue are reused once
    // the fold that read them (`freed`) is done.
    struct Slot {
        hipStream_t s = nullptr;
        float4* samp = nullptr;
        size_t cap = 0;
        unsigned long long* queue = nullptr;
        bool queue_dirty = true;
        hipEvent_t done = nullptr, freed = nullptr;
        bool in_use = false;
    };
    std::vector<Slot> slots;
    int launch_streams = 2;       // fewer than 2: every launch on the context's stream (rmr_create: 4 with
                                  // 8 or more hardware queues)
    int slot_reserve = kSlotGridReserve;   // workgroups a slotted launch leaves free (RMR_SLOT_RESERVE)
    size_t next_slot = 0;
    float4* last_samp = nullptr;  // the last launch's planes (rmr_trace_samples)
    hipEvent_t trace_end = nullptr;   // after the last trace launch, on its stream
    // device tile lists by content (tile_list): a list is uploaded once and reused by every later launch
    // with the same tiles (the reference's per-tile, per-sample calls; a rank's share each frame) with no
    // copy and no stream sync; least recently used entries go beyond kTileCacheEntries
    struct TileList { std::vector<TileXY> host; TileXY* dev; uint64_t hash; uint64_t used; };
    std::vector<TileList> tile_cache;
    uint64_t tile_clock = 0;
    // seeds of launches of more than one sample: a pinned host ring and its device twin, so the copy is
    // asynchronous (from the caller's pageable array hipMemcpyAsync had waited for the copy, i.e. for the
    // work queued before it); a one-sample launch passes its seed as a kernel argument (KParams::time1)
    float* d_times = nullptr;
    float* h_times = nullptr;
    size_t times_cap = 0, times_pos = 0;
    bool queue_dirty = false;   // a trace launch went out without the fold that zeroes the queue after it
    // deferred one-sample calls (rmr_render, the reference's Graphics::Render pattern): per pixel rect
    // the consecutive samples requested so far, launched together at the next call of any other entry
    // point (flush_calls); rmr_set_call_batching: -1 auto (on while the context owns its stream and its
    // accumulator), 0 off, 1 on
    std::vector<rmr::DeferredCall> deferred;
    uint64_t deferred_units = 0;
    int call_batching = -1;
    unsigned long long* d_queue = nullptr;
    unsigned long long* d_counters = nullptr;
    // timing
    std::vector<EventPair> pending, pool;
    rmr_stats stats{};
    int kernel_mode = 0;  // 0 persistent, 1 thread-per-path
    int shade_threshold = 16;   // explicit (env RMR_SHADE_T / rmr_set_tuning) or, with shade_auto, per kernel:
    bool shade_auto = true;     // per specialised kernel (ensure_jit: 20 / 8 / 16), 16 for the table kernels
    // idle lanes before a refill: -1 = half the shading threshold, at least 2 (round 2: T/2 = 8 at T = 16:
    // Cornell-5 -0.4%, RM3 -1.2%, default -2% against 2; Mandelbulb T = 8: 4 best); 0 = the shading
    // threshold; refills are cheap with the LDS chunk rays
    int refill_threshold = -1;
    // lane-slot kernels (rmr_trace.h RMR_LANE_SLOTS): -1 the kernel class's default, 0 off, 1 on where
    // the class can run it; park / batch thresholds (0: the class's, rmr_jit.hpp JitFacts). Their
    // refill threshold follows the park threshold as the others' follows the shading threshold
    int lane_slots = -1;
    int park_threshold = 0, slot_threshold = 0;
    // trailing passes per map-loop iteration (rmr_set_trail_steps, rmr_set_trail_tuning): rmr_trail_rule.h's
    // trail_word, -1 the kernel class's
    int trail_word = -1;
    // ... the word asks for the pass rule (a ratio or the park exit): the launch runs the code object that has
    // the rule compiled in (rmr_trace.h RMR_TRAIL_RULE; its own cache key), every other launch the one without
    bool trail_rule = false;
    int jit_slots = -1;         // the request `jit` was specialised with (slots_request)
    // nearest-primitive cache: 40 lanes per full map() batch, or once waiting lanes >= cache-served ones
    // (R = 8; csg256 with the candidate grid: 15.7 -> 14.8 ms per 4 spp against R = 2)
    int full_threshold = 40 | (8 << 8);
    int cull = RMR_CULL_ESCAPE | RMR_CULL_NPC | RMR_CULL_APPROX | RMR_CULL_EYE;   // rmr_set_culling
    int instrument = 0;   // RMR_INSTR_* (rmr_set_instrument): instrumented specialised kernels
    int grid_per_cu = 0;  // 0 = occupancy
    int grid_reserve = 0;  // persistent grid: workgroups left free of the occupancy grid (rmr_set_grid_reserve)
    bool diag_no_fold = false;   // RMR_DIAG_NO_FOLD (diagnostic library, timing only): no k_fold launch
    int small_chunk = 64;  // fewest units per work claim when a launch is too small to fill every wave (0: off)
    // hipRTC per-scene specialisation (rmr_jit.hpp): 0 off, 1 always, 2 auto (launches of
    // >= jit_min_units units; smaller renders use the ahead-of-time kernels). 2^16: C1's 256x256
    // 1-spp frame is 65536 units and runs 0.157 -> 0.106 ms per launch specialised (the compile,
    // ~1 s once per scene and process, is cached)
    int jit_mode = 2;
    uint64_t jit_min_units = (uint64_t)1 << 16;
    bool jit_ready = false;     // `jit` matches the loaded scene
    bool jit_failed = false;    // compile/load failed for the loaded scene (auto mode falls back)
    rmr::JitKernel jit;
    bool jit_rays_ready = false;   // `jit_rays`, the scene's ray-source kernel (rmr_jit_trace_rays), matches it
    rmr::JitKernel jit_rays;
    std::string jit_struct_src;  // structure-only source of the last specialised scene
    std::vector<rmr_prim> jit_base;   // primitive values the specialised kernel was baked with
    std::vector<char> jit_live;       // primitives that moved since: loaded, not literals
    std::vector<rmr::JitKernel> jit_loaded;  // modules loaded by this context (unloaded at destroy)
    // sample planes per launch (bytes): 48 GiB, at most a quarter of the device's memory (rmr_create).
    // 288 GB of HBM hold a whole C4 frame (3840x2160 x 256 spp: 34 GB) in one launch, so the frame
    // pays one persistent-kernel drain instead of one per 8 GiB
    size_t samp_budget = (size_t)48 << 30;
    std::string err;
    // capacity of each table buffer (keyed by the address of its device-pointer member): a reload of
    // the same scene layout (an animation frame) copies into the buffers it has, ordered on the
    // context's stream, instead of hipFree + hipMalloc, which wait for the whole device — including
    // another context's frame still rendering (FrameRenderer's two overlapping contexts)
    std::unordered_map<const void*, size_t> dev_caps;
};

namespace {

// the kernel's refill threshold from the context setting (rmr_ctx::refill_threshold) and the
// shading threshold in effect
int refill_for(int setting, int shade_t) {
    if (setting > 0) return setting;
    if (setting == 0) return shade_t;
    return std::max(2, shade_t / 2);
}

int fail(rmr_ctx* c, int code, const std::string& m) {
    if (c) c->err = m;
    return code;
}
#define HIPCHK(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(ctx, RMR_E_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

// Host -> device table upload, ordered on the context's stream: kernels of this context launched
// before it have read the old contents, those launched after read the new. A buffer is reallocated
// only when it must grow. The call returns once this context's stream has completed the copy (the
// source may be a temporary); another context's work on its own stream is not waited for.
template <class T>
int dev_upload(rmr_ctx* c, T** dst, const T* src, size_t n) {
    const size_t bytes = std::max<size_t>(1, n) * sizeof(T);
    size_t& cap = c->dev_caps[(const void*)dst];
    if (!*dst || cap < bytes) {
        if (*dst) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            (void)hipFree(*dst);
            *dst = nullptr;
        }
        HIPCHK(c, hipMalloc((void**)dst, bytes));
        cap = bytes;
    }
    if (n) {
        HIPCHK(c, hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return RMR_OK;
}

// All of a stage's device buffers or none: on a failure what was allocated is freed, every pointer of the
// list is null again and the error is RMR_E_NOMEM with `msg`.
struct Buf {
    void** p;
    size_t bytes;
    template <class T>
    Buf(T** q, size_t b = 0) : p((void**)q), bytes(b) {}
};
int alloc_all(rmr_ctx* c, std::initializer_list<Buf> list, const char* msg) {
    for (const Buf* a = list.begin(); a != list.end(); ++a) {
        if (hipMalloc(a->p, a->bytes) == hipSuccess) continue;
        (void)hipGetLastError();
        *a->p = nullptr;
        for (const Buf* k = list.begin(); k != a; ++k) { (void)hipFree(*k->p); *k->p = nullptr; }
        return fail(c, RMR_E_NOMEM, msg);
    }
    return RMR_OK;
}
void free_all(std::initializer_list<Buf> list) {
    for (const Buf& b : list) { if (*b.p) (void)hipFree(*b.p); *b.p = nullptr; }
}

// The end of every rmr_read_*: `bytes` from the device to the caller's buffer on the context's stream, done
// when the call returns.
int read_back(rmr_ctx* c, void* dst, const void* src, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

// Device scratch of one call of a host-image entry point (rmr_*_images): buffers, copies and launches on
// one stream until the first error, which it keeps and after which every request does nothing; done() waits
// for the stream whatever happened; the buffers go with the object.
struct Scratch {
    hipStream_t s;
    hipError_t e = hipSuccess;
    std::vector<void*> bufs;
    explicit Scratch(hipStream_t stream) : s(stream) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { for (void* b : bufs) (void)hipFree(b); }
    template <class T>
    T* get(size_t bytes) {
        void* b = nullptr;
        if (e == hipSuccess && (e = hipMalloc(&b, bytes)) == hipSuccess) bufs.push_back(b);
        return (T*)b;
    }
    void up(void* dst, const void* src, size_t bytes) { if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s); }
    void down(void* dst, const void* src, size_t bytes) { if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s); }
    template <class F>
    void run(F launch) { if (e == hipSuccess) e = launch(); }
    hipError_t done() {
        const hipError_t es = hipStreamSynchronize(s);
        return e == hipSuccess ? es : e;
    }
};

int alloc_accum(rmr_ctx* c) {
    if (!c->accum_external && c->d_accum) { (void)hipFree(c->d_accum); c->d_accum = nullptr; }
    c->accum_external = false;
    const size_t bytes = (size_t)c->W * c->H * sizeof(float4);
    HIPCHK(c, hipMalloc((void**)&c->d_accum, bytes));
    HIPCHK(c, hipMemsetAsync(c->d_accum, 0, bytes, c->stream));
    return RMR_OK;
}

void default_view(rmr_ctx* c) {
    // Program.cpp:102: Camera((0,4,-6), normalized(0,-3,6), W/H, PI/4), PI = 3.141592653f
    const double m = std::sqrt(0.0 + 9.0 + 36.0);
    const double eye[3] = {0.0, 4.0, -6.0};
    const double dir[3] = {0.0, -3.0 / m, 6.0 / m};
    const float pi = 3.141592653f;
    rmr_camera_view(eye, dir, (float)((double)c->W / (double)c->H), pi / 4.0f, c->view, c->view + 3, c->view + 6,
                    c->view + 9, c->view + 12);
    c->view_set = true;
}

int free_slots(rmr_ctx* c);

// Release the guide planes and the filter images (the caller has synced the context's stream).
void free_guides(rmr_ctx* c) {
    free_all({&c->d_guide[0], &c->d_guide[1], &c->d_guide[2], &c->d_dn[0], &c->d_dn[1],
              &c->d_var[0], &c->d_var[1], &c->d_var[2]});
    c->st.guides_freed();
}

// Release the temporal stage's planes (the caller has synced the context's stream).
void free_temporal(rmr_ctx* c) {
    free_all({&c->d_tcol[0], &c->d_tcol[1], &c->d_tn[0], &c->d_tn[1],
              &c->d_tguide[0], &c->d_tguide[1]});
    c->st.temporal_reset();
}

// Release the tone-mapping stage's buffers, the adaptation state with them (the caller has synced the
// context's stream).
void free_tonemap(rmr_ctx* c) {
    free_all({&c->d_tm, &c->d_tm_slab, &c->d_tm_state, &c->d_tm_lc});
    c->st.tonemap_begin();
    c->tm_used = 0;
}

// Release the bloom stage's planes (the caller has synced the context's stream).
void free_bloom(rmr_ctx* c) {
    free_all({&c->d_bl, &c->d_bl_pyr});
    c->st.bloom_reset();
}

// Release the sampled AOVs' planes (the caller has synced the context's stream).
void free_aov(rmr_ctx* c) {
    free_all({&c->d_aov, &c->d_aov_res});
    c->aov_rendered = c->aov_res_valid = false;
    c->aov_samples = 0;
}

// Release the mesh's buffers (the caller has synced the context's stream); there is no mesh afterwards.
void drop_mesh(rmr_ctx* c) {
    free_all({&c->d_mesh_v, &c->d_mesh_n, &c->d_mesh_id, &c->d_mesh_q, &c->d_mesh_rgba, &c->d_mesh_ao});
    c->mesh_valid = false;
    c->mesh_flags = c->mesh_baked = 0;
    c->mesh_nv = c->mesh_nq = 0;
}
// The same, the extraction's working memory and the bakes' per-point state.
void free_mesh(rmr_ctx* c) {
    drop_mesh(c);
    free_all({&c->d_mesh_dist, &c->d_mesh_flag, &c->d_mesh_cell, &c->d_mesh_scan, &c->d_bake_state});
    c->mesh_dist_cap = c->mesh_flag_cap = c->mesh_cell_cap = c->mesh_scan_cap = c->bake_state_cap = 0;
}

// Release the probe field and the probe bakes' state (the caller has synced the context's stream).
void free_probes(rmr_ctx* c) {
    free_all({&c->d_probe_field, &c->d_probe_state, &c->d_probe_vis, &c->d_probe_vis_state});
    c->probe_state_cap = 0;
    c->probe_vis_state_cap = 0;
    c->probe_valid = false;
    c->probe_vis_valid = false;
}

// Release the half image and the tile-error map (the caller has synced the context's stream).
void free_estimate(rmr_ctx* c) {
    free_all({&c->d_half, &c->d_tile_err});
    c->est_valid = false;
}

// Switch the estimate on: the half image and the tile-error map at the image's size if they are not
// there; valid, with the half image zeroed on the context's stream, when nothing has been rendered
// since the last rmr_reload.
int enable_estimate(rmr_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_half) {
        const size_t tiles = (size_t)((c->W + 7) / 8) * ((c->H + 7) / 8);
        const int r = alloc_all(c, {{&c->d_half, (size_t)c->W * c->H * sizeof(float4)},
                                    {&c->d_tile_err, tiles * sizeof(float)}},
                                "cannot allocate the half image (W x H x 16 bytes)");
        c->est_valid = false;
        if (r) {
            c->est_on = false;
            return r;
        }
    }
    c->est_on = true;
    if (c->est_valid) return RMR_OK;
    if (!c->rendered) {
        HIPCHK(c, hipMemsetAsync(c->d_half, 0, (size_t)c->W * c->H * sizeof(float4), c->stream));
        c->est_valid = true;
    }
    return RMR_OK;
}

// The experiments' switches of the diagnostic library that take effect at a scene load (RMR_ENV is
// nullptr in the release library, rmr_jit.hpp; rmr_create reads those of a context's settings).
rmr::AccelOptions read_switches(rmr_ctx* c) {
    rmr::AccelOptions o;
    if (const char* e = RMR_ENV("RMR_ESC_BOXES")) o.max_esc_boxes = (size_t)std::max(1, std::min(64, std::atoi(e)));
    if (const char* e = RMR_ENV("RMR_BVH_LEAF")) o.bvh_leaf = std::max(1, std::min(16, std::atoi(e)));
    if (const char* e = RMR_ENV("RMR_GRID")) o.grid = std::atoi(e) != 0;
    if (const char* e = RMR_ENV("RMR_GRID_CELLS")) o.grid_cells = std::max(1.0, std::atof(e));
    if (const char* e = RMR_ENV("RMR_GRID_PAD")) o.grid_pad = std::max(0.0, std::atof(e));
    c->npc_ksel = 0;
    if (const char* e = RMR_ENV("RMR_NPC_KSEL")) c->npc_ksel = std::atoi(e) == 1 ? 1 : 2;
    if (const char* e = RMR_ENV("RMR_FULL_T"))
        c->full_threshold = (c->full_threshold & ~0xff) | std::max(1, std::min(64, std::atoi(e)));
    if (const char* e = RMR_ENV("RMR_FULL_R"))
        c->full_threshold = (c->full_threshold & 0xff) | (std::max(0, std::min(255, std::atoi(e))) << 8);
    if (const char* e = RMR_ENV("RMR_SMALL_CHUNK")) c->small_chunk = std::max(0, std::atoi(e));
    c->diag_no_fold = false;
    if (const char* e = RMR_ENV("RMR_DIAG_NO_FOLD")) c->diag_no_fold = std::atoi(e) != 0;
    if (const char* e = RMR_ENV("RMR_SLOT_RESERVE")) c->slot_reserve = std::max(0, std::atoi(e));
    if (const char* e = RMR_ENV("RMR_LAUNCH_STREAMS")) {   // (the slots go at the next launch)
        (void)free_slots(c);
        c->launch_streams = std::max(0, std::min(4, std::atoi(e)));
    }
    return o;
}

// The launch parameters that only a scene load changes: the tables and what accel.hpp derived from them.
KParams scene_params(const rmr_ctx* c) {
    const CompiledScene& s = c->scene;
    const rmr::SceneAccel& a = c->accel;
    KParams P{};
    P.prims = c->d_prims; P.ops = c->d_ops; P.consts = c->d_consts; P.mats = c->d_mats;
    P.spec = c->d_spec; P.rm2 = c->d_rm2;
    P.dprims = c->d_dprims; P.dmats = c->d_dmats;
    P.bvh = c->d_bvh; P.n_nodes = (int)a.nodes.size(); P.bvh_margin = a.bvh_margin;
    if (a.grid_on) {
        P.grid = c->d_grid; P.grid_list = c->d_grid_list; P.grid_inv = a.grid.inv; P.grid_n_large = a.n_large;
        for (int k = 0; k < 3; k++) {
            P.grid_lo[k] = a.grid.lo[k];
            P.grid_dim[k] = a.grid.dim[k];
            P.grid_dimf[k] = (float)a.grid.dim[k];
        }
        for (int k = 0; k < 6; k++) P.grid_sbox[k] = a.grid.sbox[k];
    }
    P.n_prims = (int)s.prims.size();
    P.am_r2 = a.am_r2;
    P.npc_eps0 = a.npc_eps0;
    P.trail_eps_hi = INFINITY;   // (the launch's escape bound sets it, escape_params)
    P.cert_k = a.cert_k;
    P.full_threshold = c->full_threshold;
    P.n_mats = (int)(s.variant == RMR_VARIANT_RM3 ? s.spectral.size() : s.materials.size());
    P.v2_begin = s.v2_begin; P.v2_end = s.v2_end;
    P.spec_sky = s.spectral_sky;
    for (int i = 0; i < 3; i++) { P.sky[i] = s.sky[i]; P.rm2_light[i] = s.rm2.light_pos[i]; }
    P.rm2_light_power = s.rm2.light_power;
    P.rm2_node_id = s.rm2.node_mat_id;
    P.queue = c->d_queue;
    P.counters = c->d_counters;
    P.flops_static = (int32_t)s.flops_per_map();
    P.transc_static = (int32_t)s.transc_per_map();
    return P;
}

int upload_scene(rmr_ctx* c) {
    const CompiledScene& s = c->scene;
    const rmr::AccelOptions opt = read_switches(c);
    c->accel = rmr::build_scene_accel(s, opt);
    rmr::SceneAccel& a = c->accel;
    int r;
    if ((r = dev_upload(c, &c->d_prims, s.prims.data(), s.prims.size()))) return r;
    if ((r = dev_upload(c, &c->d_ops, s.ops.data(), s.ops.size()))) return r;
    if ((r = dev_upload(c, &c->d_consts, s.consts.data(), s.consts.size()))) return r;
    if ((r = dev_upload(c, &c->d_mats, s.materials.data(), s.materials.size()))) return r;
    if ((r = dev_upload(c, &c->d_spec, s.spectral.data(), s.spectral.size()))) return r;
    if ((r = dev_upload(c, &c->d_rm2, &s.rm2, 1))) return r;
    if ((r = dev_upload(c, &c->d_dmats, a.dmats.data(), a.dmats.size()))) return r;
    if ((r = dev_upload(c, &c->d_dprims, a.dprims.data(), a.dprims.size()))) return r;
    if (a.map_np == -2 && (r = dev_upload(c, &c->d_bvh, a.nodes.data(), a.nodes.size()))) return r;
    if (a.grid_on) {
        if ((r = dev_upload(c, &c->d_grid, a.grid_cells.data(), a.grid_cells.size()))) return r;
        if ((r = dev_upload(c, &c->d_grid_list, a.grid.list.data(), a.grid.list.size()))) return r;
    }
    // (the grid's arrays live on the device from here: 16 MB of cell records)
    a.grid_cells = {};
    a.grid.cells = {};
    a.grid.list = {};
    c->esc_infl_dev = -1.0;
    if (c->d_aov) {   // the sampled AOVs are the old scene's
        HIPCHK(c, hipStreamSynchronize(c->stream));
        free_aov(c);
    }
    c->scene_kp = scene_params(c);
    c->st.scene_loaded();   // (every scene load comes through here)
    c->scene_loaded = true;
    c->jit_ready = false;
    c->jit_rays_ready = false;
    c->jit_failed = false;
    c->stats.flops_per_map = s.flops_per_map();
    return RMR_OK;
}

// The lane-slot request of a launch with the context's parameters: the schedule covers paths with one
// channel pass and the constant sky (an event's record has no channel and a miss is shaded where it is
// found), and packs the bounce count above bit 9 of a word; other launches run the class's kernel without it.
int slots_request(const rmr_ctx* c) {
    if (c->params.separate_channels != 0 || c->params.use_env_tex != 0 || c->params.max_bounces >= (1 << 21)) return 0;
    return c->lane_slots;
}

// Compile (or fetch from the cache) and load the specialised trace kernel of the loaded scene.
// rays: the ray-source kernel (rmr_jit_trace_rays; never with lane slots), kept beside the other.
int ensure_jit(rmr_ctx* c, bool rays = false) {
    const int slots = rays ? 0 : slots_request(c);
    rmr::JitKernel& jk = rays ? c->jit_rays : c->jit;
    bool& ready = rays ? c->jit_rays_ready : c->jit_ready;
    if (ready && (rays || c->jit_slots == slots)) return RMR_OK;
    ready = false;
    if (!rays) c->jit_slots = slots;
    // animation: same structure as the last specialised scene, different numbers -> the primitives
    // that changed since the kernel's baked values become loads ("live"), the others stay literals:
    // one compile when the motion starts, then the same kernel every frame
    const std::string struct_src = rmr::jit_source(c->scene, c->accel.has_prog, false, c->cull);
    const auto& prims = c->scene.prims;
    if (struct_src != c->jit_struct_src || c->jit_base.size() != prims.size()) {   // new layout
        c->jit_base = prims;
        c->jit_live.assign(prims.size(), 0);
    } else {
        for (size_t j = 0; j < prims.size(); j++)
            if (std::memcmp(&prims[j], &c->jit_base[j], sizeof(rmr_prim)) != 0) c->jit_live[j] = 1;
    }
    c->jit_struct_src = struct_src;
    const rmr::CacheFacts cache = rmr::cache_kernel_facts(c->accel, c->accel.grid_on);
    rmr::JitFacts facts;
    const std::string src = rmr::jit_source(c->scene, c->accel.has_prog, true, c->cull, &c->jit_live,
                                            c->npc_ksel ? c->npc_ksel : cache.npc_k, cache.npc_spheres, &facts, slots, rays);
    std::vector<char> code;
    std::string key, log;
    std::vector<std::string> opts;
    if (c->instrument & RMR_INSTR_COUNT_FLOPS) opts.push_back("-DRMR_COUNT_FLOPS");
    const bool trail_rule = facts.trail && c->trail_rule;   // (classes without the steps: the one code object)
    if (trail_rule) opts.push_back("-DRMR_TRAIL_RULE=1");
    if (!rmr::jit_compile(src, code, key, log, opts)) {
        c->jit_failed = true;
        return fail(c, RMR_E_HIP, "hipRTC specialisation failed: " + log.substr(0, 2000));
    }
    for (const auto& k : c->jit_loaded) {
        if (k.key == key) {
            jk = k;
            ready = true;
            return RMR_OK;
        }
    }
    rmr::JitKernel k;
    k.key = key;
    k.trail_rule = trail_rule;
    // a code object that does not load (e.g. a stale disk-cache entry) marks the scene as failed, so
    // auto mode falls back to the ahead-of-time kernels instead of retrying every launch
    if (hipModuleLoadData(&k.module, code.data()) != hipSuccess) {
        c->jit_failed = true;
        return fail(c, RMR_E_HIP, "hipModuleLoadData of the specialised kernel failed (key " + key + ")");
    }
    const char* entry = rays ? "rmr_jit_trace_rays" : "rmr_jit_trace";
    if (hipModuleGetFunction(&k.fn, k.module, entry) != hipSuccess) {
        (void)hipModuleUnload(k.module);
        c->jit_failed = true;
        return fail(c, RMR_E_HIP, std::string(entry) + " missing from the specialised code object (key " + key + ")");
    }
    k.block = 256;
    k.chunk = facts.chunk();
    int b = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&b, k.fn, k.block, 0) != hipSuccess || b <= 0) b = 4;
    k.blocks_per_cu = b;
    // shading batch per kernel class (rmr_jit.hpp JitFacts::shade_t). Measured: the Mandelbulb 10 (8
    // until round 5's early bailout made the passes cheaper: 10 -0.6%, csg_nodes -0.5%); RM1 inline sphere/box maps 16 (20 until the map() loop lost ~12% of its instructions in
    // round 2; then 14-16 best on Cornell-5, 20 -> 16: -2.4%, multilight -4%, default +1.2%); node-program
    // materials 20 (round 4, 1080p 16 spp: default.scene 27.9 -> 26.9 ms, multilight 13.41 -> 13.24; 24:
    // -6% / +1.4%); the cache kernels 20 (csg256 1080p 8 spp: 16.83 -> 16.68 ms; 24: 16.81); the
    // certified sphere/box kernels at 7 waves 20 (Cornell-5 1080p 64 spp: 47.17 -> 46.63 ms; 18: 46.77,
    // 14: 47.92)
    k.shade_t = facts.shade_t();
    k.slots = facts.slots;
    k.park_t = facts.park_t();
    k.slot_t = facts.slot_t();
    k.slot_t_small = facts.slot_t_small();
    k.trail = facts.trail;
    k.trail_word = facts.trail_word();
    k.trail_word_small = facts.trail_word_small();
    c->jit_loaded.push_back(k);
    jk = k;
    ready = true;
    return RMR_OK;
}

// The ray buffer for `units` records. A failed allocation leaves the context without one (and as it was
// otherwise): RMR_E_NOMEM.
int ensure_rays(rmr_ctx* c, size_t units) {
    if (units <= c->rays_cap) return RMR_OK;
    if (c->d_rays) {
        HIPCHK(c, hipStreamSynchronize(c->stream));   // launches queued before may still read it
        (void)hipFree(c->d_rays);
        c->d_rays = nullptr;
        c->rays_cap = 0;
    }
    if (hipMalloc((void**)&c->d_rays, units * rmr::kRayRecordBytes) != hipSuccess) {
        (void)hipGetLastError();
        c->d_rays = nullptr;
        return fail(c, RMR_E_NOMEM, "cannot allocate the ray buffer (" + std::to_string(units * rmr::kRayRecordBytes) +
                                        " bytes; lower the plane budget, rmr_set_tuning)");
    }
    c->rays_cap = units;
    return RMR_OK;
}

int ensure_samp(rmr_ctx* c, size_t n) {
    if (n <= c->samp_cap) return RMR_OK;
    if (c->d_samp) { (void)hipFree(c->d_samp); c->d_samp = nullptr; c->samp_cap = 0; }
    HIPCHK(c, hipMalloc((void**)&c->d_samp, n * sizeof(float4)));
    c->samp_cap = n;
    return RMR_OK;
}


// Create every launch slot's stream, events and work queue (rmr_create, rmr_set_launch_streams: a
// stream created at a slot's first launch cost that launch ~6 ms, r06s_timeline_full_ls2.txt).
int make_slots(rmr_ctx* c) {
    c->slots.resize(c->launch_streams >= 2 ? (size_t)c->launch_streams : 0);
    c->next_slot = 0;
    for (auto& S : c->slots) {
        if (S.s) continue;
        HIPCHK(c, hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&S.freed, hipEventDisableTiming));
        HIPCHK(c, hipMalloc((void**)&S.queue, rmr::kQueueBytes));
        S.queue_dirty = true;
    }
    return RMR_OK;
}

// The next launch slot, for `units` sample-plane entries. Planes grow for every slot at once (the
// launches that follow are the same size: no allocation inside a run of them), each once the fold
// that last read it is done; the slot's stream then waits for that fold.
int slot_prepare(rmr_ctx* c, size_t units, rmr_ctx::Slot** out) {
    int r;
    if (c->slots.empty() || !c->slots[0].s) {
        if ((r = make_slots(c))) return r;
    }
    if (units > c->slots[c->next_slot].cap) {
        for (auto& T : c->slots) {
            if (units <= T.cap) continue;
            if (T.samp) {
                if (T.in_use) HIPCHK(c, hipEventSynchronize(T.freed));
                (void)hipFree(T.samp);
                T.samp = nullptr;
                T.cap = 0;
            }
            HIPCHK(c, hipMalloc((void**)&T.samp, units * sizeof(float4)));
            T.cap = units;
        }
    }
    rmr_ctx::Slot& S = c->slots[c->next_slot];
    c->next_slot = (c->next_slot + 1) % c->slots.size();
    if (S.in_use) HIPCHK(c, hipStreamWaitEvent(S.s, S.freed, 0));
    *out = &S;
    return RMR_OK;
}

// Release the launch slots (the context's stream synced first: every trace queued is done).
int free_slots(rmr_ctx* c) {
    if (c->slots.empty() && !c->trace_end) return RMR_OK;
    const hipError_t e = c->stream ? hipStreamSynchronize(c->stream) : hipSuccess;
    for (auto& S : c->slots) {
        if (S.s) {
            (void)hipStreamSynchronize(S.s);
            (void)hipStreamDestroy(S.s);
        }
        if (S.done) (void)hipEventDestroy(S.done);
        if (S.freed) (void)hipEventDestroy(S.freed);
        if (S.samp) (void)hipFree(S.samp);
        if (S.queue) (void)hipFree(S.queue);
    }
    c->slots.clear();
    c->next_slot = 0;
    if (c->trace_end) (void)hipEventDestroy(c->trace_end);
    c->trace_end = nullptr;
    c->last_samp = c->d_samp;
    if (e != hipSuccess) return fail(c, RMR_E_HIP, std::string("launch slots: ") + hipGetErrorString(e));
    return RMR_OK;
}

constexpr size_t kTileCacheEntries = 64;

uint64_t tiles_hash(const std::vector<TileXY>& t) {
    uint64_t h = 1469598103934665603ull ^ t.size();
    for (const TileXY& v : t) {
        h = (h ^ (uint32_t)v.x) * 1099511628211ull;
        h = (h ^ (uint32_t)v.y) * 1099511628211ull;
    }
    return h;
}

// The device copy of a tile list (cached by content, see rmr_ctx::tile_cache).
int tile_list(rmr_ctx* c, const std::vector<TileXY>& t, const TileXY** out) {
    const uint64_t h = tiles_hash(t);
    auto same = [](const TileXY& a, const TileXY& b) { return a.x == b.x && a.y == b.y; };
    for (auto& e : c->tile_cache)
        if (e.hash == h && e.host.size() == t.size() && std::equal(t.begin(), t.end(), e.host.begin(), same)) {
            e.used = ++c->tile_clock;
            *out = e.dev;
            return RMR_OK;
        }
    if (c->tile_cache.size() >= kTileCacheEntries) {
        auto lru = std::min_element(c->tile_cache.begin(), c->tile_cache.end(),
                                    [](const rmr_ctx::TileList& a, const rmr_ctx::TileList& b) { return a.used < b.used; });
        HIPCHK(c, hipStreamSynchronize(c->stream));   // launches queued before may still read it
        (void)hipFree(lru->dev);
        c->tile_cache.erase(lru);
    }
    rmr_ctx::TileList e{t, nullptr, h, ++c->tile_clock};
    HIPCHK(c, hipMalloc((void**)&e.dev, std::max<size_t>(1, t.size()) * sizeof(TileXY)));
    // a new buffer no queued launch reads: a plain synchronous copy, no wait for the stream
    const hipError_t er = hipMemcpy(e.dev, t.data(), t.size() * sizeof(TileXY), hipMemcpyHostToDevice);
    if (er != hipSuccess) {
        (void)hipFree(e.dev);
        return fail(c, RMR_E_HIP, std::string("tile list upload: ") + hipGetErrorString(er));
    }
    c->tile_cache.push_back(std::move(e));
    *out = c->tile_cache.back().dev;
    return RMR_OK;
}

// The launch's seeds on the device (launches of more than one sample; see rmr_ctx::h_times).
int stage_times(rmr_ctx* c, const float* times, uint32_t n, const float** out, hipStream_t st = nullptr) {
    if (!st) st = c->stream;
    if (n > c->times_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->d_times) (void)hipFree(c->d_times);
        if (c->h_times) (void)hipHostFree(c->h_times);
        c->d_times = nullptr;
        c->h_times = nullptr;
        c->times_cap = c->times_pos = 0;
        const size_t cap = std::max<size_t>(n, (size_t)1 << 16);
        HIPCHK(c, hipMalloc((void**)&c->d_times, cap * sizeof(float)));
        HIPCHK(c, hipHostMalloc((void**)&c->h_times, cap * sizeof(float), hipHostMallocDefault));
        c->times_cap = cap;
    }
    if (c->times_pos + n > c->times_cap) {   // wrap: every copy and launch that used the ring is done
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->times_pos = 0;
    }
    float* h = c->h_times + c->times_pos;
    float* d = c->d_times + c->times_pos;
    std::memcpy(h, times, n * sizeof(float));
    // (on a slot's stream, the copy is covered by the context stream's syncs above: the slot's trace
    // follows it there, and the trace's fold on the context stream waits for the trace)
    HIPCHK(c, hipMemcpyAsync(d, h, n * sizeof(float), hipMemcpyHostToDevice, st));
    c->times_pos += n;
    *out = d;
    return RMR_OK;
}

EventPair get_events(rmr_ctx* c) {
    if (!c->pool.empty()) {
        EventPair e = c->pool.back();
        c->pool.pop_back();
        return e;
    }
    EventPair e;
    (void)hipEventCreate(&e.a);
    (void)hipEventCreate(&e.b);
    (void)hipEventCreate(&e.c);
    return e;
}

int collect_timing(rmr_ctx* c) {
    for (auto& e : c->pending) {
        HIPCHK(c, hipEventSynchronize(e.c));
        float t1 = 0, t2 = 0;
        (void)hipEventElapsedTime(&t1, e.a, e.b);
        (void)hipEventElapsedTime(&t2, e.b, e.c);
        c->stats.trace_ms += t1;
        c->stats.fold_ms += t2;
        c->pool.push_back(e);
    }
    c->pending.clear();
    return RMR_OK;
}

// The launch's escape bound (rmr_trace.h ray_exit, accel.hpp escape_inflation): on for scenes whose every
// primitive takes part; the boxes go to the device again when the inflation changed.
// org_extent >= 0 (ray-source launches): the largest |coordinate| of any ray origin, in the eye's place.
int escape_params(rmr_ctx* c, KParams& P, double org_extent = -1.0) {
    const rmr::SceneAccel& a = c->accel;
    float org[3] = {c->view[0], c->view[1], c->view[2]};
    if (org_extent >= 0.0) {
        org[0] = std::nextafter((float)org_extent, INFINITY);
        org[1] = org[2] = 0.0f;
    }
    const double infl = rmr::escape_inflation(org, a.esc_extent, c->params.max_dist);
    // (infl < 2^44: |eye|, E, maxDist < 2^60, the range ray_exit's FMA slab form is exact in)
    P.esc_on = (c->cull & RMR_CULL_ESCAPE) && a.esc_all && infl < 0x1p44 && !a.esc_raw.empty() ? 1 : 0;
    if (P.esc_on && infl != c->esc_infl_dev) {
        const std::vector<float> bx = rmr::inflate_escape_boxes(a.esc_raw, infl);
        int rr;
        if ((rr = dev_upload(c, &c->d_esc, bx.data(), bx.size()))) return rr;
        c->esc_infl_dev = infl;
    }
    P.esc_boxes = c->d_esc;
    P.n_esc = (int)(a.esc_raw.size() / 6);
    // trailing steps (rmr_trail_rule.h): eps at every point a march bounded by these boxes can evaluate; without
    // the bound there is none, the rule refuses every lane, and the launch takes no trailing step (render_tiles)
    P.trail_eps_hi = P.esc_on ? rmr::trail_eps_bound(org, a.esc_extent, infl, a.err_extent) : INFINITY;
    return RMR_OK;
}

// What a launch needs of the context's state (rmr_render gives the same errors at the call it defers).
int launch_precheck(rmr_ctx* c) {
    if (!c->scene_loaded) return fail(c, RMR_E_STATE, "no scene loaded (call rmr_load_scene_json / rmr_load_builtin_scene)");
    if (c->params.use_env_tex && !c->d_env) return fail(c, RMR_E_STATE, "useEnvTex != 0 but no env map (rmr_set_env_map)");
    return RMR_OK;
}

// KParams::am_dmax (rmr_trace.h am_far): the largest float strictly below maxDist - (2^-20 (maxDist + 2 R)
// + 2^-39), twice the approximate minimum's error bound at maxDist, computed in double and rounded
// down; -inf (every lane takes the exact fold) where that is not positive or maxDist is not finite.
float am_direct_bound(float max_dist, float am_r2) {
    if (!std::isfinite(max_dist) || !std::isfinite(am_r2)) return -INFINITY;
    const double b = (double)max_dist - (((double)max_dist + (double)am_r2) * 0x1p-20 + 0x1p-39);
    const float f = std::nextafter((float)b, -INFINITY);
    return f > 0.0f ? f : -INFINITY;
}

// The view, the render parameters, the env map and the buffers on top of the scene's parameters.
int view_params(rmr_ctx* c, KParams& P, double org_extent = -1.0) {
    P = c->scene_kp;
    int r;
    if ((r = escape_params(c, P, org_extent))) return r;
    {
        // primary rays' first march step from the eye (rmr_trace.h eye_map): the march point
        // fma(dir, 0, eye) is the eye itself for every finite direction unless an eye coordinate is
        // -0 (then it is +-0 by the direction's sign), so that case keeps the per-lane step
        bool neg0 = false;
        for (int k = 0; k < 3; k++)
            neg0 = neg0 || (c->view[k] == 0.0f && std::signbit(c->view[k])) || !std::isfinite(c->view[k]);
        P.eye_step = (c->cull & RMR_CULL_EYE) && !neg0 ? 1 : 0;
    }
    P.env = c->d_env; P.env_w = c->env_w; P.env_h = c->env_h;
    P.use_env = (c->params.use_env_tex != 0 && c->d_env) ? 1 : 0;
    P.max_dist = c->params.max_dist; P.step_mult = c->params.step_multiply;
    P.am_dmax = am_direct_bound(P.max_dist, P.am_r2);
    P.max_steps = c->params.max_steps; P.max_bounces = c->params.max_bounces;
    P.separate_channels = c->params.separate_channels;
    for (int i = 0; i < 3; i++) {
        P.eye[i] = c->view[i]; P.r00[i] = c->view[3 + i]; P.r01[i] = c->view[6 + i];
        P.r10[i] = c->view[9 + i]; P.r11[i] = c->view[12 + i];
    }
    P.W = c->W; P.H = c->H;
    for (int i = 0; i < 3; i++) {
        P.dr01[i] = P.r01[i] - P.r00[i];   // float subtraction: the bits fmix's y - x gives
        P.dr11[i] = P.r11[i] - P.r10[i];
    }
    P.Wf = (float)c->W; P.Hf = (float)c->H;
    P.env_wf[0] = (float)c->env_w; P.env_wf[1] = (float)c->env_h;
    P.env_wf[2] = (float)(c->env_w - 1); P.env_wf[3] = (float)(c->env_h - 1);
    P.eye_xy = P.eye[0] + P.eye[1];
    P.accum = c->d_accum;
    P.shade_threshold = c->shade_threshold;
    P.refill_threshold = refill_for(c->refill_threshold, c->shade_threshold);
    return RMR_OK;
}

// One trace launch and its fold, queued: the trace on the slot's stream (or the context's), the fold on the
// context's stream after it.
// rays: the launch's ray buffer (the ray-source kernels), null for the view's own rays. fold false
// (rmr_trace_rays): the planes are the result, the accumulator is not touched (the next launch then
// zeroes the queue with a memset).
int submit_launch(rmr_ctx* c, const KParams& P, rmr_ctx::Slot* S, bool use_jit, int grid, const float4* rays = nullptr,
                  bool fold = true) {
    const hipStream_t ts = S ? S->s : c->stream;   // the trace's stream
    bool& qdirty = S ? S->queue_dirty : c->queue_dirty;
    if (qdirty) HIPCHK(c, hipMemsetAsync(P.queue, 0, rmr::kQueueBytes, ts));
    qdirty = true;   // until the fold that zeroes it is queued
    EventPair ev = get_events(c);
    HIPCHK(c, hipEventRecord(ev.a, ts));
    hipError_t le;
    if (use_jit) {
        const rmr::JitKernel& jk = rays ? c->jit_rays : c->jit;
        void* args[] = {const_cast<KParams*>(&P), (void*)&rays};
        le = hipModuleLaunchKernel(jk.fn, (unsigned)grid, 1, 1, (unsigned)jk.block, 1, 1, 0, ts, args, nullptr);
        if (le == hipSuccess) c->stats.jit_launches++;
    } else if (rays) {
        le = rmr::launch_trace_rays(P, rays, c->scene.variant, c->accel.map_np, c->accel.has_prog, c->kernel_mode == 0, grid, ts);
    } else {
        le = rmr::launch_trace(P, c->scene.variant, c->accel.map_np, c->accel.has_prog, c->kernel_mode == 0, grid, ts);
    }
    if (le == hipSuccess) le = hipEventRecord(ev.b, ts);
    if (le == hipSuccess && c->launch_streams >= 2) {
        if (!c->trace_end) le = hipEventCreateWithFlags(&c->trace_end, hipEventDisableTiming);
        if (le == hipSuccess) le = hipEventRecord(c->trace_end, ts);
    }
    if (S) {
        // the context's stream waits for the trace before its fold (and before anything after it)
        if (le == hipSuccess) le = hipEventRecord(S->done, ts);
        if (le == hipSuccess) le = hipStreamWaitEvent(c->stream, S->done, 0);
        if (le != hipSuccess) (void)hipStreamSynchronize(ts);   // nothing of this slot left running
    }
    if (le != hipSuccess) return fail(c, RMR_E_HIP, std::string("trace launch: ") + hipGetErrorString(le));
    // (RMR_DIAG_NO_FOLD: what the fold costs the frame, a timing experiment with a wrong accumulator;
    // the next launch then zeroes the queue with a memset)
    if (!c->diag_no_fold && fold) {
        HIPCHK(c, c->est_on ? rmr::launch_fold_half(P, c->d_half, c->stream) : rmr::launch_fold(P, c->stream));
        qdirty = false;
    }
    if (S) {
        HIPCHK(c, hipEventRecord(S->freed, c->stream));
        S->in_use = true;
    }
    HIPCHK(c, hipEventRecord(ev.c, c->stream));
    c->pending.push_back(ev);
    c->stats.trace_launches++;
    c->stats.samples += P.n_units;  // upper bound
    return RMR_OK;
}

// A caller's ray list as the core's work (rmr_trace_rays): n rays, their radiance to out (RGBA32F).
// d_rays set (rmr_trace_rays_device): the list and the result live on the device, the records are
// packed and the planes unpacked by kernels (rmr_query.hip), `extent` bounds the origins, and nothing
// is copied or synchronised.
// bake set (rmr_bake_points_device): the list is a bake's tile-samples instead (rmr_bake.hip: tile t of 64
// points, sample k, at index t nspp + k; the plan's "samples" are these), n counts them, k_bake_rays writes
// the records and k_bake_fold reads the planes: d_out is the points' [n][4] result.
// probe set (rmr_bake_probes_device): the units are probes' tile-samples, k_probe_rays and k_probe_fold take the
// two kernels' places (rmr_probe.hip), list states n and nspp, and d_out is the probes' [n][28] result.
struct BakeJob { rmr::BakeList list; const float* h_times; float4* state; rmr::ProbeList* probe = nullptr; };
struct RayList { const rmr_ray* rays; size_t n; float* out; const rmr_ray* d_rays; float* d_out; float extent;
                 BakeJob* bake = nullptr; };

// words of rmr_ctx::d_query: rays the device forms rejected (rmr_query_rejects); the device forms'
// first rejected index (not read); the same two of a host form's call
enum { kQueryRejects = 0, kQueryFirstBad = 1, kQueryHostRejects = 2, kQueryHostFirstBad = 3, kQueryWords = 4 };

int ensure_query(rmr_ctx* c) {
    if (c->d_query) return RMR_OK;
    HIPCHK(c, hipMalloc((void**)&c->d_query, kQueryWords * sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->d_query, 0, kQueryWords * sizeof(unsigned long long), c->stream));
    return RMR_OK;
}

// The device records (rmr_trace.h ray_record) of list units [u0, u0 + h.size() / 3): the caller's rays,
// then "no ray" records up to the end of the last tile.
void pack_rays(const RayList& rl, size_t u0, std::vector<float4>& h) {
    const size_t units = h.size() / 3;
    for (size_t i = 0; i < units; i++) {
        float4* q = &h[3 * i];
        if (u0 + i < rl.n) {
            const rmr_ray& y = rl.rays[u0 + i];
            q[0] = make_float4(y.o[0], y.o[1], y.o[2], y.time);
            q[1] = make_float4(y.d[0], y.d[1], y.d[2], y.rc);
            q[2] = make_float4((float)y.gx + y.time, (float)y.gy + y.time, 0.0f, 0.0f);   // gid + time, one rounding
        } else {
            q[0] = q[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            q[2] = make_float4(0.0f, 0.0f, NAN, 0.0f);
        }
    }
}

// Core: nspp samples over an 8x8 tile list, clipped to [x0,x1)x[y0,y1).
// With a camera model other than the view's own, each launch is the generator (k_camera_rays), the
// ray-source trace kernel on its records, and the unchanged fold. With a ray list (rl; tiles, the rect,
// the seeds and the sample indices are then not used) the list's 64-ray tiles take the samples' place
// in the plan (one "tile" of 64 units, ceil(n / 64) "samples": the same unit order), each launch is the
// upload of its records, the ray-source kernel and the readback of its planes, and nothing is folded.
// A device list (rl->d_rays) has k_pack_rays in the upload's place and k_unpack_rgba in the readback's, and
// is not synchronised. A bake (rl->bake) is a device list whose units are a bake's tile-samples: k_bake_rays
// writes the records from the points and k_bake_fold folds the planes onto the points' state (rmr_bake.hip).
// Ray-source launches run on the context's stream: no launch slots.
int render_tiles(rmr_ctx* c, const std::vector<TileXY>& tiles, int x0, int y0, int x1, int y1,
                 const float* times, uint32_t first_sample, uint32_t nspp, const RayList* rl = nullptr) {
    int r;
    if ((r = launch_precheck(c))) return r;
    if (rl) nspp = rl->bake ? (uint32_t)rl->n : (uint32_t)((rl->n + 63) / 64);
    if ((!rl && tiles.empty()) || nspp == 0) return RMR_OK;
    const bool rays = rl || c->camera.model != RMR_CAMERA_VIEW;
    if (!c->view_set) default_view(c);
    // the model's frame (not needed where every ray starts at the eye along the view's own direction)
    rmr::CamParams cam{};
    double org_extent = -1.0;
    if (rays && !rl) {
        const rmr_camera_model& m = c->camera;
        cam.model = m.model;
        cam.p[0] = m.aperture; cam.p[1] = m.focus; cam.p[2] = m.width; cam.p[3] = m.height;
        float f[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (!(m.model == RMR_CAMERA_THIN_LENS && m.aperture == 0.0f) && !rmr::camera_frame(c->view, f))
            return fail(c, RMR_E_INVALID, "the view has no camera frame (rmr_camera_frame): the camera model needs one");
        for (int k = 0; k < 3; k++) { cam.U[k] = f[k]; cam.V[k] = f[3 + k]; cam.F[k] = f[6 + k]; }
        org_extent = rmr::camera_origin_extent(m, c->view);
    }
    if (rl && (rl->d_rays || rl->bake)) {
        org_extent = (double)rl->extent;
        if ((r = ensure_query(c))) return r;
    } else if (rl) {
        org_extent = 0.0;
        for (size_t i = 0; i < rl->n; i++)
            for (int k = 0; k < 3; k++) org_extent = std::max(org_extent, std::fabs((double)rl->rays[i].o[k]));
    }
    const TileXY* d_tiles = nullptr;
    if (!rl) {
        c->st.accum_changed();   // the denoised image is of the old one
        c->rendered = true;
        if ((r = tile_list(c, tiles, &d_tiles))) return r;
    }
    const size_t plane = rl ? 64 : tiles.size() * 64;
    const rmr::SamplePlan sp = rmr::plan_samples(plane, nspp, c->samp_budget, rays ? 0 : c->launch_streams,
                                                 rays ? sizeof(float4) + rmr::kRayRecordBytes : sizeof(float4));
    const size_t chunk = sp.per_launch;
    if (rl && rl->bake && (r = stage_times(c, rl->bake->h_times, rl->bake->list.nspp, &rl->bake->list.times))) return r;
    if (rl && rl->bake && rl->bake->probe) rl->bake->probe->times = rl->bake->list.times;
    if (sp.slotted && c->slots.size() != (size_t)c->launch_streams) {
        if ((r = free_slots(c)) || (r = make_slots(c))) return r;
    }
    KParams P;
    if ((r = view_params(c, P, org_extent))) return r;
    P.x0 = x0; P.y0 = y0; P.x1 = x1; P.y1 = y1;
    P.tiles = d_tiles;
    P.n_tiles = rl ? 1 : (int)tiles.size();

    // hipRTC specialisation for large launches (always when jit_mode == 1)
    bool use_jit = false;
    if (c->kernel_mode == 0 && c->jit_mode != 0 && !(c->jit_mode == 2 && c->jit_failed)) {
        if (c->jit_mode == 1 || (uint64_t)chunk * plane >= c->jit_min_units) {
            const int jr = ensure_jit(c, rays);
            if (jr == RMR_OK) use_jit = true;
            else if (c->jit_mode == 1) return jr;
        }
    }
    const rmr::JitKernel& jk = rays ? c->jit_rays : c->jit;   // (when use_jit)
    int bpc = c->grid_per_cu;
    if (bpc <= 0) {
        if (use_jit) bpc = jk.blocks_per_cu;
        else if ((rays ? rmr::trace_rays_occupancy(c->scene.variant, c->accel.map_np, c->accel.has_prog, &bpc)
                       : rmr::trace_occupancy(c->scene.variant, c->accel.map_np, c->accel.has_prog, &bpc)) != 0 || bpc <= 0)
            bpc = 4;
    }
    const int full_grid = c->n_cu * bpc;
    for (uint32_t k0 = 0; k0 < nspp; k0 += (uint32_t)chunk) {
        const uint32_t n = (uint32_t)std::min<size_t>(chunk, nspp - k0);
        // a slot only while the previous trace is still running (something to overlap); otherwise the
        // context's stream, with no stream hop (one launch per frame, then a sync: r06t_slot_ab.log)
        rmr_ctx::Slot* S = nullptr;
        if (sp.slotted && c->trace_end && hipEventQuery(c->trace_end) == hipErrorNotReady) {
            if ((r = slot_prepare(c, plane * n, &S))) return r;
            P.samp = S->samp;
            P.queue = S->queue;
        } else {
            if ((r = ensure_samp(c, plane * n))) return r;
            P.samp = c->d_samp;
            P.queue = c->d_queue;
        }
        if (rays && (r = ensure_rays(c, plane * n))) return r;
        const float* d_times = nullptr;
        if (!rl && n > 1 && (r = stage_times(c, times + k0, n, &d_times, S ? S->s : c->stream))) return r;
        c->last_samp = P.samp;
        P.nspp = n;
        P.first_sample = first_sample + k0;
        P.times = d_times;
        P.time1 = rl ? 0.0f : times[k0];   // the seed when this launch has one sample (unit_pixel)
        P.n_units = (uint64_t)n * plane;
        std::vector<float4> h_rays;   // (a list's records; the launch is synchronised below)
        if (rl && rl->bake && rl->bake->probe) {
            HIPCHK(c, rmr::launch_probe_rays(P, c->accel.map_np, *rl->bake->probe, k0, n, c->d_rays, c->d_query + kQueryRejects,
                                             c->stream));
        } else if (rl && rl->bake) {
            HIPCHK(c, rmr::launch_bake_rays(rl->bake->list, k0, n, c->d_rays, c->d_query + kQueryRejects, c->stream));
        } else if (rl && rl->d_rays) {
            HIPCHK(c, rmr::launch_pack_rays(rl->d_rays, rl->n, (uint64_t)k0 * 64, (uint32_t)P.n_units, rl->extent, c->d_rays,
                                            c->d_query + kQueryRejects, c->d_query + kQueryFirstBad, c->stream));
        } else if (rl) {
            h_rays.resize(3 * (size_t)P.n_units);
            pack_rays(*rl, (size_t)k0 * 64, h_rays);
            HIPCHK(c, hipMemcpyAsync(c->d_rays, h_rays.data(), h_rays.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        } else if (rays) {
            HIPCHK(c, rmr::launch_camera_rays(P, cam, c->d_rays, c->stream));
        }
        // slotted launches leave workgroups free for the previous launch's fold, which waits behind
        // the next trace's persistent workgroups otherwise (and the slot's reuse behind that fold)
        const int reserve = (S && c->grid_reserve == 0) ? c->slot_reserve : c->grid_reserve;
        const rmr::GridPlan gp = rmr::plan_grid(P.n_units, full_grid, reserve, (use_jit ? jk.block : 256) / 64,
                                                use_jit ? jk.chunk : 128, c->small_chunk, P.max_bounces,
                                                c->grid_per_cu, c->kernel_mode);
        P.chunk_units = gp.chunk_units;
        // tuned shading batch size of the kernel that runs (measured: C2 +2% at 20; the Mandelbulb
        // and the cached BVH map -1..2%)
        if (c->shade_auto) {
            P.shade_threshold = use_jit ? jk.shade_t : 16;
            P.refill_threshold = refill_for(c->refill_threshold, P.shade_threshold);
        }
        if (use_jit && jk.slots) {
            const int park = c->park_threshold > 0 ? c->park_threshold : jk.park_t;
            // the class's batch threshold by the launch's size (JitFacts::slot_t_small): claims per wave
            const bool small = P.n_units < (uint64_t)gp.grid * (uint64_t)(jk.block / 64) * (uint64_t)jk.chunk *
                                               (uint64_t)rmr::JitFacts::kSlotSmallClaims;
            const int batch = c->slot_threshold > 0 ? c->slot_threshold : (small ? jk.slot_t_small : jk.slot_t);
            // trailing passes (rmr_trace.h RMR_TRAIL_STEPS; rmr_trail_rule.h trail_word), bits 16-24: only where
            // the source has them, and only for a march that advances (rmr_trail_rule.h: the rule's t >= t0)
            int trail = !jk.trail ? 0 : (c->trail_word >= 0 ? c->trail_word : (small ? jk.trail_word_small : jk.trail_word));
            if (!(P.step_mult > 0.0f) || !std::isfinite(P.step_mult)) trail = 0;
            if (!std::isfinite(P.trail_eps_hi)) trail = 0;   // no escape bound: no bound of eps either
            if (!jk.trail_rule) trail = rmr::trail_word(rmr::trail_word_k(trail), 0, false);   // (this code object reads no rule)
            P.shade_threshold = park | (batch << 8) | (trail << rmr::kTrailWordShift);
            P.refill_threshold = refill_for(c->refill_threshold, park);
        }
        if ((r = submit_launch(c, P, S, use_jit, gp.grid, rays ? c->d_rays : nullptr, !rl))) return r;
        if (rl && rl->bake && rl->bake->probe) {
            HIPCHK(c, rmr::launch_probe_fold(c->probe_fold_mapping, P.samp, c->d_rays, rl->bake->state, rl->bake->list.n,
                                             rl->bake->list.nspp, k0, n, rl->d_out, c->stream));
        } else if (rl && rl->bake) {
            HIPCHK(c, rmr::launch_bake_fold(false, P.samp, c->d_rays, rl->bake->state, rl->bake->list.n, rl->bake->list.nspp,
                                            k0, n, rl->d_out, c->stream));
        } else if (rl && rl->d_rays) {
            const size_t u0 = (size_t)k0 * 64, cnt = std::min<size_t>((size_t)P.n_units, rl->n - u0);
            HIPCHK(c, rmr::launch_unpack_rgba(P.samp, c->d_rays, rl->d_out + 4 * u0, (uint32_t)cnt, c->stream));
        } else if (rl) {
            const size_t u0 = (size_t)k0 * 64, cnt = std::min<size_t>((size_t)P.n_units, rl->n - u0);
            HIPCHK(c, hipMemcpyAsync(rl->out + 4 * u0, P.samp, cnt * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    return RMR_OK;
}

using rmr::rect_tiles;

// The device image of a source StageState::readable found valid, in buffer i.
const float4* source_image(const rmr_ctx* c, int source, int i) {
    switch (source) {
    case RMR_OUTPUT_DENOISED: return c->d_dn[i];
    case RMR_OUTPUT_TEMPORAL: return c->d_tcol[i];
    case RMR_OUTPUT_TONEMAPPED: return c->d_tm;
    case RMR_OUTPUT_BLOOM: return c->d_bl;
    default: return c->d_accum;
    }
}
// The words the refusals of a source that is not valid are made of: the image's name and the call that makes it.
const char* const kSourceName[5] = {"", "denoised", "temporal", "tonemapped", "bloom"};
const char* const kSourceCall[5] = {"", "rmr_denoise", "rmr_temporal_accumulate", "rmr_tonemap", "rmr_bloom"};
int no_valid(rmr_ctx* c, int source) {
    return fail(c, RMR_E_STATE, std::string("no valid ") + kSourceName[source] + " image (call " + kSourceCall[source] + ")");
}

// The image rmr_save_bmp / rmr_display* read (rmr_set_output_source).
int output_image(rmr_ctx* c, const char* who, const float4** out) {
    const int src = c->output_source, i = c->st.readable(src);
    if (i < 0)
        return fail(c, RMR_E_STATE, std::string(who) + ": output source is the " + kSourceName[src] + " image, but none is valid (call " +
                                        kSourceCall[src] + ")");
    *out = source_image(c, src, i);
    return RMR_OK;
}

bool batching_on(const rmr_ctx* c) {
    return c->call_batching > 0 || (c->call_batching < 0 && c->own_stream && !c->accum_external);
}

// deferred units beyond which rmr_render launches what it holds (2^28 units: 4 GiB of sample planes)
constexpr uint64_t kDeferredUnitsMax = (uint64_t)1 << 28;
constexpr size_t kDeferredRectsMax = 4096;

// Launch the deferred one-sample calls, grouped by accel.hpp group_deferred.
int flush_calls(rmr_ctx* c) {
    if (c->deferred.empty()) return RMR_OK;
    std::vector<rmr::DeferredCall> d;
    d.swap(c->deferred);
    c->deferred_units = 0;
    for (const rmr::CallLaunch& l : rmr::group_deferred(d)) {
        const int r = render_tiles(c, rect_tiles(l.x0, l.y0, l.x1, l.y1), l.x0, l.y0, l.x1, l.y1, l.times, l.s0, l.n);
        if (r) return r;
    }
    return RMR_OK;
}

// The *_device_ptr getters' flush: false when the deferred calls could not be launched (the getter returns null).
bool flushed(rmr_ctx* c) { return c->deferred.empty() || flush_calls(c) == RMR_OK; }

#if RMR_DIAG
// Diagnostic library only (rmr_diag_tonemap_time, rmr_diag_bloom_time):
// *ms = the GPU's time per round of n back-to-back rounds on the context's stream, between two events. So that
// the time is the GPU's and not the host's enqueue rate, the stream is first kept busy (k_lum_hist over the
// accumulator, then 32 k_meter launches, about 0.9 ms; fold and run_meter: their arguments) while the host
// queues the first event, the rounds and the second event behind it; n <= 64 keeps the host ahead. The tone
// stage's buffers are there (ensure_tonemap). Synchronises.
template <class Round>
int timed_rounds(rmr_ctx* c, bool fold, bool run_meter, int n, float* ms, Round round) {
    const size_t px = (size_t)c->W * c->H;
    const int blocks = rmr::lum_hist_blocks(px);
    rmr_tonemap_params tq;
    rmr_default_tonemap_params(&tq);
    const rmr::ToneMeter M = rmr::tonemap_meter(tq);
    hipEvent_t ev[2] = {nullptr, nullptr};
    HIPCHK(c, hipEventCreate(&ev[0]));
    hipError_t e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) e = rmr::launch_lum_hist(c->d_accum, px, c->d_tm_slab, blocks, fold, c->stream);
    for (int i = 0; i < 32 && e == hipSuccess; i++)
        e = rmr::launch_meter(c->d_tm_slab, blocks, c->d_tm_state, c->d_tm_lc, M, run_meter, c->stream);
    if (e == hipSuccess) e = hipEventRecord(ev[0], c->stream);
    for (int i = 0; i < n && e == hipSuccess; i++) e = round();
    if (e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    float t = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ev[0], ev[1]);
    (void)hipEventDestroy(ev[0]);
    if (ev[1]) (void)hipEventDestroy(ev[1]);
    HIPCHK(c, e);
    *ms = t / (float)n;
    return RMR_OK;
}
#endif

}  // namespace

// every entry point but rmr_render (and the pure getters) first launches the deferred calls, so that
// whatever it reads, changes or orders sees them done in call order
#define RMR_FLUSH(c)                                                   \
    do {                                                               \
        if (!(c)->deferred.empty()) {                                  \
            const int rf_ = flush_calls(c);                            \
            if (rf_) return rf_;                                       \
        }                                                              \
    } while (0)

extern "C" {

const char* rmr_build_info(void) {
    return "rmr gfx950 (CDNA4): variants RM1/RM2/RM3; wave64 persistent path-state kernel; "
           "scalar-cached scene tables; -ffp-contract=off deterministic math";
}

void rmr_default_params(rmr_params* p) {
    if (!p) return;
    p->max_dist = 1000.0f;  // Graphics.cpp:326
    p->max_steps = 512;     // Graphics.cpp:327
    p->max_bounces = 16;    // Graphics.cpp:328
    p->step_multiply = 0.5f;  // Graphics.cpp:329
    p->separate_channels = 0; // Graphics.cpp:340
    p->use_env_tex = 0;       // Graphics.cpp:338
}

int rmr_create(rmr_ctx** out, int device) {
    if (!out) return RMR_E_INVALID;
    *out = nullptr;
    rmr_ctx* c = new (std::nothrow) rmr_ctx();
    if (!c) return RMR_E_NOMEM;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        delete c;
        return RMR_E_HIP;
    }
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return RMR_E_HIP; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        c->n_cu = prop.multiProcessorCount;
        if (prop.totalGlobalMem > 0) c->samp_budget = std::min(c->samp_budget, (size_t)prop.totalGlobalMem / 4);
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return RMR_E_HIP; }
    c->own_stream = true;
    rmr_default_params(&c->params);
    if (hipMalloc((void**)&c->d_queue, rmr::kQueueBytes) != hipSuccess ||
        hipMalloc((void**)&c->d_counters, rmr::kCounterSlots * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(c->d_counters, 0, rmr::kCounterSlots * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(c->d_queue, 0, rmr::kQueueBytes) != hipSuccess) {   // then each fold zeroes it
        rmr_destroy(c);
        return RMR_E_HIP;
    }
    if (const char* e = RMR_ENV("RMR_SHADE_T")) {
        c->shade_threshold = std::max(1, std::atoi(e));
        c->shade_auto = false;
    }
    if (const char* e = RMR_ENV("RMR_REFILL_T")) c->refill_threshold = std::max(0, std::atoi(e));
    if (const char* e = RMR_ENV("RMR_LANE_SLOTS")) c->lane_slots = std::atoi(e) != 0;
    if (const char* e = RMR_ENV("RMR_PARK_T")) c->park_threshold = std::max(0, std::min(64, std::atoi(e)));
    if (const char* e = RMR_ENV("RMR_SLOT_T")) c->slot_threshold = std::max(0, std::min(64, std::atoi(e)));
    if (const char* e = RMR_ENV("RMR_ESC")) if (std::atoi(e) == 0) c->cull &= ~RMR_CULL_ESCAPE;
    if (const char* e = RMR_ENV("RMR_NPC")) if (std::atoi(e) == 0) c->cull &= ~RMR_CULL_NPC;
    if (const char* e = RMR_ENV("RMR_JIT_APPROX")) if (std::atoi(e) == 0) c->cull &= ~RMR_CULL_APPROX;
    if (const char* e = RMR_ENV("RMR_EYE")) if (std::atoi(e) == 0) c->cull &= ~RMR_CULL_EYE;
    if (const char* e = RMR_ENV("RMR_GRID_PER_CU")) c->grid_per_cu = std::max(0, std::atoi(e));
    if (const char* e = RMR_ENV("RMR_GRID_RESERVE")) c->grid_reserve = std::max(0, std::atoi(e));
    if (const char* e = RMR_ENV("RMR_JIT")) c->jit_mode = std::max(0, std::min(2, std::atoi(e)));
    // launch slots: 2 within HIP's default 4 hardware queues per process (the context's stream, two
    // slots, the caller's default stream); 4 where the process has 8 or more (GPU_MAX_HW_QUEUES, the
    // variable HIP reads): the per-call loop then runs at 511 against 356 Msamples/s (r06ze_api_ls.log)
    if (const char* e = std::getenv("GPU_MAX_HW_QUEUES"))
        if (std::atoi(e) >= 8) c->launch_streams = 4;
    if (alloc_accum(c) != RMR_OK || make_slots(c) != RMR_OK) { rmr_destroy(c); return RMR_E_HIP; }
    *out = c;
    return RMR_OK;
}

void rmr_destroy(rmr_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)free_slots(c);
    for (auto& e : c->pending) c->pool.push_back(e);
    for (auto& e : c->pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); (void)hipEventDestroy(e.c); }
    void* bufs[] = {c->d_prims, c->d_ops, c->d_consts, c->d_mats, c->d_spec, c->d_rm2, c->d_dprims, c->d_dmats, c->d_bvh, c->d_esc, c->d_env, c->d_samp, c->d_rays, c->d_query, c->d_qin, c->d_qout,
                    c->d_times, c->d_queue, c->d_counters, c->d_srgb_thr, c->d_screen, c->d_grid, c->d_grid_list};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    for (auto& e : c->tile_cache) (void)hipFree(e.dev);
    if (c->h_times) (void)hipHostFree(c->h_times);
    free_guides(c);
    free_temporal(c);
    free_tonemap(c);
    free_bloom(c);
    free_aov(c);
    free_mesh(c);
    free_probes(c);
    free_estimate(c);
    if (c->d_accum && !c->accum_external) (void)hipFree(c->d_accum);
    for (auto& k : c->jit_loaded)
        if (k.module) (void)hipModuleUnload(k.module);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* rmr_last_error(const rmr_ctx* c) { return c ? c->err.c_str() : "null context"; }

int rmr_set_stream(rmr_ctx* c, void* s) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int r = free_slots(c);   // (every queued trace done)
    if (r) return r;
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    if (s) {
        c->stream = (hipStream_t)s;
        c->own_stream = false;
    } else {
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    // the slots' streams again, created after the context's stream (HIP hands out its hardware queues
    // in creation order: r06v_set_stream_slots.log)
    return make_slots(c);
}

int rmr_set_image_size(rmr_ctx* c, int w, int h) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (w <= 0 || h <= 0 || w > 32768 || h > 32768) return fail(c, RMR_E_INVALID, "bad image size");
    c->pend_W = w;
    c->pend_H = h;
    if (c->d_aov) {   // (the sampled AOVs are of the old size's image)
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        free_aov(c);
    }
    // (the auto-exposure's adaptation state is of the old size's images)
    if (c->d_tm_state) HIPCHK(c, hipSetDevice(c->device));
    if (c->d_tm_state) HIPCHK(c, hipMemsetAsync(&c->d_tm_state->valid, 0, sizeof(uint32_t), c->stream));
    return RMR_OK;
}

int rmr_get_image_size(const rmr_ctx* c, int* w, int* h) {
    if (!c || !w || !h) return RMR_E_INVALID;
    *w = c->W;
    *h = c->H;
    return RMR_OK;
}

int rmr_set_params(rmr_ctx* c, const rmr_params* p) {
    if (!c || !p) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (p->max_steps < 0 || p->max_bounces < 0 || !(p->max_dist > 0.0f)) return fail(c, RMR_E_INVALID, "bad params");
    c->params = *p;
    c->st.inputs_changed();
    return RMR_OK;
}

int rmr_get_params(const rmr_ctx* c, rmr_params* p) {
    if (!c || !p) return RMR_E_INVALID;
    *p = c->params;
    return RMR_OK;
}

int rmr_set_view(rmr_ctx* c, const float eye[3], const float r00[3], const float r01[3], const float r10[3],
                 const float r11[3]) {
    if (!c || !eye || !r00 || !r01 || !r10 || !r11) return RMR_E_INVALID;
    RMR_FLUSH(c);
    for (int i = 0; i < 3; i++) {
        c->view[i] = eye[i]; c->view[3 + i] = r00[i]; c->view[6 + i] = r01[i];
        c->view[9 + i] = r10[i]; c->view[12 + i] = r11[i];
    }
    c->view_set = true;
    c->st.inputs_changed();
    return RMR_OK;
}

int rmr_load_scene_json(rmr_ctx* c, int variant, const char* json, size_t len) {
    if (!c || !json) return RMR_E_INVALID;
    RMR_FLUSH(c);
    try {
        CompiledScene s = rmr::compile_scene(std::string(json, len), variant);
        if (const char* bad = rmr::validate_scene(s)) return fail(c, RMR_E_SCENE, bad);
        c->scene = std::move(s);
    } catch (const rmr::SceneError& e) {
        return fail(c, RMR_E_SCENE, e.what());
    } catch (const std::exception& e) {
        return fail(c, RMR_E_SCENE, e.what());
    }
    HIPCHK(c, hipSetDevice(c->device));
    return upload_scene(c);
}

int rmr_load_scene_tables(rmr_ctx* c, const rmr_scene* s) {
    if (!c || !s) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (s->variant < RMR_VARIANT_RM1 || s->variant > RMR_VARIANT_RM3) return fail(c, RMR_E_INVALID, "bad variant");
    if (s->n_prims < 0 || s->n_prims > RMR_MAX_PRIMS || s->n_ops < 0 || s->n_ops > RMR_MAX_OPS ||
        s->n_consts < 0 || s->n_consts > RMR_MAX_CONSTS || s->n_materials < 0 || s->n_materials > RMR_MAX_MATERIALS)
        return fail(c, RMR_E_INVALID, "table sizes out of range");
    CompiledScene cs;
    cs.from_tables(*s);
    if (const char* bad = rmr::validate_scene(cs)) return fail(c, RMR_E_SCENE, bad);
    c->scene = std::move(cs);
    HIPCHK(c, hipSetDevice(c->device));
    return upload_scene(c);
}

int rmr_load_builtin_scene(rmr_ctx* c, int variant) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (variant == RMR_VARIANT_RM2) return fail(c, RMR_E_SCENE, "RayMarch2.glsl needs a v2 scene for mat_func_1; use rmr_load_scene_json");
    try {
        c->scene = rmr::builtin_scene(variant);
    } catch (const std::exception& e) {
        return fail(c, RMR_E_SCENE, e.what());
    }
    HIPCHK(c, hipSetDevice(c->device));
    return upload_scene(c);
}

int rmr_reload(rmr_ctx* c) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->accum_external && (c->pend_W != c->W || c->pend_H != c->H))
        return fail(c, RMR_E_STATE, "bound accumulator cannot be resized");
    const bool resize = (c->pend_W != c->W || c->pend_H != c->H);
    free_guides(c);   // (the stream is idle)
    free_temporal(c);
    free_tonemap(c);
    free_bloom(c);
    free_aov(c);
    free_mesh(c);
    free_probes(c);
    c->W = c->pend_W;
    c->H = c->pend_H;
    if (resize) {
        if (c->view_set) { /* caller's view is kept (reference: camera.calculateRays after Reload) */ }
        int r = alloc_accum(c);
        if (r) return r;
    } else {
        HIPCHK(c, hipMemsetAsync(c->d_accum, 0, (size_t)c->W * c->H * sizeof(float4), c->stream));
    }
    c->rendered = false;
    c->sample_counts.clear();
    c->est_valid = false;
    if (resize) free_estimate(c);   // (the stream is idle)
    if (c->est_on) return enable_estimate(c);   // the setting survives: B for the new size, zeroed
    return RMR_OK;
}

int rmr_render(rmr_ctx* c, float time, float min_x, float min_y, float max_x, float max_y, uint32_t current_sample) {
    if (!c) return RMR_E_INVALID;
    // pix >= bounds.xy && pix < bounds.zw for integer pix (RM1:572) <=> pix in [ceil(min), ceil(max))
    int x0 = (int)std::ceil(min_x), y0 = (int)std::ceil(min_y), x1 = (int)std::ceil(max_x), y1 = (int)std::ceil(max_y);
    if (!rmr::clamp_rect(c->W, c->H, x0, y0, x1, y1)) return RMR_OK;
    if (!batching_on(c) || c->camera.model != RMR_CAMERA_VIEW) {   // (ray-source launches are not call-batched)
        RMR_FLUSH(c);
        return render_tiles(c, rect_tiles(x0, y0, x1, y1), x0, y0, x1, y1, &time, current_sample, 1);
    }
    // deferred (rmr_set_call_batching): the errors the launch would give now come at the call
    if (const int r = launch_precheck(c)) return r;
    c->st.accum_changed();
    c->rendered = true;
    rmr::DeferredCall* same = nullptr;
    bool overlap = false;
    for (auto& e : c->deferred) {
        if (e.x0 == x0 && e.y0 == y0 && e.x1 == x1 && e.y1 == y1) same = &e;
        else if (x0 < e.x1 && e.x0 < x1 && y0 < e.y1 && e.y0 < y1) overlap = true;
    }
    if (overlap || (same && current_sample != same->s0 + (uint32_t)same->times.size()) ||
        (!same && c->deferred.size() >= kDeferredRectsMax)) {
        RMR_FLUSH(c);
        same = nullptr;
    }
    if (same) same->times.push_back(time);
    else c->deferred.push_back(rmr::DeferredCall{x0, y0, x1, y1, current_sample, std::vector<float>(1, time)});
    c->deferred_units += (uint64_t)((x1 - x0 + 7) / 8) * ((y1 - y0 + 7) / 8) * 64;
    if (c->deferred_units >= kDeferredUnitsMax) RMR_FLUSH(c);
    return RMR_OK;
}

int rmr_set_call_batching(rmr_ctx* c, int mode) {
    if (!c || mode < -1 || mode > 1) return RMR_E_INVALID;
    RMR_FLUSH(c);
    c->call_batching = mode;
    return RMR_OK;
}

int rmr_set_launch_streams(rmr_ctx* c, int n) {
    if (!c || n < 0 || n > 4) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (n == c->launch_streams) return RMR_OK;
    int r = free_slots(c);   // (syncs the context's stream: every queued trace is done)
    c->launch_streams = n;
    return r ? r : make_slots(c);
}

int rmr_get_launch_streams(const rmr_ctx* c) { return c ? c->launch_streams : -1; }

int rmr_render_spp(rmr_ctx* c, const float* times, int x0, int y0, int x1, int y1, uint32_t first_sample, uint32_t nspp) {
    if (!c || (!times && nspp)) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!rmr::clamp_rect(c->W, c->H, x0, y0, x1, y1)) return RMR_OK;
    return render_tiles(c, rect_tiles(x0, y0, x1, y1), x0, y0, x1, y1, times, first_sample, nspp);
}

int rmr_render_tiles(rmr_ctx* c, const float* times, const int32_t* tiles_xy, int n_tiles, int tile_size,
                     uint32_t first_sample, uint32_t nspp) {
    if (!c || (!times && nspp) || (!tiles_xy && n_tiles) || tile_size <= 0 || (tile_size % 8) != 0)
        return fail(c, RMR_E_INVALID, "tile_size must be a positive multiple of 8");
    RMR_FLUSH(c);
    // every (tx, ty) at most once: k_fold gives each pixel of a launch one thread, and a repeated
    // tile would have two threads read-modify-write the same accumulator pixel
    std::vector<std::pair<int, int>> seen;
    seen.reserve((size_t)n_tiles);
    for (int i = 0; i < n_tiles; i++) {
        if (tiles_xy[2 * i] < 0 || tiles_xy[2 * i + 1] < 0) return fail(c, RMR_E_INVALID, "negative tile index");
        seen.emplace_back(tiles_xy[2 * i], tiles_xy[2 * i + 1]);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
        return fail(c, RMR_E_INVALID, "duplicate tile in rmr_render_tiles");
    const std::vector<TileXY> t = rmr::expand_tiles(tiles_xy, n_tiles, tile_size, c->W, c->H);
    if (t.empty()) return RMR_OK;
    return render_tiles(c, t, 0, 0, c->W, c->H, times, first_sample, nspp);
}

int rmr_read_accum(rmr_ctx* c, float* rgba, size_t bytes) {
    if (!c || !rgba) return RMR_E_INVALID;
    RMR_FLUSH(c);
    const size_t need = (size_t)c->W * c->H * sizeof(float4);
    if (bytes < need) return fail(c, RMR_E_INVALID, "buffer too small");
    return read_back(c, rgba, c->d_accum, need);
}

int rmr_write_accum(rmr_ctx* c, const float* rgba, size_t bytes) {
    if (!c || !rgba) return RMR_E_INVALID;
    RMR_FLUSH(c);
    const size_t need = (size_t)c->W * c->H * sizeof(float4);
    if (bytes < need) return fail(c, RMR_E_INVALID, "buffer too small");
    c->st.accum_changed();
    c->rendered = true;    // (the accumulator has contents the half image knows nothing of)
    c->est_valid = false;
    HIPCHK(c, hipMemcpyAsync(c->d_accum, rgba, need, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

void* rmr_accum_device_ptr(rmr_ctx* c) {
    if (!c) return nullptr;
    if (!flushed(c)) return nullptr;   // the pointer's contents include them
    return (void*)c->d_accum;
}

int rmr_bind_accum(rmr_ctx* c, void* ptr, size_t bytes) {
    if (!c || !ptr) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (bytes < (size_t)c->W * c->H * sizeof(float4)) return fail(c, RMR_E_INVALID, "bound accumulator too small");
    if (c->d_accum && !c->accum_external) {  // the context's own buffer: free it once idle
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(c->d_accum);
    }
    // (an external buffer is only swapped: launches already queued keep the pointer they captured)
    c->d_accum = (float4*)ptr;
    c->accum_external = true;
    c->st.accum_changed();
    c->est_valid = false;
    return RMR_OK;
}

int rmr_save_bmp(rmr_ctx* c, const char* path) {
    if (!c || !path) return RMR_E_INVALID;
    RMR_FLUSH(c);
    std::vector<float> host((size_t)c->W * c->H * 4);
    const float4* src = nullptr;
    int r = output_image(c, "rmr_save_bmp", &src);
    if (r) return r;
    if ((r = read_back(c, host.data(), src, host.size() * sizeof(float)))) return r;
    r = rmr_encode_bmp(host.data(), c->W, c->H, path);
    if (r) return fail(c, r, std::string("cannot write ") + path);
    return RMR_OK;
}

int rmr_save_accum(rmr_ctx* c, const char* path, uint32_t samples_done) {
    if (!c || !path) return RMR_E_INVALID;
    RMR_FLUSH(c);
    std::vector<float> host((size_t)c->W * c->H * 4);
    int r = rmr_read_accum(c, host.data(), host.size() * sizeof(float));
    if (r) return r;
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(c, RMR_E_IO, std::string("cannot open ") + path);
    const char magic[8] = {'R', 'M', 'R', 'A', 'C', 'C', '1', 0};
    const uint32_t hdr[3] = {(uint32_t)c->W, (uint32_t)c->H, samples_done};
    bool ok = std::fwrite(magic, 1, 8, f) == 8 && std::fwrite(hdr, 4, 3, f) == 3 &&
              std::fwrite(host.data(), sizeof(float), host.size(), f) == host.size();
    ok = (std::fclose(f) == 0) && ok;
    return ok ? RMR_OK : fail(c, RMR_E_IO, "write failed");
}

int rmr_load_accum(rmr_ctx* c, const char* path, uint32_t* samples_done) {
    if (!c || !path) return RMR_E_INVALID;
    RMR_FLUSH(c);
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(c, RMR_E_IO, std::string("cannot open ") + path);
    char magic[8];
    uint32_t hdr[3];
    if (std::fread(magic, 1, 8, f) != 8 || std::memcmp(magic, "RMRACC1", 8) != 0 || std::fread(hdr, 4, 3, f) != 3) {
        std::fclose(f);
        return fail(c, RMR_E_IO, "not an rmr accumulator file");
    }
    if ((int)hdr[0] != c->W || (int)hdr[1] != c->H) {
        std::fclose(f);
        return fail(c, RMR_E_STATE, "accumulator size does not match the image size");
    }
    std::vector<float> host((size_t)c->W * c->H * 4);
    const bool ok = std::fread(host.data(), sizeof(float), host.size(), f) == host.size();
    std::fclose(f);
    if (!ok) return fail(c, RMR_E_IO, "truncated accumulator file");
    if (samples_done) *samples_done = hdr[2];
    return rmr_write_accum(c, host.data(), host.size() * sizeof(float));
}

int rmr_sync(rmr_ctx* c) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return collect_timing(c);
}

int rmr_get_stats(rmr_ctx* c, rmr_stats* out) {
    if (!c || !out) return RMR_E_INVALID;
    RMR_FLUSH(c);
    int r = rmr_sync(c);
    if (r) return r;
    unsigned long long cnt[16];
    HIPCHK(c, hipMemcpy(cnt, c->d_counters, sizeof cnt, hipMemcpyDeviceToHost));
    c->stats.map_evals = cnt[0];
    c->stats.map_iters = cnt[1];
    c->stats.shade_batches = cnt[2];
    *out = c->stats;
    return RMR_OK;
}

int rmr_get_section_cycles(rmr_ctx* c, uint64_t out[4]) {
    if (!c || !out) return RMR_E_INVALID;
    RMR_FLUSH(c);
    int r = rmr_sync(c);
    if (r) return r;
    unsigned long long cnt[8];
    HIPCHK(c, hipMemcpy(cnt, c->d_counters, sizeof cnt, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; i++) out[i] = cnt[4 + i];
    return RMR_OK;
}

int rmr_get_counters(rmr_ctx* c, uint64_t out[16]) {
    if (!c || !out) return RMR_E_INVALID;
    RMR_FLUSH(c);
    int r = rmr_sync(c);
    if (r) return r;
    unsigned long long cnt[16];
    HIPCHK(c, hipMemcpy(cnt, c->d_counters, sizeof cnt, hipMemcpyDeviceToHost));
    for (int i = 0; i < 16; i++) out[i] = cnt[i];
    return RMR_OK;
}

int rmr_get_counters_n(rmr_ctx* c, uint64_t* out, int n) {
    if (!c || !out || n < 0 || n > rmr::kCounterSlots) return RMR_E_INVALID;
    RMR_FLUSH(c);
    int r = rmr_sync(c);
    if (r) return r;
    unsigned long long cnt[rmr::kCounterSlots];
    HIPCHK(c, hipMemcpy(cnt, c->d_counters, (size_t)n * sizeof cnt[0], hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) out[i] = cnt[i];
    return RMR_OK;
}

int rmr_reset_stats(rmr_ctx* c) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    int r = rmr_sync(c);
    if (r) return r;
    const double fpm = c->stats.flops_per_map;
    c->stats = rmr_stats{};
    c->stats.flops_per_map = fpm;
    HIPCHK(c, hipMemset(c->d_counters, 0, rmr::kCounterSlots * sizeof(unsigned long long)));
    return RMR_OK;
}

int rmr_set_kernel(rmr_ctx* c, int kernel) {
    if (!c || kernel < 0 || kernel > 1) return RMR_E_INVALID;
    RMR_FLUSH(c);
    c->kernel_mode = kernel;
    return RMR_OK;
}

// The candidate grid a context builds for a BVH scene, on the host (contract: rmr.h; construction:
// grid.cpp build_candidate_grid).
int rmr_candidate_grid(const float* prims, int n, int n_large, double E, double target, double pad, int32_t idims[5],
                       float geom[12], uint32_t* cells, size_t cells_cap, uint16_t* list, size_t list_cap) {
    if (!prims || n <= 0 || n_large < 0 || n_large > n || !idims || !geom) return RMR_E_INVALID;
    std::vector<rmr::DPrim> dp((size_t)n);
    for (int i = 0; i < n; i++) {
        const float* r = prims + 8 * (size_t)i;
        rmr::DPrim q{};
        for (int k = 0; k < 3; k++) { q.c[k] = r[k]; q.r[k] = r[3 + k]; }
        q.type = (int32_t)r[6] | (i << 8);
        q.mat_id = r[7];
        dp[(size_t)i] = q;
    }
    rmr::CandidateGrid g;
    const bool built = rmr::build_candidate_grid(dp, n_large, E, target > 0.0 ? target : 1048576.0,
                                                 pad > 0.0 ? pad : 0.5, g);
    for (int k = 0; k < 5; k++) idims[k] = 0;
    for (int k = 0; k < 12; k++) geom[k] = 0.0f;
    idims[4] = built ? 1 : 0;
    if (!built) return RMR_OK;
    for (int k = 0; k < 3; k++) { idims[k] = g.dim[k]; geom[k] = g.lo[k]; }
    idims[3] = (int32_t)g.list.size();
    geom[3] = g.inv;
    for (int k = 0; k < 6; k++) geom[4 + k] = g.sbox[k];
    geom[10] = (float)g.eps;
    geom[11] = (float)g.margin;
    if (!cells || !list || cells_cap < g.cells.size() || list_cap < g.list.size()) return RMR_E_INVALID;
    std::memcpy(cells, g.cells.data(), g.cells.size() * sizeof(uint32_t));
    std::memcpy(list, g.list.data(), g.list.size() * sizeof(uint16_t));
    return RMR_OK;
}

// (rmr_srgb_thresholds, the sRGB decision points of the display's encode, is host-only code: bake.cpp)
namespace {
int display_common(rmr_ctx* c, float cx, float cy, float zoom, float min_x, float min_y, float max_x, float max_y,
                   int sw, int sh, uint32_t* dev) {
    if (!c->d_srgb_thr) {
        float t[256];
        rmr_srgb_thresholds(t);
        int r = dev_upload(c, &c->d_srgb_thr, t, 256);
        if (r) return r;
    }
    const float4* src = nullptr;
    if (const int r = output_image(c, "rmr_display", &src)) return r;
    HIPCHK(c, rmr::launch_display(src, c->W, c->H, cx, cy, zoom, min_x, min_y, max_x, max_y, sw, sh, dev,
                                  c->d_srgb_thr, c->stream));
    return RMR_OK;
}
}  // namespace

int rmr_display(rmr_ctx* c, float centre_x, float centre_y, float zoom, float min_x, float min_y, float max_x,
                float max_y, int screen_w, int screen_h, uint8_t* rgba8, size_t nbytes) {
    if (!c || !rgba8 || screen_w <= 0 || screen_h <= 0 || screen_w > 32768 || screen_h > 32768)
        return fail(c, RMR_E_INVALID, "rmr_display: bad screen image");
    if (nbytes < (size_t)screen_w * screen_h * 4)
        return fail(c, RMR_E_INVALID, "rmr_display: screen buffer smaller than screen_w * screen_h * 4 bytes");
    RMR_FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)screen_w * screen_h;
    if (n > c->screen_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->d_screen) (void)hipFree(c->d_screen);
        c->d_screen = nullptr;
        c->screen_cap = 0;
        HIPCHK(c, hipMalloc((void**)&c->d_screen, n * sizeof(uint32_t)));
        c->screen_cap = n;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_screen, rgba8, n * 4, hipMemcpyHostToDevice, c->stream));
    int r = display_common(c, centre_x, centre_y, zoom, min_x, min_y, max_x, max_y, screen_w, screen_h, c->d_screen);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(rgba8, c->d_screen, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

int rmr_display_device(rmr_ctx* c, float centre_x, float centre_y, float zoom, float min_x, float min_y, float max_x,
                       float max_y, int screen_w, int screen_h, void* rgba8_dev, size_t nbytes) {
    if (!c || !rgba8_dev || screen_w <= 0 || screen_h <= 0 || screen_w > 32768 || screen_h > 32768)
        return fail(c, RMR_E_INVALID, "rmr_display_device: bad screen image");
    if (nbytes < (size_t)screen_w * screen_h * 4)
        return fail(c, RMR_E_INVALID, "rmr_display_device: screen buffer smaller than screen_w * screen_h * 4 bytes");
    RMR_FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    return display_common(c, centre_x, centre_y, zoom, min_x, min_y, max_x, max_y, screen_w, screen_h,
                          (uint32_t*)rgba8_dev);
}

int rmr_set_env_map(rmr_ctx* c, const uint8_t* rgba8, int w, int h) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!rgba8) {
        if (c->d_env) (void)hipFree(c->d_env);
        c->d_env = nullptr;
        c->env_w = c->env_h = 0;
        return RMR_OK;
    }
    if (w <= 0 || h <= 0 || (size_t)w * h > ((size_t)1 << 26)) return fail(c, RMR_E_INVALID, "bad env map size");
    std::vector<float4> t((size_t)w * h);
    for (size_t i = 0; i < t.size(); i++)  // GL unorm8 -> float: c / 255
        t[i] = make_float4((float)rgba8[4 * i] / 255.0f, (float)rgba8[4 * i + 1] / 255.0f,
                           (float)rgba8[4 * i + 2] / 255.0f, (float)rgba8[4 * i + 3] / 255.0f);
    int r;
    if ((r = dev_upload(c, &c->d_env, t.data(), t.size()))) return r;
    c->env_w = w;
    c->env_h = h;
    return RMR_OK;
}

int rmr_set_jit(rmr_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 2) return RMR_E_INVALID;
    RMR_FLUSH(c);
    c->jit_mode = mode;
    c->jit_failed = false;
    return RMR_OK;
}

int rmr_set_culling(rmr_ctx* c, int flags) {
    if (!c || (flags & ~(RMR_CULL_ESCAPE | RMR_CULL_NPC | RMR_CULL_APPROX | RMR_CULL_EYE))) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (flags != c->cull) c->jit_ready = c->jit_rays_ready = false;   // the specialised kernels depend on it
    c->cull = flags;
    return RMR_OK;
}

static int jit_compile_scene(int variant, const char* json, size_t len, char* log, size_t loglen, bool rays) {
    std::string lg;
    try {
        CompiledScene s = (json && len) ? rmr::compile_scene(std::string(json, len), variant) : rmr::builtin_scene(variant);
        // the kernel class as a context picks it (ensure_jit), with the candidate grid of a BVH scene
        // taken as built (as it is unless it would exceed 2^31 cells) rather than built here
        rmr::AccelOptions opt;
        opt.grid = false;
        const rmr::SceneAccel a = rmr::build_scene_accel(s, opt);
        const rmr::CacheFacts cache = rmr::cache_kernel_facts(a, true);
        std::vector<char> code;
        std::string key;
        const bool ok = rmr::jit_compile(
            rmr::jit_source(s, a.has_prog, true, RMR_CULL_ESCAPE | RMR_CULL_NPC | RMR_CULL_APPROX | RMR_CULL_EYE, nullptr,
                            cache.npc_k, cache.npc_spheres, nullptr, -1, rays),
            code, key, lg);
        if (log && loglen) std::snprintf(log, loglen, "%s", ok ? key.c_str() : lg.c_str());
        return ok ? RMR_OK : RMR_E_HIP;
    } catch (const std::exception& e) {
        if (log && loglen) std::snprintf(log, loglen, "%s", e.what());
        return RMR_E_SCENE;
    }
}
int rmr_jit_compile_scene(int variant, const char* json, size_t len, char* log, size_t loglen) {
    return jit_compile_scene(variant, json, len, log, loglen, false);
}
int rmr_jit_compile_scene_rays(int variant, const char* json, size_t len, char* log, size_t loglen) {
    return jit_compile_scene(variant, json, len, log, loglen, true);
}

int rmr_set_instrument(rmr_ctx* c, int flags) {
    if (!c || (flags & ~RMR_INSTR_COUNT_FLOPS)) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (flags != c->instrument) {
        c->instrument = flags;
        c->jit_ready = c->jit_rays_ready = false;   // another code object (its own cache key)
        c->jit_failed = false;
    }
    return RMR_OK;
}

int rmr_set_tuning(rmr_ctx* c, int shade_threshold, int grid_per_cu, long long samp_budget_bytes) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (shade_threshold > 0) {
        if (shade_threshold & 0xff) {
            c->shade_threshold = std::max(1, std::min(64, shade_threshold & 0xff));
            c->shade_auto = false;
        }
        const int tr = (shade_threshold >> 8) & 0xff;
        if ((shade_threshold & 0xffff) || !(shade_threshold & (1 << 23)))
            c->refill_threshold = tr ? std::min(64, tr) : -1;   // unset: half the shading threshold
        // lane-slot kernels, when bit 23 is set: bits 16..22 the park threshold (127: the schedule off),
        // 24..30 the batch threshold (0: the kernel class's)
        if (shade_threshold & (1 << 23)) {
            const int park = (shade_threshold >> 16) & 0x7f;
            c->lane_slots = park == 127 ? 0 : -1;
            c->park_threshold = park == 127 ? 0 : std::min(64, park);
            c->slot_threshold = std::min(64, (shade_threshold >> 24) & 0x7f);
        }
    }
    if (grid_per_cu >= 0) c->grid_per_cu = grid_per_cu;
    if (samp_budget_bytes > 0) c->samp_budget = (size_t)samp_budget_bytes;
    return RMR_OK;
}

// the trailing passes' code object: with the pass rule compiled in or without (ensure_jit)
static void set_trail_rule(rmr_ctx* c, bool rule) {
    if (rule == c->trail_rule) return;
    c->trail_rule = rule;
    c->jit_ready = false;   // another code object (its own cache key); the ray-source kernels have no passes
    c->jit_failed = false;
}

int rmr_set_trail_steps(rmr_ctx* c, int steps) {
    if (!c || steps < -1 || steps > rmr::kTrailMaxSteps) return RMR_E_INVALID;
    RMR_FLUSH(c);
    c->trail_word = steps < 0 ? -1 : rmr::trail_word(steps, 0, false);
    set_trail_rule(c, false);
    return RMR_OK;
}

int rmr_set_trail_tuning(rmr_ctx* c, int k_max, int ratio_eighths, int park_exit) {
    if (!c) return RMR_E_INVALID;
    if (k_max < 0 || k_max > rmr::kTrailMaxSteps)
        return fail(c, RMR_E_INVALID, "rmr_set_trail_tuning: k_max " + std::to_string(k_max) + " outside 0.." +
                                          std::to_string(rmr::kTrailMaxSteps));
    if (ratio_eighths < 0 || ratio_eighths > rmr::kTrailMaxRatio)
        return fail(c, RMR_E_INVALID, "rmr_set_trail_tuning: ratio_eighths " + std::to_string(ratio_eighths) + " outside 0.." +
                                          std::to_string(rmr::kTrailMaxRatio));
    if (park_exit != 0 && park_exit != 1)
        return fail(c, RMR_E_INVALID, "rmr_set_trail_tuning: park_exit " + std::to_string(park_exit) + " is neither 0 nor 1");
    RMR_FLUSH(c);
    c->trail_word = rmr::trail_word(k_max, ratio_eighths, park_exit != 0);
    set_trail_rule(c, ratio_eighths != 0 || park_exit != 0);
    return RMR_OK;
}

int rmr_set_grid_reserve(rmr_ctx* c, int blocks) {
    if (!c || blocks < 0) return RMR_E_INVALID;
    RMR_FLUSH(c);
    c->grid_reserve = blocks;
    return RMR_OK;
}

// Per-sample radiance planes for parity tests: out[k][y-y0][x-x0][4] for the rect.
int rmr_trace_samples(rmr_ctx* c, const float* times, int x0, int y0, int x1, int y1, uint32_t nspp, float* out) {
    if (!c || !times || !out) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!rmr::clamp_rect(c->W, c->H, x0, y0, x1, y1) || nspp == 0) return RMR_OK;
    std::vector<TileXY> tiles = rect_tiles(x0, y0, x1, y1);
    const size_t saved_budget = c->samp_budget;
    const size_t plane = tiles.size() * 64;
    // one chunk (under a camera model a unit also holds its ray record)
    const size_t unit_bytes = sizeof(float4) + (c->camera.model != RMR_CAMERA_VIEW ? rmr::kRayRecordBytes : 0);
    c->samp_budget = std::max(saved_budget, plane * nspp * unit_bytes);
    // render into a scratch accumulator region: trace writes samp planes; fold into accum is harmless
    std::vector<float> keep((size_t)c->W * c->H * 4);
    int r = rmr_read_accum(c, keep.data(), keep.size() * sizeof(float));
    if (!r) r = render_tiles(c, tiles, x0, y0, x1, y1, times, 0, nspp);
    c->samp_budget = saved_budget;
    if (r) return r;
    std::vector<float4> h(plane * nspp);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->last_samp, h.size() * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int w = x1 - x0, hh = y1 - y0;
    const int tx = (w + 7) / 8;
    for (uint32_t k = 0; k < nspp; k++)
        for (int y = 0; y < hh; y++)
            for (int x = 0; x < w; x++) {
                const size_t tile = (size_t)(y / 8) * tx + (x / 8);
                const size_t lane = (size_t)(y % 8) * 8 + (x % 8);
                const float4 v = h[(size_t)k * plane + tile * 64 + lane];
                float* o = out + (((size_t)k * hh + y) * w + x) * 4;
                o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
            }
    return rmr_write_accum(c, keep.data(), keep.size() * sizeof(float));
}

// ---- camera models and caller-supplied rays (rmr_camera.hip, camera.cpp, rmr_trace.h RAYS) ---------
int rmr_set_camera_model(rmr_ctx* c, const rmr_camera_model* m) {
    if (!c || !m) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!rmr::camera_model_ok(*m))
        return fail(c, RMR_E_INVALID, "bad camera model (thin lens: aperture finite >= 0, focus finite > 0; ortho: width, "
                                      "height finite > 0)");
    c->camera = *m;
    return RMR_OK;
}

int rmr_get_camera_model(const rmr_ctx* c, rmr_camera_model* m) {
    if (!c || !m) return RMR_E_INVALID;
    *m = c->camera;
    return RMR_OK;
}

namespace {
// The generator kernels' second argument from the context's camera model and view.
int camera_params(rmr_ctx* c, rmr::CamParams& cam) {
    const rmr_camera_model& m = c->camera;
    cam = rmr::CamParams{};
    cam.model = m.model;
    cam.p[0] = m.aperture; cam.p[1] = m.focus; cam.p[2] = m.width; cam.p[3] = m.height;
    float f[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const bool eye_rays = m.model == RMR_CAMERA_VIEW || (m.model == RMR_CAMERA_THIN_LENS && m.aperture == 0.0f);
    if (!eye_rays && !rmr::camera_frame(c->view, f))
        return fail(c, RMR_E_INVALID, "the view has no camera frame (rmr_camera_frame): the camera model needs one");
    for (int k = 0; k < 3; k++) { cam.U[k] = f[k]; cam.V[k] = f[3 + k]; cam.F[k] = f[6 + k]; }
    return RMR_OK;
}
}  // namespace

int rmr_trace_rays(rmr_ctx* c, const rmr_ray* rays, size_t n, float* out_rgba) {
    if (!c || (n && (!rays || !out_rgba))) return RMR_E_INVALID;
    RMR_FLUSH(c);
    int r;
    if ((r = launch_precheck(c))) return r;
    if (c->params.separate_channels != 0)
        return fail(c, RMR_E_STATE, "rmr_trace_rays with separate_channels set: a caller's ray has no channel passes");
    if (n >= ((size_t)1 << 37)) return fail(c, RMR_E_INVALID, "rmr_trace_rays: too many rays");
    const long long bad = rmr::first_bad_ray(rays, n);
    if (bad >= 0)
        return fail(c, RMR_E_INVALID, "rmr_trace_rays: ray " + std::to_string(bad) + " fails rmr_check_rays");
    if (n == 0) return RMR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const RayList rl{rays, n, out_rgba, nullptr, nullptr, 0.0f};
    return render_tiles(c, std::vector<TileXY>(), 0, 0, 0, 0, nullptr, 0, 0, &rl);
}

int rmr_camera_rays(rmr_ctx* c, const float* times, uint32_t nspp, int x0, int y0, int x1, int y1, rmr_ray* out) {
    if (!c || (nspp && (!times || !out))) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!rmr::clamp_rect(c->W, c->H, x0, y0, x1, y1) || nspp == 0) return RMR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->view_set) default_view(c);
    rmr::CamParams cam{};
    int r;
    if ((r = camera_params(c, cam))) return r;
    const std::vector<TileXY> tiles = rect_tiles(x0, y0, x1, y1);
    const TileXY* d_tiles = nullptr;
    if ((r = tile_list(c, tiles, &d_tiles))) return r;
    KParams P;
    if ((r = view_params(c, P))) return r;
    P.x0 = x0; P.y0 = y0; P.x1 = x1; P.y1 = y1;
    P.tiles = d_tiles;
    P.n_tiles = (int)tiles.size();
    const size_t plane = tiles.size() * 64;
    const size_t chunk = rmr::plan_samples(plane, nspp, c->samp_budget, 0, rmr::kRayRecordBytes).per_launch;
    const int w = x1 - x0, hh = y1 - y0, tx = (w + 7) / 8;
    std::vector<float4> h;
    for (uint32_t k0 = 0; k0 < nspp; k0 += (uint32_t)chunk) {
        const uint32_t n = (uint32_t)std::min<size_t>(chunk, nspp - k0);
        if ((r = ensure_rays(c, plane * n))) return r;
        const float* d_times = nullptr;
        if (n > 1 && (r = stage_times(c, times + k0, n, &d_times))) return r;
        P.nspp = n;
        P.times = d_times;
        P.time1 = times[k0];
        P.n_units = (uint64_t)n * plane;
        HIPCHK(c, rmr::launch_camera_rays(P, cam, c->d_rays, c->stream));
        h.resize(3 * plane * n);
        HIPCHK(c, hipMemcpyAsync(h.data(), c->d_rays, h.size() * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < n; k++)
            for (int y = 0; y < hh; y++)
                for (int x = 0; x < w; x++) {
                    const size_t tile = (size_t)(y / 8) * tx + (x / 8), lane = (size_t)(y % 8) * 8 + (x % 8);
                    const float4* q = &h[3 * ((size_t)k * plane + tile * 64 + lane)];
                    rmr_ray& o = out[((size_t)(k0 + k) * hh + y) * w + x];
                    o.o[0] = q[0].x; o.o[1] = q[0].y; o.o[2] = q[0].z; o.time = q[0].w;
                    o.d[0] = q[1].x; o.d[1] = q[1].y; o.d[2] = q[1].z; o.rc = q[1].w;
                    o.gx = x0 + x;
                    o.gy = y0 + y;
                }
    }
    return RMR_OK;
}

// ---- first-hit and distance queries, device-resident ray lists (rmr_query.hip) -----
namespace {
// What the cast and eval kernels need: a scene, the counters, the launch parameters (the view is not read).
int query_begin(rmr_ctx* c, KParams& P) {
    if (!c->scene_loaded) return fail(c, RMR_E_STATE, "no scene loaded (call rmr_load_scene_json / rmr_load_builtin_scene)");
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if ((r = ensure_query(c))) return r;
    if (!c->view_set) default_view(c);
    return view_params(c, P);
}

// A host form's device copy of the caller's list or result: grows only, after the stream's work on it.
int ensure_qbuf(rmr_ctx* c, void** buf, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return RMR_OK;
    if (*buf) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(*buf);
        *buf = nullptr;
        *cap = 0;
    }
    if (hipMalloc(buf, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *buf = nullptr;
        return fail(c, RMR_E_NOMEM, "cannot allocate a query buffer (" + std::to_string(bytes) + " bytes)");
    }
    *cap = bytes;
    return RMR_OK;
}
}  // namespace

int rmr_cast_rays_device(rmr_ctx* c, const rmr_ray* d_rays, size_t n, int flags, rmr_hit* d_out) {
    if (!c || (n && (!d_rays || !d_out))) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (flags & ~RMR_CAST_NORMALS) return fail(c, RMR_E_INVALID, "rmr_cast_rays: unknown flags");
    KParams P;
    int r;
    if ((r = query_begin(c, P))) return r;
    HIPCHK(c, rmr::launch_cast_rays(P, c->accel.map_np, (flags & RMR_CAST_NORMALS) != 0, d_rays, n, d_out,
                                    c->d_query + kQueryRejects, c->d_query + kQueryFirstBad, c->query_grid, c->stream));
    return RMR_OK;
}

int rmr_eval_map_device(rmr_ctx* c, const float* d_xyz, size_t n, float* d_out) {
    if (!c || (n && (!d_xyz || !d_out))) return RMR_E_INVALID;
    RMR_FLUSH(c);
    KParams P;
    int r;
    if ((r = query_begin(c, P))) return r;
    HIPCHK(c, rmr::launch_eval_map(P, c->accel.map_np, d_xyz, n, d_out, c->query_grid, c->stream));
    return RMR_OK;
}

int rmr_cast_rays(rmr_ctx* c, const rmr_ray* rays, size_t n, int flags, rmr_hit* out) {
    if (!c || (n && (!rays || !out))) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (flags & ~RMR_CAST_NORMALS) return fail(c, RMR_E_INVALID, "rmr_cast_rays: unknown flags");
    KParams P;
    int r;
    if ((r = query_begin(c, P))) return r;
    if (n == 0) return RMR_OK;
    if ((r = ensure_qbuf(c, &c->d_qin, &c->qin_cap, n * sizeof(rmr_ray)))) return r;
    if ((r = ensure_qbuf(c, &c->d_qout, &c->qout_cap, n * sizeof(rmr_hit)))) return r;
    // the caller's list as it is; the kernel validates it and leaves the first failing index
    HIPCHK(c, hipMemcpyAsync(c->d_qin, rays, n * sizeof(rmr_ray), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_query + kQueryHostRejects, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_query + kQueryHostFirstBad, 0xff, sizeof(unsigned long long), c->stream));
    HIPCHK(c, rmr::launch_cast_rays(P, c->accel.map_np, (flags & RMR_CAST_NORMALS) != 0, (const rmr_ray*)c->d_qin, n,
                                    (rmr_hit*)c->d_qout, c->d_query + kQueryHostRejects, c->d_query + kQueryHostFirstBad,
                                    c->query_grid, c->stream));
    unsigned long long bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, c->d_query + kQueryHostFirstBad, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad != ~0ull) return fail(c, RMR_E_INVALID, "rmr_cast_rays: ray " + std::to_string(bad) + " fails rmr_check_rays");
    HIPCHK(c, hipMemcpyAsync(out, c->d_qout, n * sizeof(rmr_hit), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

int rmr_eval_map(rmr_ctx* c, const float* xyz, size_t n, float* out) {
    if (!c || (n && (!xyz || !out))) return RMR_E_INVALID;
    RMR_FLUSH(c);
    KParams P;
    int r;
    if ((r = query_begin(c, P))) return r;
    if (n == 0) return RMR_OK;
    if ((r = ensure_qbuf(c, &c->d_qin, &c->qin_cap, n * 3 * sizeof(float)))) return r;
    if ((r = ensure_qbuf(c, &c->d_qout, &c->qout_cap, n * 2 * sizeof(float)))) return r;
    HIPCHK(c, hipMemcpyAsync(c->d_qin, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, rmr::launch_eval_map(P, c->accel.map_np, (const float*)c->d_qin, n, (float*)c->d_qout, c->query_grid, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, c->d_qout, n * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

int rmr_trace_rays_device(rmr_ctx* c, const rmr_ray* d_rays, size_t n, float origin_extent, float* d_out_rgba) {
    if (!c || (n && (!d_rays || !d_out_rgba))) return RMR_E_INVALID;
    RMR_FLUSH(c);
    int r;
    if ((r = launch_precheck(c))) return r;
    if (c->params.separate_channels != 0)
        return fail(c, RMR_E_STATE, "rmr_trace_rays_device with separate_channels set: a caller's ray has no channel passes");
    if (n >= ((size_t)1 << 37)) return fail(c, RMR_E_INVALID, "rmr_trace_rays_device: too many rays");
    if (!rmr::extent_ok(origin_extent))
        return fail(c, RMR_E_INVALID, "rmr_trace_rays_device: origin_extent must be finite and >= 0");
    if (n == 0) return RMR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const RayList rl{nullptr, n, nullptr, d_rays, d_out_rgba, origin_extent};
    return render_tiles(c, std::vector<TileXY>(), 0, 0, 0, 0, nullptr, 0, 0, &rl);
}

int rmr_query_rejects(rmr_ctx* c, uint64_t* out) {
    if (!c || !out) return RMR_E_INVALID;
    RMR_FLUSH(c);
    *out = 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!c->d_query) return RMR_OK;
    unsigned long long v = 0;
    HIPCHK(c, hipMemcpyAsync(&v, c->d_query + kQueryRejects, sizeof(v), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_query + kQueryRejects, 0, sizeof(v), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = (uint64_t)v;
    return RMR_OK;
}

int rmr_set_query_grid(rmr_ctx* c, int blocks) {
    if (!c || blocks < 0) return RMR_E_INVALID;
    c->query_grid = blocks;
    return RMR_OK;
}

// ---- sampled AOVs (rmr_aov.hip, rmr_aov_rule.h) ---------------------------------
namespace {
constexpr uint64_t kAovMaxSamples = (uint64_t)1 << 24;   // float32 counts are exact up to here

// The five state planes, in the initial state, at first use.
int ensure_aov(rmr_ctx* c) {
    if (c->d_aov) return RMR_OK;
    const size_t n_px = (size_t)c->W * c->H;
    if (const int r = alloc_all(c, {{&c->d_aov, 5 * n_px * sizeof(float4)}},
                                "cannot allocate the sampled AOVs' state (W x H x 80 bytes)"))
        return r;
    c->aov_rendered = c->aov_res_valid = false;
    c->aov_samples = 0;
    HIPCHK(c, rmr::launch_aov_init(c->d_aov, n_px, c->stream));
    return RMR_OK;
}

// The resolved planes of the current state, queued on the context's stream unless they are that already.
int resolve_aov(rmr_ctx* c) {
    if (!c->d_aov || !c->aov_rendered) return fail(c, RMR_E_STATE, "no sampled AOVs (call rmr_render_aov)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_px = (size_t)c->W * c->H;
    if (!c->d_aov_res) {
        if (const int r = alloc_all(c, {{&c->d_aov_res, 5 * n_px * sizeof(float4)}},
                                    "cannot allocate the sampled AOVs' resolved planes (W x H x 80 bytes)"))
            return r;
        c->aov_res_valid = false;
    }
    if (c->aov_res_valid) return RMR_OK;
    HIPCHK(c, rmr::launch_aov_resolve(c->d_aov, n_px, c->params.max_dist, c->d_aov_res, c->stream));
    c->aov_res_valid = true;
    return RMR_OK;
}

bool aov_plane_ok(int plane) { return plane >= RMR_AOV_STATS && plane <= RMR_AOV_IDS23; }
}  // namespace

int rmr_render_aov(rmr_ctx* c, const float* times, uint32_t nspp, int x0, int y0, int x1, int y1, int restart) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if ((nspp == 0) != (times == nullptr))
        return fail(c, RMR_E_INVALID, "rmr_render_aov: times and nspp must both be given or both be empty");
    if (!c->scene_loaded) return fail(c, RMR_E_STATE, "no scene loaded (call rmr_load_scene_json / rmr_load_builtin_scene)");
    const bool whole = rmr::clamp_rect(c->W, c->H, x0, y0, x1, y1) && x0 == 0 && y0 == 0 && x1 == c->W && y1 == c->H;
    const uint64_t before = (restart && whole) ? 0 : c->aov_samples;
    if (before + nspp > kAovMaxSamples)
        return fail(c, RMR_E_INVALID, "rmr_render_aov: more than 2^24 samples per pixel (restart, or call rmr_aov_reset)");
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if ((r = ensure_aov(c))) return r;
    c->aov_rendered = true;
    if (x0 >= x1 || y0 >= y1 || (nspp == 0 && !restart)) return RMR_OK;
    if (!c->view_set) default_view(c);
    rmr::CamParams cam{};
    if ((r = camera_params(c, cam))) return r;
    KParams P;
    if ((r = view_params(c, P))) return r;
    P.x0 = x0; P.y0 = y0; P.x1 = x1; P.y1 = y1;
    c->aov_res_valid = false;
    c->aov_samples = before + nspp;
    const uint32_t per = (uint32_t)std::max(1, c->aov_launch_samples);
    uint32_t k0 = 0;
    do {   // (once with no samples for a bare restart)
        const uint32_t n = std::min(per, nspp - k0);
        const float* d_times = nullptr;
        if (n > 1 && (r = stage_times(c, times + k0, n, &d_times))) return r;
        P.nspp = n;
        P.times = d_times;
        P.time1 = n ? times[k0] : 0.0f;
        HIPCHK(c, rmr::launch_aov(P, cam, c->accel.map_np, c->d_aov, restart != 0 && k0 == 0, c->stream));
        k0 += n;
    } while (k0 < nspp);
    return RMR_OK;
}

int rmr_aov_reset(rmr_ctx* c) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    c->aov_samples = 0;
    if (!c->d_aov) return RMR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    c->aov_res_valid = false;
    HIPCHK(c, rmr::launch_aov_init(c->d_aov, (size_t)c->W * c->H, c->stream));
    return RMR_OK;
}

int rmr_read_aov(rmr_ctx* c, int plane, float* rgba, size_t bytes) {
    if (!c || !rgba) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!aov_plane_ok(plane)) return fail(c, RMR_E_INVALID, "bad sampled-AOV plane");
    const size_t n_px = (size_t)c->W * c->H;
    if (bytes != n_px * sizeof(float4)) return fail(c, RMR_E_INVALID, "rmr_read_aov: bytes must be W x H x 16");
    if (!c->d_aov || !c->aov_rendered) return fail(c, RMR_E_STATE, "no sampled AOVs (call rmr_render_aov)");
    HIPCHK(c, hipSetDevice(c->device));
    return read_back(c, rgba, c->d_aov + (size_t)plane * n_px, bytes);
}

int rmr_read_aov_resolved(rmr_ctx* c, int which, float* rgba, size_t bytes) {
    if (!c || !rgba) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!aov_plane_ok(which)) return fail(c, RMR_E_INVALID, "bad sampled-AOV plane");
    const size_t n_px = (size_t)c->W * c->H;
    if (bytes != n_px * sizeof(float4)) return fail(c, RMR_E_INVALID, "rmr_read_aov_resolved: bytes must be W x H x 16");
    if (const int r = resolve_aov(c)) return r;
    return read_back(c, rgba, c->d_aov_res + (size_t)which * n_px, bytes);
}

void* rmr_aov_device_ptr(rmr_ctx* c, int plane) {
    if (!c || !aov_plane_ok(plane)) return nullptr;
    if (!flushed(c)) return nullptr;
    if (hipSetDevice(c->device) != hipSuccess || ensure_aov(c) != RMR_OK) return nullptr;
    return (void*)(c->d_aov + (size_t)plane * c->W * c->H);
}

void* rmr_aov_resolved_device_ptr(rmr_ctx* c, int which) {
    if (!c || !aov_plane_ok(which)) return nullptr;
    if (!flushed(c)) return nullptr;
    if (resolve_aov(c) != RMR_OK) return nullptr;
    return (void*)(c->d_aov_res + (size_t)which * c->W * c->H);
}

int rmr_set_aov_launch_samples(rmr_ctx* c, int n) {
    if (!c || n < 1) return RMR_E_INVALID;
    c->aov_launch_samples = n;
    return RMR_OK;
}

// ---- SDF volume sampling and surface-nets extraction (rmr_volume.hip, rmr_mesh_rule.h) ----
namespace {
int volume_begin(rmr_ctx* c, const char* who, const rmr_volume_desc* desc, KParams& P) {
    const char* bad = nullptr;
    if (rmr_check_volume(desc, &bad) != RMR_OK)
        return fail(c, RMR_E_INVALID, std::string(who) + ": bad volume descriptor field '" + bad + "'");
    return query_begin(c, P);
}
size_t volume_points(const rmr_volume_desc* d) { return (size_t)d->n[0] * (size_t)d->n[1] * (size_t)d->n[2]; }
}  // namespace

int rmr_sample_volume_device(rmr_ctx* c, const rmr_volume_desc* desc, float* d_dist, float* d_id) {
    if (!c || !desc || !d_dist) return RMR_E_INVALID;
    RMR_FLUSH(c);
    KParams P;
    int r;
    if ((r = volume_begin(c, "rmr_sample_volume_device", desc, P))) return r;
    HIPCHK(c, rmr::launch_sample_volume(P, c->accel.map_np, *desc, d_dist, d_id, c->query_grid, c->stream));
    return RMR_OK;
}

int rmr_sample_volume(rmr_ctx* c, const rmr_volume_desc* desc, float* dist, float* id) {
    if (!c || !desc || !dist) return RMR_E_INVALID;
    RMR_FLUSH(c);
    KParams P;
    int r;
    if ((r = volume_begin(c, "rmr_sample_volume", desc, P))) return r;
    const size_t n = volume_points(desc);
    if ((r = ensure_qbuf(c, &c->d_qout, &c->qout_cap, n * (id ? 2 : 1) * sizeof(float)))) return r;
    float* d_dist = (float*)c->d_qout;
    float* d_id = id ? d_dist + n : nullptr;
    HIPCHK(c, rmr::launch_sample_volume(P, c->accel.map_np, *desc, d_dist, d_id, c->query_grid, c->stream));
    HIPCHK(c, hipMemcpyAsync(dist, d_dist, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (id) HIPCHK(c, hipMemcpyAsync(id, d_id, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

int rmr_extract_mesh(rmr_ctx* c, const rmr_volume_desc* desc, const rmr_mesh_params* mp, rmr_mesh_info* info) {
    if (!c || !desc || !mp || !info) return RMR_E_INVALID;
    RMR_FLUSH(c);
    info->n_vertices = info->n_quads = 0;
    c->mesh_valid = false;   // (whatever happens from here on, the last mesh is gone; its buffers go below or with the next free)
    if (!(mp->iso - mp->iso == 0.0f)) return fail(c, RMR_E_INVALID, "rmr_extract_mesh: iso must be finite");
    if (mp->flags & ~(RMR_MESH_NORMALS | RMR_MESH_IDS)) return fail(c, RMR_E_INVALID, "rmr_extract_mesh: unknown flags");
    KParams P;
    int r;
    if ((r = volume_begin(c, "rmr_extract_mesh", desc, P))) return r;
    if (c->d_mesh_v || c->d_mesh_q) HIPCHK(c, hipStreamSynchronize(c->stream));   // (the last mesh's queued work)
    drop_mesh(c);
    // the working memory: distances, a flag byte and a cell number per point; block totals, group totals,
    // the groups' bases and the two counts
    const size_t n = volume_points(desc);
    const uint32_t blocks = rmr::mesh_blocks(*desc), groups = rmr::mesh_scan_groups(blocks);
    const size_t scan_bytes = ((size_t)blocks + groups) * sizeof(uint2) + ((size_t)groups * 2 + 2) * sizeof(unsigned long long);
    if ((r = ensure_qbuf(c, &c->d_mesh_dist, &c->mesh_dist_cap, n * sizeof(float)))) return r;
    if ((r = ensure_qbuf(c, &c->d_mesh_flag, &c->mesh_flag_cap, n))) return r;
    if ((r = ensure_qbuf(c, &c->d_mesh_cell, &c->mesh_cell_cap, n * sizeof(uint32_t)))) return r;
    if ((r = ensure_qbuf(c, &c->d_mesh_scan, &c->mesh_scan_cap, scan_bytes))) return r;
    float* dist = (float*)c->d_mesh_dist;
    uint8_t* flags = (uint8_t*)c->d_mesh_flag;
    uint2* totals = (uint2*)c->d_mesh_scan;
    uint2* group_totals = totals + blocks;
    unsigned long long* bases = (unsigned long long*)(group_totals + groups);
    unsigned long long* d_counts = bases + 2 * (size_t)groups;
    HIPCHK(c, rmr::launch_sample_volume(P, c->accel.map_np, *desc, dist, nullptr, c->query_grid, c->stream));
    HIPCHK(c, rmr::launch_mesh_count(*desc, dist, mp->iso, flags, totals, group_totals, bases, d_counts, c->stream));
    unsigned long long counts[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // the call's one synchronisation: the counts size the buffers
    const unsigned long long nv = counts[0], nq = counts[1];
    if (nv >= (1ull << 32) || nq >= (1ull << 32)) return fail(c, RMR_E_INVALID, "rmr_extract_mesh: 2^32 or more vertices or quads");
    auto get = [&](auto** p, size_t bytes) {
        if (bytes == 0 || hipMalloc((void**)p, bytes) == hipSuccess) return true;
        (void)hipGetLastError();
        *p = nullptr;
        return false;
    };
    if (!get(&c->d_mesh_v, nv * 3 * sizeof(float)) || !get(&c->d_mesh_q, nq * 4 * sizeof(uint32_t)) ||
        !get(&c->d_mesh_n, (mp->flags & RMR_MESH_NORMALS) ? nv * 3 * sizeof(float) : 0) ||
        !get(&c->d_mesh_id, (mp->flags & RMR_MESH_IDS) ? nv * sizeof(float) : 0)) {
        drop_mesh(c);
        return fail(c, RMR_E_NOMEM, "rmr_extract_mesh: cannot allocate the mesh (" + std::to_string(nv) + " vertices, " +
                                        std::to_string(nq) + " quads)");
    }
    if (nv) {
        HIPCHK(c, rmr::launch_mesh_emit(*desc, dist, mp->iso, flags, totals, bases, (uint32_t*)c->d_mesh_cell, c->d_mesh_v,
                                        c->d_mesh_q, c->stream));
        HIPCHK(c, rmr::launch_mesh_attr(P, c->accel.map_np, c->d_mesh_v, (uint32_t)nv, c->d_mesh_n, c->d_mesh_id, c->stream));
    }
    c->mesh_valid = true;
    c->mesh_desc = *desc;
    c->mesh_flags = mp->flags;
    c->mesh_nv = info->n_vertices = nv;
    c->mesh_nq = info->n_quads = nq;
    return RMR_OK;
}

int rmr_read_mesh(rmr_ctx* c, float* vertices, float* normals, float* ids, uint32_t* quads) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!c->mesh_valid) return fail(c, RMR_E_STATE, "no mesh (call rmr_extract_mesh)");
    if ((normals && !(c->mesh_flags & RMR_MESH_NORMALS)) || (ids && !(c->mesh_flags & RMR_MESH_IDS)))
        return fail(c, RMR_E_STATE, "rmr_read_mesh: the attribute was not extracted (rmr_mesh_params.flags)");
    if ((c->mesh_nv && !vertices) || (c->mesh_nq && !quads)) return fail(c, RMR_E_INVALID, "rmr_read_mesh: null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nv = (size_t)c->mesh_nv, nq = (size_t)c->mesh_nq;
    if (nv) HIPCHK(c, hipMemcpyAsync(vertices, c->d_mesh_v, nv * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (nv && normals) HIPCHK(c, hipMemcpyAsync(normals, c->d_mesh_n, nv * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (nv && ids) HIPCHK(c, hipMemcpyAsync(ids, c->d_mesh_id, nv * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (nq) HIPCHK(c, hipMemcpyAsync(quads, c->d_mesh_q, nq * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

void* rmr_mesh_device_ptr(rmr_ctx* c, int which) {
    if (!c || !c->mesh_valid) return nullptr;
    switch (which) {
    case RMR_MESH_BUF_VERTICES: return c->d_mesh_v;
    case RMR_MESH_BUF_NORMALS: return c->d_mesh_n;
    case RMR_MESH_BUF_IDS: return c->d_mesh_id;
    case RMR_MESH_BUF_QUADS: return c->d_mesh_q;
    default: return nullptr;
    }
}

int rmr_mesh_free(rmr_ctx* c) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_mesh(c);
    return RMR_OK;
}

// ---- light baking at surface points and mesh vertices (rmr_bake.hip, rmr_bake_rule.h) ----
namespace {
// The call's params (NULL: the defaults) and counts, checked.
int bake_args(rmr_ctx* c, const char* who, size_t n, const float* times, uint32_t nspp, const rmr_bake_params* params,
              rmr_bake_params& q) {
    if (params) q = *params;
    else rmr_default_bake_params(&q);
    if (rmr_check_bake_params(&q) != RMR_OK)
        return fail(c, RMR_E_INVALID, std::string(who) + ": params fail rmr_check_bake_params (flags, bias, ao_distance, first_index)");
    if (nspp == 0 || nspp > (1u << 24) || !times) return fail(c, RMR_E_INVALID, std::string(who) + ": 1 <= nspp <= 2^24 seeds");
    if ((uint64_t)n > rmr::kBakeMaxIndex - q.first_index)
        return fail(c, RMR_E_INVALID, std::string(who) + ": first_index + n exceeds 2^36");
    if ((((uint64_t)n + 63) / 64) * (uint64_t)nspp >= ((uint64_t)1 << 32))
        return fail(c, RMR_E_INVALID, std::string(who) + ": ceil(n / 64) nspp must stay below 2^32 (bake slices, first_index)");
    return RMR_OK;
}

// The bake of a device list, queued: the radiance through render_tiles' plan and launches, the occlusion by
// launches of its own kernel under the same budget (8 bytes per ray), each followed by its fold.
int bake_device(rmr_ctx* c, const char* who, const float* d_points, const float* d_normals, size_t n, const float* times,
                uint32_t nspp, const rmr_bake_params& q, float* d_rgba, float* d_ao) {
    int r;
    if ((r = launch_precheck(c))) return r;
    if (c->params.separate_channels != 0)
        return fail(c, RMR_E_STATE, std::string(who) + " with separate_channels set: a bake's ray has no channel passes");
    if (!rmr::extent_ok(q.origin_extent))
        return fail(c, RMR_E_INVALID, std::string(who) + ": origin_extent must be finite and >= 0");
    if (n == 0) return RMR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if ((r = ensure_query(c))) return r;
    if ((r = ensure_qbuf(c, &c->d_bake_state, &c->bake_state_cap, n * sizeof(float4)))) return r;
    BakeJob job{{d_points, d_normals, (uint64_t)n, q.first_index, nullptr, nspp, q.bias, q.origin_extent}, times,
                (float4*)c->d_bake_state};
    const size_t n_ts = ((n + 63) / 64) * (size_t)nspp;
    if (q.flags & RMR_BAKE_RADIANCE) {
        const RayList rl{nullptr, n_ts, nullptr, nullptr, d_rgba, q.origin_extent, &job};
        if ((r = render_tiles(c, std::vector<TileXY>(), 0, 0, 0, 0, nullptr, 0, 0, &rl))) return r;
    }
    if (q.flags & RMR_BAKE_AO) {
        if (!c->view_set) default_view(c);
        KParams P;
        if ((r = view_params(c, P, (double)q.origin_extent))) return r;   // (the bound of the radiance pass: no new boxes)
        if ((r = stage_times(c, times, nspp, &job.list.times))) return r;
        // a point is counted as rejected once per call: by the radiance pass where there is one
        unsigned long long* rejects = (q.flags & RMR_BAKE_RADIANCE) ? nullptr : c->d_query + kQueryRejects;
        // (fewer than 2^31 units per launch, as the trace's: the kernels index a launch's units with 32 bits)
        const size_t chunk = rmr::plan_samples(64, (uint32_t)n_ts, c->samp_budget, 0, sizeof(float2)).per_launch;
        for (size_t k0 = 0; k0 < n_ts; k0 += chunk) {
            const uint32_t cnt = (uint32_t)std::min(chunk, n_ts - k0);
            if ((r = ensure_samp(c, ((size_t)cnt * 64 + 1) / 2))) return r;
            c->last_samp = c->d_samp;
            HIPCHK(c, rmr::launch_bake_ao(P, c->accel.map_np, job.list, q.ao_distance, k0, cnt, (float2*)c->d_samp, rejects,
                                          c->query_grid, c->stream));
            HIPCHK(c, rmr::launch_bake_fold(true, c->d_samp, nullptr, job.state, n, nspp, k0, cnt, d_ao, c->stream));
        }
    }
    return RMR_OK;
}
}  // namespace

int rmr_bake_points_device(rmr_ctx* c, const float* d_points, const float* d_normals, size_t n, const float* times,
                           uint32_t nspp, const rmr_bake_params* params, float* d_out_rgba, float* d_out_ao) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_bake_params q;
    int r;
    if ((r = bake_args(c, "rmr_bake_points_device", n, times, nspp, params, q))) return r;
    if (n && (!d_points || !d_normals || ((q.flags & RMR_BAKE_RADIANCE) && !d_out_rgba) || ((q.flags & RMR_BAKE_AO) && !d_out_ao)))
        return fail(c, RMR_E_INVALID, "rmr_bake_points_device: null buffer");
    return bake_device(c, "rmr_bake_points_device", d_points, d_normals, n, times, nspp, q, d_out_rgba, d_out_ao);
}

int rmr_bake_points(rmr_ctx* c, const float* points, const float* normals, size_t n, const float* times, uint32_t nspp,
                    const rmr_bake_params* params, float* out_rgba, float* out_ao) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_bake_params q;
    int r;
    if ((r = bake_args(c, "rmr_bake_points", n, times, nspp, params, q))) return r;
    const bool rad = (q.flags & RMR_BAKE_RADIANCE) != 0, ao = (q.flags & RMR_BAKE_AO) != 0;
    if (n && (!points || !normals || (rad && !out_rgba) || (ao && !out_ao))) return fail(c, RMR_E_INVALID, "rmr_bake_points: null buffer");
    // the origins' bound, over the points the rule uses
    float ext = 0.0f;
    for (size_t i = 0; i < n; i++) {
        if (!rmr::bake_point_ok(points + 3 * i, normals + 3 * i)) continue;
        float o[3];
        rmr::bake_origin(points + 3 * i, normals + 3 * i, q.bias, o);
        for (int k = 0; k < 3; k++) ext = std::max(ext, std::fabs(o[k]));
    }
    q.origin_extent = ext;
    if (!rmr::extent_ok(ext)) return fail(c, RMR_E_INVALID, "rmr_bake_points: a ray origin (p + bias n) is not finite");
    if ((r = launch_precheck(c))) return r;
    if (n == 0) return bake_device(c, "rmr_bake_points", nullptr, nullptr, 0, times, nspp, q, nullptr, nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    if ((r = ensure_qbuf(c, &c->d_qin, &c->qin_cap, n * 6 * sizeof(float)))) return r;
    if ((r = ensure_qbuf(c, &c->d_qout, &c->qout_cap, n * 5 * sizeof(float)))) return r;
    float* d_p = (float*)c->d_qin;
    float* d_n = d_p + 3 * n;
    float* d_rgba = (float*)c->d_qout;
    float* d_ao = d_rgba + 4 * n;
    HIPCHK(c, hipMemcpyAsync(d_p, points, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_n, normals, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((r = bake_device(c, "rmr_bake_points", d_p, d_n, n, times, nspp, q, d_rgba, d_ao))) return r;
    if (rad) HIPCHK(c, hipMemcpyAsync(out_rgba, d_rgba, n * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (ao) HIPCHK(c, hipMemcpyAsync(out_ao, d_ao, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

int rmr_bake_rays_device(rmr_ctx* c, const float* d_points, const float* d_normals, size_t n, const float* times,
                         uint32_t nspp, const rmr_bake_params* params, rmr_ray* d_out) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_bake_params q;
    int r;
    if ((r = bake_args(c, "rmr_bake_rays_device", n, times, nspp, params, q))) return r;
    if (n && (!d_points || !d_normals || !d_out)) return fail(c, RMR_E_INVALID, "rmr_bake_rays_device: null buffer");
    if (n == 0) return RMR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if ((r = ensure_query(c))) return r;
    rmr::BakeList B{d_points, d_normals, (uint64_t)n, q.first_index, nullptr, nspp, q.bias, INFINITY};
    if ((r = stage_times(c, times, nspp, &B.times))) return r;
    HIPCHK(c, rmr::launch_bake_ray_list(B, d_out, c->d_query + kQueryRejects, c->stream));
    return RMR_OK;
}

int rmr_bake_mesh(rmr_ctx* c, const float* times, uint32_t nspp, const rmr_bake_params* params) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!c->mesh_valid) return fail(c, RMR_E_STATE, "no mesh (call rmr_extract_mesh)");
    if (!(c->mesh_flags & RMR_MESH_NORMALS)) return fail(c, RMR_E_STATE, "rmr_bake_mesh: the mesh has no normals (RMR_MESH_NORMALS)");
    rmr_bake_params q;
    int r;
    const size_t nv = (size_t)c->mesh_nv;
    if ((r = bake_args(c, "rmr_bake_mesh", nv, times, nspp, params, q))) return r;
    // every vertex lies in the lattice's box; |n| is 1 to the reject rule's 1e-6
    double ext = 0.0;
    for (int a = 0; a < 3; a++) {
        const double lo = (double)c->mesh_desc.origin[a];
        const double hi = lo + (double)(c->mesh_desc.n[a] - 1) * (double)c->mesh_desc.spacing;
        ext = std::max(ext, std::max(std::fabs(lo), std::fabs(hi)));
    }
    ext = (ext + 2.0 * std::fabs((double)q.bias)) * (1.0 + 0x1p-20);
    q.origin_extent = std::nextafter((float)ext, INFINITY);
    HIPCHK(c, hipSetDevice(c->device));
    if (nv && (q.flags & RMR_BAKE_RADIANCE) && !c->d_mesh_rgba &&
        (r = alloc_all(c, {{&c->d_mesh_rgba, nv * 4 * sizeof(float)}}, "rmr_bake_mesh: cannot allocate the colours")))
        return r;
    if (nv && (q.flags & RMR_BAKE_AO) && !c->d_mesh_ao &&
        (r = alloc_all(c, {{&c->d_mesh_ao, nv * sizeof(float)}}, "rmr_bake_mesh: cannot allocate the occlusion")))
        return r;
    if ((r = bake_device(c, "rmr_bake_mesh", c->d_mesh_v, c->d_mesh_n, nv, times, nspp, q, c->d_mesh_rgba, c->d_mesh_ao))) return r;
    c->mesh_baked |= q.flags;
    return RMR_OK;
}

int rmr_read_mesh_bake(rmr_ctx* c, float* rgba, float* ao) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!c->mesh_valid) return fail(c, RMR_E_STATE, "no mesh (call rmr_extract_mesh)");
    if ((rgba && !(c->mesh_baked & RMR_BAKE_RADIANCE)) || (ao && !(c->mesh_baked & RMR_BAKE_AO)))
        return fail(c, RMR_E_STATE, "rmr_read_mesh_bake: not baked (rmr_bake_mesh and its flags)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nv = (size_t)c->mesh_nv;
    if (nv && rgba) HIPCHK(c, hipMemcpyAsync(rgba, c->d_mesh_rgba, nv * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (nv && ao) HIPCHK(c, hipMemcpyAsync(ao, c->d_mesh_ao, nv * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

void* rmr_mesh_bake_device_ptr(rmr_ctx* c, int which) {
    if (!c || !c->mesh_valid) return nullptr;
    if (which == RMR_MESH_BAKE_RGBA && (c->mesh_baked & RMR_BAKE_RADIANCE)) return c->d_mesh_rgba;
    if (which == RMR_MESH_BAKE_AO && (c->mesh_baked & RMR_BAKE_AO)) return c->d_mesh_ao;
    return nullptr;
}

// ---- irradiance probes (rmr_probe.hip, rmr_probe_rule.h) ----------------------------------
namespace {
// The call's params (NULL: the defaults) and counts, checked as bake_args checks a bake's.
int probe_args(rmr_ctx* c, const char* who, size_t n, const float* times, uint32_t nspp, const rmr_probe_params* params,
               rmr_probe_params& q) {
    if (params) q = *params;
    else rmr_default_probe_params(&q);
    if (rmr_check_probe_params(&q) != RMR_OK)
        return fail(c, RMR_E_INVALID, std::string(who) + ": params fail rmr_check_probe_params (clearance, first_index)");
    if (nspp == 0 || nspp > (1u << 24) || !times) return fail(c, RMR_E_INVALID, std::string(who) + ": 1 <= nspp <= 2^24 seeds");
    if ((uint64_t)n > rmr::kBakeMaxIndex - q.first_index)
        return fail(c, RMR_E_INVALID, std::string(who) + ": first_index + n exceeds 2^36");
    if ((((uint64_t)n + 63) / 64) * (uint64_t)nspp >= ((uint64_t)1 << 32))
        return fail(c, RMR_E_INVALID, std::string(who) + ": ceil(n / 64) nspp must stay below 2^32 (bake slices, first_index)");
    return RMR_OK;
}

rmr::ProbeList probe_list(const float* d_points, const rmr_volume_desc* desc, size_t n, uint32_t nspp, const rmr_probe_params& q,
                          float extent) {
    rmr::ProbeList B{};
    B.points = d_points;
    if (desc) {
        for (int a = 0; a < 3; a++) B.origin[a] = desc->origin[a];
        B.spacing = desc->spacing;
        B.nx = desc->n[0];
        B.ny = desc->n[1];
    }
    B.n = (uint64_t)n;
    B.first_index = q.first_index;
    B.nspp = nspp;
    B.clearance = q.clearance;
    B.extent = extent;
    return B;
}

// The bake of a device list (d_points) or of a lattice's points (desc), queued: render_tiles' plan and launches,
// as the light bake's radiance pass.
int probe_bake_device(rmr_ctx* c, const char* who, const float* d_points, const rmr_volume_desc* desc, size_t n,
                      const float* times, uint32_t nspp, const rmr_probe_params& q, float* d_out) {
    int r;
    if ((r = launch_precheck(c))) return r;
    if (c->params.separate_channels != 0)
        return fail(c, RMR_E_STATE, std::string(who) + " with separate_channels set: a probe's ray has no channel passes");
    if (!rmr::extent_ok(q.origin_extent))
        return fail(c, RMR_E_INVALID, std::string(who) + ": origin_extent must be finite and >= 0");
    if (n == 0) return RMR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if ((r = ensure_query(c))) return r;
    if ((r = ensure_qbuf(c, &c->d_probe_state, &c->probe_state_cap, n * rmr::kProbeSH * sizeof(float4)))) return r;
    rmr::ProbeList B = probe_list(d_points, desc, n, nspp, q, q.origin_extent);
    BakeJob job{{nullptr, nullptr, (uint64_t)n, q.first_index, nullptr, nspp, 0.0f, q.origin_extent}, times,
                (float4*)c->d_probe_state, &B};
    const size_t n_ts = ((n + 63) / 64) * (size_t)nspp;
    const RayList rl{nullptr, n_ts, nullptr, nullptr, d_out, q.origin_extent, &job};
    return render_tiles(c, std::vector<TileXY>(), 0, 0, 0, 0, nullptr, 0, 0, &rl);
}

// the bound on |coordinate| over a lattice's points: the box's largest, times 1 + 2^-20, rounded up
float lattice_extent(const rmr_volume_desc& d) {
    double ext = 0.0;
    for (int a = 0; a < 3; a++) {
        const double lo = (double)d.origin[a];
        const double hi = lo + (double)(d.n[a] - 1) * (double)d.spacing;
        ext = std::max(ext, std::max(std::fabs(lo), std::fabs(hi)));
    }
    return std::nextafter((float)(ext * (1.0 + 0x1p-20)), INFINITY);
}

// A new field for the lattice (the last one is gone, whatever happens from here on).
int probe_field_alloc(rmr_ctx* c, const char* who, const rmr_volume_desc* desc) {
    const char* bad = nullptr;
    if (rmr_check_volume(desc, &bad) != RMR_OK)
        return fail(c, RMR_E_INVALID, std::string(who) + ": bad volume descriptor field '" + bad + "'");
    HIPCHK(c, hipSetDevice(c->device));
    c->probe_valid = false;
    c->probe_vis_valid = false;   // (a new field has no visibility)
    if (c->d_probe_field || c->d_probe_vis) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        free_all({&c->d_probe_field, &c->d_probe_vis});
    }
    return alloc_all(c, {{&c->d_probe_field, volume_points(desc) * rmr::kProbeFloats * sizeof(float)}},
                     "cannot allocate the probe field");
}
}  // namespace

int rmr_bake_probes_device(rmr_ctx* c, const float* d_points, size_t n, const float* times, uint32_t nspp,
                           const rmr_probe_params* params, float* d_out_sh) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_probe_params q;
    int r;
    if ((r = probe_args(c, "rmr_bake_probes_device", n, times, nspp, params, q))) return r;
    if (n && (!d_points || !d_out_sh)) return fail(c, RMR_E_INVALID, "rmr_bake_probes_device: null buffer");
    return probe_bake_device(c, "rmr_bake_probes_device", d_points, nullptr, n, times, nspp, q, d_out_sh);
}

int rmr_bake_probes(rmr_ctx* c, const float* points, size_t n, const float* times, uint32_t nspp,
                    const rmr_probe_params* params, float* out_sh) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_probe_params q;
    int r;
    if ((r = probe_args(c, "rmr_bake_probes", n, times, nspp, params, q))) return r;
    if (n && (!points || !out_sh)) return fail(c, RMR_E_INVALID, "rmr_bake_probes: null buffer");
    // the probes' bound, over the finite ones
    float ext = 0.0f;
    for (size_t i = 0; i < 3 * n; i++)
        if (std::isfinite(points[i])) ext = std::max(ext, std::fabs(points[i]));
    q.origin_extent = ext;
    if ((r = launch_precheck(c))) return r;
    if (n == 0) return probe_bake_device(c, "rmr_bake_probes", nullptr, nullptr, 0, times, nspp, q, nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    if ((r = ensure_qbuf(c, &c->d_qin, &c->qin_cap, n * 3 * sizeof(float)))) return r;
    if ((r = ensure_qbuf(c, &c->d_qout, &c->qout_cap, n * rmr::kProbeFloats * sizeof(float)))) return r;
    HIPCHK(c, hipMemcpyAsync(c->d_qin, points, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((r = probe_bake_device(c, "rmr_bake_probes", (const float*)c->d_qin, nullptr, n, times, nspp, q, (float*)c->d_qout))) return r;
    HIPCHK(c, hipMemcpyAsync(out_sh, c->d_qout, n * rmr::kProbeFloats * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

int rmr_probe_rays_device(rmr_ctx* c, const float* d_points, size_t n, const float* times, uint32_t nspp,
                          const rmr_probe_params* params, rmr_ray* d_out) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_probe_params q;
    int r;
    if ((r = probe_args(c, "rmr_probe_rays_device", n, times, nspp, params, q))) return r;
    if (n && (!d_points || !d_out)) return fail(c, RMR_E_INVALID, "rmr_probe_rays_device: null buffer");
    KParams P;
    if ((r = query_begin(c, P))) return r;
    if (n == 0) return RMR_OK;
    rmr::ProbeList B = probe_list(d_points, nullptr, n, nspp, q, INFINITY);
    if ((r = stage_times(c, times, nspp, &B.times))) return r;
    HIPCHK(c, rmr::launch_probe_ray_list(P, c->accel.map_np, B, d_out, c->d_query + kQueryRejects, c->stream));
    return RMR_OK;
}

int rmr_bake_probe_field(rmr_ctx* c, const rmr_volume_desc* desc, const float* times, uint32_t nspp,
                         const rmr_probe_params* params) {
    if (!c || !desc) return RMR_E_INVALID;
    RMR_FLUSH(c);
    const char* bad = nullptr;
    if (rmr_check_volume(desc, &bad) != RMR_OK)
        return fail(c, RMR_E_INVALID, std::string("rmr_bake_probe_field: bad volume descriptor field '") + bad + "'");
    rmr_probe_params q;
    int r;
    const size_t n = volume_points(desc);
    if ((r = probe_args(c, "rmr_bake_probe_field", n, times, nspp, params, q))) return r;
    if (q.first_index != 0) return fail(c, RMR_E_INVALID, "rmr_bake_probe_field: first_index must be 0");
    q.origin_extent = lattice_extent(*desc);
    if ((r = launch_precheck(c))) return r;
    if (c->params.separate_channels != 0)
        return fail(c, RMR_E_STATE, "rmr_bake_probe_field with separate_channels set: a probe's ray has no channel passes");
    if (!rmr::extent_ok(q.origin_extent)) return fail(c, RMR_E_INVALID, "rmr_bake_probe_field: the lattice's box is not finite");
    if ((r = probe_field_alloc(c, "rmr_bake_probe_field", desc))) return r;
    if ((r = probe_bake_device(c, "rmr_bake_probe_field", nullptr, desc, n, times, nspp, q, c->d_probe_field))) return r;
    c->probe_desc = *desc;
    c->probe_valid = true;
    return RMR_OK;
}

int rmr_write_probe_field(rmr_ctx* c, const rmr_volume_desc* desc, const float* sh) {
    if (!c || !desc || !sh) return RMR_E_INVALID;
    RMR_FLUSH(c);
    int r;
    if ((r = probe_field_alloc(c, "rmr_write_probe_field", desc))) return r;
    HIPCHK(c, hipMemcpyAsync(c->d_probe_field, sh, volume_points(desc) * rmr::kProbeFloats * sizeof(float),
                             hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->probe_desc = *desc;
    c->probe_valid = true;
    return RMR_OK;
}

int rmr_read_probe_field(rmr_ctx* c, rmr_volume_desc* desc_out, float* sh) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!c->probe_valid) return fail(c, RMR_E_STATE, "no probe field (call rmr_bake_probe_field / rmr_write_probe_field)");
    HIPCHK(c, hipSetDevice(c->device));
    if (desc_out) *desc_out = c->probe_desc;
    if (sh)
        HIPCHK(c, hipMemcpyAsync(sh, c->d_probe_field, volume_points(&c->probe_desc) * rmr::kProbeFloats * sizeof(float),
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

void* rmr_probe_field_device_ptr(rmr_ctx* c) { return c && c->probe_valid ? c->d_probe_field : nullptr; }

int rmr_probe_field_free(rmr_ctx* c) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_probes(c);
    return RMR_OK;
}

int rmr_probe_irradiance_device(rmr_ctx* c, const float* d_points, const float* d_normals, size_t n, float* d_out_rgba) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (n && (!d_points || !d_normals || !d_out_rgba)) return fail(c, RMR_E_INVALID, "rmr_probe_irradiance_device: null buffer");
    if (!c->probe_valid) return fail(c, RMR_E_STATE, "no probe field (call rmr_bake_probe_field / rmr_write_probe_field)");
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if ((r = ensure_query(c))) return r;
    HIPCHK(c, rmr::launch_probe_lookup(c->probe_desc, c->d_probe_field, d_points, d_normals, (uint64_t)n, d_out_rgba,
                                       c->d_query + kQueryRejects, c->stream));
    return RMR_OK;
}

int rmr_probe_irradiance(rmr_ctx* c, const float* points, const float* normals, size_t n, float* out_rgba) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (n && (!points || !normals || !out_rgba)) return fail(c, RMR_E_INVALID, "rmr_probe_irradiance: null buffer");
    if (!c->probe_valid) return fail(c, RMR_E_STATE, "no probe field (call rmr_bake_probe_field / rmr_write_probe_field)");
    if (n == 0) return RMR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if ((r = ensure_qbuf(c, &c->d_qin, &c->qin_cap, n * 6 * sizeof(float)))) return r;
    if ((r = ensure_qbuf(c, &c->d_qout, &c->qout_cap, n * 4 * sizeof(float)))) return r;
    float* d_p = (float*)c->d_qin;
    float* d_n = d_p + 3 * n;
    HIPCHK(c, hipMemcpyAsync(d_p, points, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_n, normals, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((r = rmr_probe_irradiance_device(c, d_p, d_n, n, (float*)c->d_qout))) return r;
    HIPCHK(c, hipMemcpyAsync(out_rgba, c->d_qout, n * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

// ---- the probes' visibility (rmr_probe_vis.hip, rmr_probe_vis_rule.h) ---------------------
namespace {
const char* const kNoProbeVis = "no probe visibility (call rmr_bake_probe_field_visibility / rmr_write_probe_field_visibility)";
const char* const kNoProbeField = "no probe field (call rmr_bake_probe_field / rmr_write_probe_field)";

// The maps of a device list (d_points) or of the context's field (desc, with its validity valid_sh), queued: the
// tile-samples in runs under the plane budget at 16 bytes per unit, each run a cast and a fold; the records
// live in the sample planes' buffer.
int probe_vis_device(rmr_ctx* c, const char* who, const float* d_points, const rmr_volume_desc* desc, const float* valid_sh,
                     size_t n, const float* times, uint32_t nspp, const rmr_probe_params& q, float range, float* d_out) {
    int r;
    if ((r = launch_precheck(c))) return r;
    if (!rmr::vis_range_ok(range)) return fail(c, RMR_E_INVALID, std::string(who) + ": range must be finite and > 0");
    if (!rmr::extent_ok(q.origin_extent))
        return fail(c, RMR_E_INVALID, std::string(who) + ": origin_extent must be finite and >= 0");
    if (n == 0) return RMR_OK;
    KParams P;
    if ((r = query_begin(c, P))) return r;
    if ((r = ensure_qbuf(c, &c->d_probe_vis_state, &c->probe_vis_state_cap, n * rmr::kVisStateFloats * sizeof(float)))) return r;
    rmr::ProbeList B = probe_list(d_points, desc, n, nspp, q, q.origin_extent);
    if ((r = stage_times(c, times, nspp, &B.times))) return r;
    const size_t n_ts = ((n + 63) / 64) * (size_t)nspp;
    // (fewer than 2^31 units per launch: the kernels index a launch's units with 32 bits)
    const size_t chunk = rmr::plan_samples(64, (uint32_t)n_ts, c->samp_budget, 0, sizeof(float4)).per_launch;
    for (size_t k0 = 0; k0 < n_ts; k0 += chunk) {
        const uint32_t cnt = (uint32_t)std::min(chunk, n_ts - k0);
        if ((r = ensure_samp(c, (size_t)cnt * 64))) return r;
        c->last_samp = c->d_samp;
        HIPCHK(c, rmr::launch_probe_vis_cast(P, c->accel.map_np, B, valid_sh, range, k0, cnt, c->d_samp,
                                             c->d_query + kQueryRejects, c->stream));
        HIPCHK(c, rmr::launch_probe_vis_fold(c->d_samp, (float*)c->d_probe_vis_state, n, nspp, range, k0, cnt, d_out, c->stream));
    }
    return RMR_OK;
}
}  // namespace

int rmr_bake_probe_visibility_device(rmr_ctx* c, const float* d_points, size_t n, const float* times, uint32_t nspp,
                                     const rmr_probe_params* params, float range, float* d_out_vis) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_probe_params q;
    int r;
    if ((r = probe_args(c, "rmr_bake_probe_visibility_device", n, times, nspp, params, q))) return r;
    if (n && (!d_points || !d_out_vis)) return fail(c, RMR_E_INVALID, "rmr_bake_probe_visibility_device: null buffer");
    return probe_vis_device(c, "rmr_bake_probe_visibility_device", d_points, nullptr, nullptr, n, times, nspp, q, range, d_out_vis);
}

int rmr_bake_probe_visibility(rmr_ctx* c, const float* points, size_t n, const float* times, uint32_t nspp,
                              const rmr_probe_params* params, float range, float* out_vis) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_probe_params q;
    int r;
    if ((r = probe_args(c, "rmr_bake_probe_visibility", n, times, nspp, params, q))) return r;
    if (n && (!points || !out_vis)) return fail(c, RMR_E_INVALID, "rmr_bake_probe_visibility: null buffer");
    // the probes' bound, over the finite ones
    float ext = 0.0f;
    for (size_t i = 0; i < 3 * n; i++)
        if (std::isfinite(points[i])) ext = std::max(ext, std::fabs(points[i]));
    q.origin_extent = ext;
    if ((r = launch_precheck(c))) return r;
    if (n == 0) return probe_vis_device(c, "rmr_bake_probe_visibility", nullptr, nullptr, nullptr, 0, times, nspp, q, range, nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    if ((r = ensure_qbuf(c, &c->d_qin, &c->qin_cap, n * 3 * sizeof(float)))) return r;
    if ((r = ensure_qbuf(c, &c->d_qout, &c->qout_cap, n * rmr::kVisFloats * sizeof(float)))) return r;
    HIPCHK(c, hipMemcpyAsync(c->d_qin, points, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((r = probe_vis_device(c, "rmr_bake_probe_visibility", (const float*)c->d_qin, nullptr, nullptr, n, times, nspp, q, range,
                              (float*)c->d_qout)))
        return r;
    HIPCHK(c, hipMemcpyAsync(out_vis, c->d_qout, n * rmr::kVisFloats * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

namespace {
// The field's maps, allocated at first use (the field's size is fixed while it lives).
int probe_vis_alloc(rmr_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->d_probe_vis) return RMR_OK;
    return alloc_all(c, {{&c->d_probe_vis, volume_points(&c->probe_desc) * rmr::kVisFloats * sizeof(float)}},
                     "cannot allocate the probe field's visibility");
}
}  // namespace

int rmr_bake_probe_field_visibility(rmr_ctx* c, const float* times, uint32_t nspp, float range) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!c->probe_valid) return fail(c, RMR_E_STATE, kNoProbeField);
    rmr_probe_params q;
    int r;
    const size_t n = volume_points(&c->probe_desc);
    if ((r = probe_args(c, "rmr_bake_probe_field_visibility", n, times, nspp, nullptr, q))) return r;
    q.origin_extent = lattice_extent(c->probe_desc);
    if ((r = launch_precheck(c))) return r;
    if (!rmr::vis_range_ok(range)) return fail(c, RMR_E_INVALID, "rmr_bake_probe_field_visibility: range must be finite and > 0");
    c->probe_vis_valid = false;
    if ((r = probe_vis_alloc(c))) return r;
    if ((r = probe_vis_device(c, "rmr_bake_probe_field_visibility", nullptr, &c->probe_desc, c->d_probe_field, n, times, nspp, q,
                              range, c->d_probe_vis)))
        return r;
    c->probe_vis_range = range;
    c->probe_vis_valid = true;
    return RMR_OK;
}

int rmr_write_probe_field_visibility(rmr_ctx* c, const float* vis, float range) {
    if (!c || !vis) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!c->probe_valid) return fail(c, RMR_E_STATE, kNoProbeField);
    if (!rmr::vis_range_ok(range)) return fail(c, RMR_E_INVALID, "rmr_write_probe_field_visibility: range must be finite and > 0");
    c->probe_vis_valid = false;
    int r;
    if ((r = probe_vis_alloc(c))) return r;
    HIPCHK(c, hipMemcpyAsync(c->d_probe_vis, vis, volume_points(&c->probe_desc) * rmr::kVisFloats * sizeof(float),
                             hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->probe_vis_range = range;
    c->probe_vis_valid = true;
    return RMR_OK;
}

int rmr_read_probe_field_visibility(rmr_ctx* c, float* vis, float* range_out) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!c->probe_valid) return fail(c, RMR_E_STATE, kNoProbeField);
    if (!c->probe_vis_valid) return fail(c, RMR_E_STATE, kNoProbeVis);
    HIPCHK(c, hipSetDevice(c->device));
    if (range_out) *range_out = c->probe_vis_range;
    if (vis)
        HIPCHK(c, hipMemcpyAsync(vis, c->d_probe_vis, volume_points(&c->probe_desc) * rmr::kVisFloats * sizeof(float),
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

void* rmr_probe_field_visibility_device_ptr(rmr_ctx* c) {
    return c && c->probe_valid && c->probe_vis_valid ? c->d_probe_vis : nullptr;
}

int rmr_probe_irradiance_vis_device(rmr_ctx* c, const float* d_points, const float* d_normals, size_t n, float bias,
                                    float* d_out_rgba) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (n && (!d_points || !d_normals || !d_out_rgba)) return fail(c, RMR_E_INVALID, "rmr_probe_irradiance_vis_device: null buffer");
    if (!rmr::vis_bias_ok(bias)) return fail(c, RMR_E_INVALID, "rmr_probe_irradiance_vis: bias must be finite and >= 0");
    if (!c->probe_valid) return fail(c, RMR_E_STATE, kNoProbeField);
    if (!c->probe_vis_valid) return fail(c, RMR_E_STATE, kNoProbeVis);
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if ((r = ensure_query(c))) return r;
    HIPCHK(c, rmr::launch_probe_lookup_vis(c->probe_desc, c->d_probe_field, c->d_probe_vis, d_points, d_normals, (uint64_t)n, bias,
                                           d_out_rgba, c->d_query + kQueryRejects, c->stream));
    return RMR_OK;
}

int rmr_probe_irradiance_vis(rmr_ctx* c, const float* points, const float* normals, size_t n, float bias, float* out_rgba) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (n && (!points || !normals || !out_rgba)) return fail(c, RMR_E_INVALID, "rmr_probe_irradiance_vis: null buffer");
    if (!rmr::vis_bias_ok(bias)) return fail(c, RMR_E_INVALID, "rmr_probe_irradiance_vis: bias must be finite and >= 0");
    if (!c->probe_valid) return fail(c, RMR_E_STATE, kNoProbeField);
    if (!c->probe_vis_valid) return fail(c, RMR_E_STATE, kNoProbeVis);
    if (n == 0) return RMR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if ((r = ensure_qbuf(c, &c->d_qin, &c->qin_cap, n * 6 * sizeof(float)))) return r;
    if ((r = ensure_qbuf(c, &c->d_qout, &c->qout_cap, n * 4 * sizeof(float)))) return r;
    float* d_p = (float*)c->d_qin;
    float* d_n = d_p + 3 * n;
    HIPCHK(c, hipMemcpyAsync(d_p, points, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_n, normals, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((r = rmr_probe_irradiance_vis_device(c, d_p, d_n, n, bias, (float*)c->d_qout))) return r;
    HIPCHK(c, hipMemcpyAsync(out_rgba, c->d_qout, n * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RMR_OK;
}

// ---- first-hit guides and the preview denoiser (rmr_guides.hip, rmr_denoise.hip) ------------------
namespace {
// The five W x H float4 buffers, at first use. The guide planes start as zeros (a read before a
// full-image pass shows zeros outside the rects rendered so far).
int ensure_guides(rmr_ctx* c) {
    if (c->d_guide[0]) return RMR_OK;
    const size_t bytes = (size_t)c->W * c->H * sizeof(float4);
    if (const int r = alloc_all(c, {{&c->d_guide[0], bytes}, {&c->d_guide[1], bytes}, {&c->d_guide[2], bytes},
                                    {&c->d_dn[0], bytes}, {&c->d_dn[1], bytes}},
                                "cannot allocate the guide planes and filter images (5 x W x H x 16 bytes)"))
        return r;
    c->st.guides_allocated();
    for (int i = 0; i < 3; i++) HIPCHK(c, hipMemsetAsync(c->d_guide[i], 0, bytes, c->stream));
    return RMR_OK;
}

// The guide pass over a rect already clamped to the image and non-empty.
int render_guides(rmr_ctx* c, int x0, int y0, int x1, int y1) {
    int r;
    if (!c->scene_loaded) return fail(c, RMR_E_STATE, "no scene loaded (call rmr_load_scene_json / rmr_load_builtin_scene)");
    if (c->camera.model == RMR_CAMERA_EQUIRECT || c->camera.model == RMR_CAMERA_ORTHO)
        return fail(c, RMR_E_STATE, "no first-hit guides for the equirect and ortho camera models");
    HIPCHK(c, hipSetDevice(c->device));
    if ((r = ensure_guides(c))) return r;
    if (!c->view_set) default_view(c);
    KParams P;
    if ((r = view_params(c, P))) return r;
    P.x0 = x0; P.y0 = y0; P.x1 = x1; P.y1 = y1;
    HIPCHK(c, rmr::launch_guides(P, c->accel.map_np, c->d_guide[RMR_GUIDE_RAY], c->d_guide[RMR_GUIDE_HIT],
                                 c->d_guide[RMR_GUIDE_NORMAL], c->stream));
    if (x0 == 0 && y0 == 0 && x1 == c->W && y1 == c->H) c->st.guides_rendered();
    return RMR_OK;
}

bool denoise_params_ok(const rmr_denoise_params& p) {
    return p.iterations >= 0 && p.iterations <= 8 && p.normal_pow2 >= 0 && p.normal_pow2 <= 7 &&
           std::isfinite(p.sigma_z) && p.sigma_z > 0.0f && std::isfinite(p.sigma_c) && p.sigma_c >= 0.0f;
}
}  // namespace

void rmr_default_denoise_params(rmr_denoise_params* p) {
    if (!p) return;
    p->iterations = 5;
    p->normal_pow2 = 5;
    p->sigma_z = 0.02f;
    p->sigma_c = 0.0f;
}

int rmr_render_guides(rmr_ctx* c, int x0, int y0, int x1, int y1) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!c->scene_loaded) return fail(c, RMR_E_STATE, "no scene loaded (call rmr_load_scene_json / rmr_load_builtin_scene)");
    if (!rmr::clamp_rect(c->W, c->H, x0, y0, x1, y1)) return RMR_OK;
    return render_guides(c, x0, y0, x1, y1);
}

int rmr_read_guide(rmr_ctx* c, int plane, float* rgba, size_t bytes) {
    if (!c || !rgba) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (plane < RMR_GUIDE_RAY || plane > RMR_GUIDE_NORMAL) return fail(c, RMR_E_INVALID, "bad guide plane");
    const size_t need = (size_t)c->W * c->H * sizeof(float4);
    if (bytes < need) return fail(c, RMR_E_INVALID, "buffer too small");
    if (!c->d_guide[plane]) return fail(c, RMR_E_STATE, "no guides rendered (call rmr_render_guides)");
    return read_back(c, rgba, c->d_guide[plane], need);
}

void* rmr_guide_device_ptr(rmr_ctx* c, int plane) {
    if (!c || plane < RMR_GUIDE_RAY || plane > RMR_GUIDE_NORMAL) return nullptr;
    if (!flushed(c)) return nullptr;
    if (hipSetDevice(c->device) != hipSuccess || ensure_guides(c) != RMR_OK) return nullptr;
    return (void*)c->d_guide[plane];
}

int rmr_denoise(rmr_ctx* c, const rmr_denoise_params* p) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_denoise_params q;
    rmr_default_denoise_params(&q);
    if (p) q = *p;
    if (!denoise_params_ok(q))
        return fail(c, RMR_E_INVALID, "bad denoise params (iterations 0..8, normal_pow2 0..7, sigma_z finite > 0, sigma_c finite >= 0)");
    int r;
    c->st.denoise_begin();
    if (!c->st.guides_valid && (r = render_guides(c, 0, 0, c->W, c->H))) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->W * c->H * sizeof(float4);
    if (q.iterations == 0) {
        HIPCHK(c, hipMemcpyAsync(c->d_dn[0], c->d_accum, bytes, hipMemcpyDeviceToDevice, c->stream));
        c->st.denoise_queued(0);
        return RMR_OK;
    }
    rmr::DenoisePass A{};
    A.hit = c->d_guide[RMR_GUIDE_HIT];
    A.nrm = c->d_guide[RMR_GUIDE_NORMAL];
    A.W = c->W;
    A.H = c->H;
    A.normal_pow2 = q.normal_pow2;
    for (int i = 0; i < q.iterations; i++) {
        A.in = i == 0 ? c->d_accum : c->d_dn[(i - 1) & 1];
        A.out = c->d_dn[i & 1];
        A.step = 1 << i;
        A.sigma_z_step = q.sigma_z * (float)A.step;
        const double sc = (double)q.sigma_c / (double)A.step;   // sigma_c 2^-i
        // (kept finite: a zero colour distance then weighs exp(-0) = 1 whatever sigma_c is)
        A.inv_sigma_c2 = q.sigma_c > 0.0f ? (float)std::min(1.0 / (sc * sc), (double)FLT_MAX) : 0.0f;
        HIPCHK(c, rmr::launch_atrous(A, i < 2 && ((c->dn_tiled_steps >> i) & 1), c->stream));
    }
    c->st.denoise_queued((q.iterations - 1) & 1);
    return RMR_OK;
}

int rmr_read_denoised(rmr_ctx* c, float* rgba, size_t bytes) {
    if (!c || !rgba) return RMR_E_INVALID;
    RMR_FLUSH(c);
    const size_t need = (size_t)c->W * c->H * sizeof(float4);
    if (bytes < need) return fail(c, RMR_E_INVALID, "buffer too small");
    const int i = c->st.readable(RMR_OUTPUT_DENOISED);
    if (i < 0) return no_valid(c, RMR_OUTPUT_DENOISED);
    return read_back(c, rgba, c->d_dn[i], need);
}

void* rmr_denoised_device_ptr(rmr_ctx* c) {
    if (!c) return nullptr;
    if (!flushed(c)) return nullptr;
    const int i = c->st.readable(RMR_OUTPUT_DENOISED);
    return i < 0 ? nullptr : (void*)c->d_dn[i];
}

int rmr_set_output_source(rmr_ctx* c, int source) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    const int i = c->st.readable(source);
    if (i == rmr::StageState::kNoSource) return fail(c, RMR_E_INVALID, "bad output source");
    // (refused, the source unchanged, while there is no temporal, tonemapped or bloom image to read; the denoised
    // image may be selected ahead of the rmr_denoise that makes it)
    if (i < 0 && source != RMR_OUTPUT_DENOISED) return no_valid(c, source);
    c->output_source = source;
    return RMR_OK;
}

// ---- per-tile error estimate and adaptive sampling (rmr_estimate.hip, adaptive.cpp) ----------------
namespace {
bool offset_ok(float offset) { return std::isfinite(offset) && offset > 0.0f; }

// The tile errors of the context's accumulator and half image, to `out` (TX x TY floats); synchronises.
int tile_error_host(rmr_ctx* c, float offset, float* out) {
    const size_t tiles = (size_t)((c->W + 7) / 8) * ((c->H + 7) / 8);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, rmr::launch_tile_error(c->d_accum, c->d_half, c->W, c->H, offset, c->d_tile_err, c->stream));
    return read_back(c, out, c->d_tile_err, tiles * sizeof(float));
}
}  // namespace

int rmr_set_error_estimate(rmr_ctx* c, int on) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!on) {   // (the buffers stay until rmr_reload resizes them or rmr_destroy: queued folds may still write them)
        c->est_on = false;
        c->est_valid = false;
        return RMR_OK;
    }
    return enable_estimate(c);
}

int rmr_read_half_accum(rmr_ctx* c, float* rgba, size_t bytes) {
    if (!c || !rgba) return RMR_E_INVALID;
    RMR_FLUSH(c);
    const size_t need = (size_t)c->W * c->H * sizeof(float4);
    if (bytes < need) return fail(c, RMR_E_INVALID, "buffer too small");
    if (!c->est_on || !c->d_half) return fail(c, RMR_E_STATE, "the error estimate is off (call rmr_set_error_estimate)");
    return read_back(c, rgba, c->d_half, need);
}

void* rmr_half_device_ptr(rmr_ctx* c) {
    if (!c) return nullptr;
    if (!flushed(c)) return nullptr;
    return c->est_on ? (void*)c->d_half : nullptr;
}

int rmr_tile_error(rmr_ctx* c, float offset, float* out, size_t bytes) {
    if (!c || !out) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!c->est_on || !c->est_valid)
        return fail(c, RMR_E_STATE, "the error estimate is not valid (enable it before the first render after rmr_reload)");
    if (!offset_ok(offset)) return fail(c, RMR_E_INVALID, "offset must be finite and > 0");
    const size_t tiles = (size_t)((c->W + 7) / 8) * ((c->H + 7) / 8);
    if (bytes < tiles * sizeof(float)) return fail(c, RMR_E_INVALID, "buffer too small");
    return tile_error_host(c, offset, out);
}

int rmr_tile_error_images(rmr_ctx* c, const float* a_rgba, const float* b_rgba, int w, int h, float offset, float* out) {
    if (!c || !a_rgba || !b_rgba || !out) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (w <= 0 || h <= 0 || w > 32768 || h > 32768) return fail(c, RMR_E_INVALID, "bad image size");
    if (!offset_ok(offset)) return fail(c, RMR_E_INVALID, "offset must be finite and > 0");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)w * h * sizeof(float4);
    const size_t tiles = (size_t)((w + 7) / 8) * ((h + 7) / 8);
    hipError_t e;
    {
        Scratch S(c->stream);
        float4 *dA = S.get<float4>(bytes), *dB = S.get<float4>(bytes);
        float* dE = S.get<float>(tiles * sizeof(float));
        S.up(dA, a_rgba, bytes);
        S.up(dB, b_rgba, bytes);
        S.run([&] { return rmr::launch_tile_error(dA, dB, w, h, offset, dE, c->stream); });
        S.down(out, dE, tiles * sizeof(float));
        e = S.done();
    }
    HIPCHK(c, e);
    return RMR_OK;
}

int rmr_render_adaptive(rmr_ctx* c, const float* times, const rmr_adaptive_params* p, rmr_adaptive_result* result) {
    if (!c || !times || !p || !result) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!rmr::adaptive_params_ok(*p))
        return fail(c, RMR_E_INVALID, "bad adaptive params (threshold finite >= 0, offset finite > 0, min_samples >= 2, "
                                      "pass_samples >= 1, max_samples >= min_samples, block_tiles 1..8)");
    int r;
    if ((r = launch_precheck(c))) return r;
    if (c->rendered)
        return fail(c, RMR_E_STATE, "rmr_render_adaptive needs an accumulator nothing has been rendered into since rmr_reload");
    c->est_valid = false;   // (zeroes the half image again: e.g. enabled, then a bound accumulator)
    if ((r = enable_estimate(c))) return r;
    const int W = c->W, H = c->H, TX = (W + 7) / 8, TY = (H + 7) / 8, bt = p->block_tiles;
    const size_t tiles = (size_t)TX * TY;
    std::vector<uint8_t> open((size_t)rmr::adaptive_blocks(TX, bt) * rmr::adaptive_blocks(TY, bt), 1);
    std::vector<float> err(tiles);
    std::vector<uint32_t> counts(tiles, p->min_samples);
    // 1. samples [0, min_samples) everywhere
    if ((r = render_tiles(c, rect_tiles(0, 0, W, H), 0, 0, W, H, times, 0, p->min_samples))) return r;
    uint32_t done = p->min_samples, passes = 1;
    for (;;) {
        // 2. decide  3. stop test
        if ((r = tile_error_host(c, p->offset, err.data()))) return r;
        const int n_open = rmr::adaptive_select(err.data(), TX, TY, bt, p->threshold, open.data());
        if (n_open == 0 || done == p->max_samples) break;
        // 4. the next pass on the open blocks' tiles
        const uint32_t n = std::min(p->pass_samples, p->max_samples - done);
        const std::vector<int32_t> xy = rmr::adaptive_tiles(open.data(), TX, TY, bt);
        std::vector<TileXY> t(xy.size() / 2);
        for (size_t i = 0; i < t.size(); i++) {
            t[i] = TileXY{xy[2 * i], xy[2 * i + 1]};
            counts[(size_t)(xy[2 * i + 1] / 8) * TX + xy[2 * i] / 8] += n;
        }
        if ((r = render_tiles(c, t, 0, 0, W, H, times + done, done, n))) return r;
        done += n;
        passes++;
    }
    rmr_adaptive_result res{};
    res.passes = passes;
    res.max_error = 0.0f;
    for (int ty = 0; ty < TY; ty++)
        for (int tx = 0; tx < TX; tx++) {
            const size_t i = (size_t)ty * TX + tx;
            res.samples += (uint64_t)counts[i] * (uint64_t)(std::min(8, W - 8 * tx) * std::min(8, H - 8 * ty));
            if (err[i] > p->threshold) res.tiles_open++;
            if (err[i] > res.max_error) res.max_error = err[i];
        }
    c->sample_counts = counts;
    *result = res;
    return RMR_OK;
}

int rmr_read_sample_counts(rmr_ctx* c, uint32_t* out, size_t bytes) {
    if (!c || !out) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (c->sample_counts.empty()) return fail(c, RMR_E_STATE, "no rmr_render_adaptive since the last rmr_reload");
    if (bytes < c->sample_counts.size() * sizeof(uint32_t)) return fail(c, RMR_E_INVALID, "buffer too small");
    std::memcpy(out, c->sample_counts.data(), c->sample_counts.size() * sizeof(uint32_t));
    return RMR_OK;
}

// ---- variance-guided mode of the preview denoiser (rmr_denoise_var.hip) ----------------------------
namespace {
bool variance_params_ok(const rmr_variance_params& v) {
    return std::isfinite(v.sigma_l) && v.sigma_l > 0.0f && v.var_radius >= 0 && v.var_radius <= 4;
}

// The seed and the guided passes over w x h images, queued on s: a / b / hit / nrm are read, dn[2] and
// var[3] (var[0] the seed) written. *img and *vres receive the indices of the result in dn[] and var[].
hipError_t run_guided(const float4* a, const float4* b, const float4* hit, const float4* nrm, int w, int h,
                      const rmr_denoise_params& q, const rmr_variance_params& v, float4* const dn[2],
                      float* const var[3], int tiled_mask, hipStream_t s, int* img, int* vres) {
    rmr::VarianceSeed V{a, b, nrm, var[0], w, h, v.var_radius};
    hipError_t e = rmr::launch_variance_seed(V, s);
    if (e != hipSuccess) return e;
    *img = 0;
    *vres = 0;
    if (q.iterations == 0)
        return hipMemcpyAsync(dn[0], a, (size_t)w * h * sizeof(float4), hipMemcpyDeviceToDevice, s);
    rmr::DenoiseVarPass P{};
    P.d.hit = hit;
    P.d.nrm = nrm;
    P.d.W = w;
    P.d.H = h;
    P.d.normal_pow2 = q.normal_pow2;
    P.sigma_l = v.sigma_l;
    for (int i = 0; i < q.iterations; i++) {
        P.d.in = i == 0 ? a : dn[(i - 1) & 1];
        P.d.out = dn[i & 1];
        P.var_in = i == 0 ? var[0] : var[1 + ((i - 1) & 1)];
        P.var_out = var[1 + (i & 1)];
        P.d.step = 1 << i;
        P.d.sigma_z_step = q.sigma_z * (float)P.d.step;
        const double sc = (double)q.sigma_c / (double)P.d.step;   // sigma_c 2^-i, as rmr_denoise
        P.d.inv_sigma_c2 = q.sigma_c > 0.0f ? (float)std::min(1.0 / (sc * sc), (double)FLT_MAX) : 0.0f;
        if ((e = rmr::launch_atrous_var(P, i < 2 && ((tiled_mask >> i) & 1), s)) != hipSuccess) return e;
    }
    *img = (q.iterations - 1) & 1;
    *vres = 1 + ((q.iterations - 1) & 1);
    return hipSuccess;
}

int guided_params(rmr_ctx* c, const rmr_denoise_params* p, const rmr_variance_params* v, rmr_denoise_params& q,
                  rmr_variance_params& u) {
    rmr_default_denoise_params(&q);
    rmr_default_variance_params(&u);
    if (p) q = *p;
    if (v) u = *v;
    if (!denoise_params_ok(q))
        return fail(c, RMR_E_INVALID, "bad denoise params (iterations 0..8, normal_pow2 0..7, sigma_z finite > 0, sigma_c finite >= 0)");
    if (!variance_params_ok(u)) return fail(c, RMR_E_INVALID, "bad variance params (sigma_l finite > 0, var_radius 0..4)");
    return RMR_OK;
}
}  // namespace

void rmr_default_variance_params(rmr_variance_params* p) {
    if (!p) return;
    p->sigma_l = 4.0f;
    p->var_radius = 3;
}

int rmr_check_variance_params(const rmr_variance_params* p) {
    return p && variance_params_ok(*p) ? RMR_OK : RMR_E_INVALID;
}

int rmr_denoise_variance(rmr_ctx* c, const rmr_denoise_params* p, const rmr_variance_params* v) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_denoise_params q;
    rmr_variance_params u;
    int r;
    if ((r = guided_params(c, p, v, q, u))) return r;
    if (!c->est_on || !c->est_valid || !c->d_half)
        return fail(c, RMR_E_STATE, "the error estimate is not valid: call rmr_set_error_estimate before the first "
                                    "render since rmr_reload, or render with rmr_render_adaptive");
    c->st.denoise_begin();
    if (!c->st.guides_valid && (r = render_guides(c, 0, 0, c->W, c->H))) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t vbytes = (size_t)c->W * c->H * sizeof(float);
    if (!c->d_var[0] && (r = alloc_all(c, {{&c->d_var[0], vbytes}, {&c->d_var[1], vbytes}, {&c->d_var[2], vbytes}},
                                       "cannot allocate the variance planes (3 x W x H x 4 bytes)")))
        return r;
    int img = 0, vres = 0;
    HIPCHK(c, run_guided(c->d_accum, c->d_half, c->d_guide[RMR_GUIDE_HIT], c->d_guide[RMR_GUIDE_NORMAL], c->W, c->H, q, u,
                         c->d_dn, c->d_var, c->dnv_tiled_steps, c->stream, &img, &vres));
    c->st.denoise_guided_queued(img, vres);
    return RMR_OK;
}

int rmr_read_variance(rmr_ctx* c, int which, float* out, size_t bytes) {
    if (!c || !out) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (which != RMR_VARIANCE_SEED && which != RMR_VARIANCE_FILTERED) return fail(c, RMR_E_INVALID, "bad variance plane");
    const size_t need = (size_t)c->W * c->H * sizeof(float);
    if (bytes < need) return fail(c, RMR_E_INVALID, "buffer too small");
    const int i = c->st.variance_plane(which);
    if (i < 0) return fail(c, RMR_E_STATE, "no valid variance planes (call rmr_denoise_variance)");
    return read_back(c, out, c->d_var[i], need);
}

void* rmr_variance_device_ptr(rmr_ctx* c, int which) {
    if (!c || (which != RMR_VARIANCE_SEED && which != RMR_VARIANCE_FILTERED)) return nullptr;
    if (!flushed(c)) return nullptr;
    const int i = c->st.variance_plane(which);
    return i < 0 ? nullptr : (void*)c->d_var[i];
}

int rmr_denoise_variance_images(rmr_ctx* c, const float* a_rgba, const float* b_rgba, const float* hit_rgba,
                                const float* nrm_rgba, int w, int h, const rmr_denoise_params* p,
                                const rmr_variance_params* v, float* out_rgba, float* out_seed, float* out_var) {
    if (!c || !a_rgba || !b_rgba || !hit_rgba || !nrm_rgba || !out_rgba) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (w <= 0 || h <= 0 || w > 32768 || h > 32768) return fail(c, RMR_E_INVALID, "bad image size");
    rmr_denoise_params q;
    rmr_variance_params u;
    int r;
    if ((r = guided_params(c, p, v, q, u))) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)w * h * sizeof(float4), vbytes = (size_t)w * h * sizeof(float);
    const float* src[4] = {a_rgba, b_rgba, hit_rgba, nrm_rgba};
    hipError_t e;
    {
        Scratch S(c->stream);
        float4* img[6];   // A, B, HIT, NORMAL, two filter images
        float* var[3];
        for (float4*& b : img) b = S.get<float4>(bytes);
        for (float*& b : var) b = S.get<float>(vbytes);
        for (int i = 0; i < 4; i++) S.up(img[i], src[i], bytes);
        int ri = 0, rv = 0;
        S.run([&] { return run_guided(img[0], img[1], img[2], img[3], w, h, q, u, img + 4, var, c->dnv_tiled_steps, c->stream, &ri, &rv); });
        S.down(out_rgba, img[4 + ri], bytes);
        if (out_seed) S.down(out_seed, var[0], vbytes);
        if (out_var) S.down(out_var, var[rv], vbytes);
        e = S.done();
    }
    HIPCHK(c, e);
    return RMR_OK;
}

// ---- temporal reprojection of the preview (rmr_temporal.hip, temporal.cpp) -------------------------
namespace {
// The pass over w x h images on s. h_view: the history's view; false when temporal_view_inverse refuses it.
bool temporal_pass(rmr::TemporalPass& T, const float h_view[15], int w, int h, float samples, const rmr_temporal_params& q) {
    double inv[12];
    if (!rmr::temporal_view_inverse(h_view, inv)) return false;
    T.d.W = w;
    T.d.H = h;
    T.d.step = 1;
    T.d.normal_pow2 = q.normal_pow2;
    T.d.sigma_z_step = q.sigma_z;
    T.d.inv_sigma_c2 = 0.0f;
    for (int i = 0; i < 3; i++) T.eye[i] = h_view[i];
    for (int i = 0; i < 9; i++) T.minv[i] = (float)inv[i];
    for (int i = 0; i < 3; i++) T.twist[i] = (float)inv[9 + i];
    T.Wf = (float)w;
    T.Hf = (float)h;
    T.n_cur = samples;
    T.max_history = q.max_history;
    return true;
}

int temporal_params(rmr_ctx* c, const rmr_temporal_params* p, float samples, rmr_temporal_params& q) {
    rmr_default_temporal_params(&q);
    if (p) q = *p;
    if (!rmr::temporal_params_ok(q))
        return fail(c, RMR_E_INVALID, "bad temporal params (max_history finite >= 1, sigma_z finite > 0, normal_pow2 0..7)");
    if (!std::isfinite(samples) || !(samples > 0.0f)) return fail(c, RMR_E_INVALID, "samples must be finite and > 0");
    return RMR_OK;
}
}  // namespace

int rmr_temporal_accumulate(rmr_ctx* c, int source, float samples, const rmr_temporal_params* p) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_temporal_params q;
    int r;
    if ((r = temporal_params(c, p, samples, q))) return r;
    if (source != RMR_OUTPUT_ACCUM && source != RMR_OUTPUT_DENOISED)
        return fail(c, RMR_E_INVALID, "bad source (RMR_OUTPUT_ACCUM or RMR_OUTPUT_DENOISED)");
    if (!c->scene_loaded) return fail(c, RMR_E_STATE, "no scene loaded (call rmr_load_scene_json / rmr_load_builtin_scene)");
    if (c->camera.model == RMR_CAMERA_EQUIRECT || c->camera.model == RMR_CAMERA_ORTHO)
        return fail(c, RMR_E_STATE, "no first-hit guides for the equirect and ortho camera models");
    const int src_i = c->st.readable(source);
    if (src_i < 0) return no_valid(c, source);
    if (!c->st.guides_valid && (r = render_guides(c, 0, 0, c->W, c->H))) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)c->W * c->H, bytes = px * sizeof(float4);
    if (!c->d_tcol[0]) {
        if ((r = alloc_all(c, {{&c->d_tcol[0], bytes}, {&c->d_tcol[1], bytes}, {&c->d_tn[0], px * sizeof(float)},
                               {&c->d_tn[1], px * sizeof(float)}, {&c->d_tguide[0], bytes}, {&c->d_tguide[1], bytes}},
                           "cannot allocate the temporal planes (72 bytes per pixel)")))
            return r;
        c->st.temporal_reset();
    }
    rmr::TemporalPass T{};
    const bool have = c->st.t_cur >= 0 && temporal_pass(T, c->t_view, c->W, c->H, samples, q);
    const int from = have ? c->st.t_cur : 0, to = 1 - from;
    // no temporal image until everything below is queued, nor the images made from the old one
    c->st.temporal_begin();
    if (!have) {
        // no history: the same kernel against counts of 0 (every other history plane zeroed, so that what
        // the skipped taps never read is defined), projected with the current view or, if that is
        // degenerate too, with the identity
        static const float kIdent[15] = {0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1, 1};
        if (!c->view_set) default_view(c);
        if (!temporal_pass(T, c->view, c->W, c->H, samples, q)) (void)temporal_pass(T, kIdent, c->W, c->H, samples, q);
        HIPCHK(c, hipMemsetAsync(c->d_tcol[0], 0, bytes, c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_tn[0], 0, px * sizeof(float), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_tguide[0], 0, bytes, c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_tguide[1], 0, bytes, c->stream));
    }
    T.d.in = source_image(c, source, src_i);
    T.d.hit = c->d_guide[RMR_GUIDE_HIT];
    T.d.nrm = c->d_guide[RMR_GUIDE_NORMAL];
    T.d.out = c->d_tcol[to];
    T.n_out = c->d_tn[to];
    T.h_col = c->d_tcol[from];
    T.h_n = c->d_tn[from];
    T.h_hit = c->d_tguide[0];
    T.h_nrm = c->d_tguide[1];
    T.xy_out = nullptr;
    HIPCHK(c, rmr::launch_temporal(T, c->stream));
    if (c->t_keep) {   // (timing the kernel alone against one history)
        c->st.temporal_queued(from);
        return RMR_OK;
    }
    // the current guides and view become the history's
    HIPCHK(c, hipMemcpyAsync(c->d_tguide[0], c->d_guide[RMR_GUIDE_HIT], bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_tguide[1], c->d_guide[RMR_GUIDE_NORMAL], bytes, hipMemcpyDeviceToDevice, c->stream));
    std::memcpy(c->t_view, c->view, sizeof c->t_view);
    c->st.temporal_queued(to);
    return RMR_OK;
}

int rmr_temporal_reset(rmr_ctx* c) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    c->st.temporal_reset();
    return RMR_OK;
}

int rmr_read_temporal(rmr_ctx* c, float* rgba, size_t bytes) {
    if (!c || !rgba) return RMR_E_INVALID;
    RMR_FLUSH(c);
    const size_t need = (size_t)c->W * c->H * sizeof(float4);
    if (bytes < need) return fail(c, RMR_E_INVALID, "buffer too small");
    const int i = c->st.readable(RMR_OUTPUT_TEMPORAL);
    if (i < 0) return no_valid(c, RMR_OUTPUT_TEMPORAL);
    return read_back(c, rgba, c->d_tcol[i], need);
}

int rmr_read_temporal_count(rmr_ctx* c, float* out, size_t bytes) {
    if (!c || !out) return RMR_E_INVALID;
    RMR_FLUSH(c);
    const size_t need = (size_t)c->W * c->H * sizeof(float);
    if (bytes < need) return fail(c, RMR_E_INVALID, "buffer too small");
    const int i = c->st.readable(RMR_OUTPUT_TEMPORAL);
    if (i < 0) return no_valid(c, RMR_OUTPUT_TEMPORAL);
    return read_back(c, out, c->d_tn[i], need);
}

void* rmr_temporal_device_ptr(rmr_ctx* c) {
    if (!c) return nullptr;
    if (!flushed(c)) return nullptr;
    const int i = c->st.readable(RMR_OUTPUT_TEMPORAL);
    return i < 0 ? nullptr : (void*)c->d_tcol[i];
}

int rmr_temporal_images(rmr_ctx* c, const float* s_rgba, const float* hit, const float* nrm, const float view[15],
                        const float* h_rgba, const float* h_n, const float* h_hit, const float* h_nrm,
                        const float h_view[15], int w, int h, float samples, const rmr_temporal_params* p,
                        float* out_rgba, float* out_n, float* out_xy) {
    (void)view;   // (the hit points carry the current view)
    if (!c || !s_rgba || !hit || !nrm || !h_rgba || !h_n || !h_hit || !h_nrm || !h_view || !out_rgba || !out_n)
        return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (w <= 0 || h <= 0 || w > 32768 || h > 32768) return fail(c, RMR_E_INVALID, "bad image size");
    rmr_temporal_params q;
    int r;
    if ((r = temporal_params(c, p, samples, q))) return r;
    rmr::TemporalPass T{};
    if (!temporal_pass(T, h_view, w, h, samples, q))
        return fail(c, RMR_E_INVALID, "degenerate history view (rmr_temporal_view_inverse)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)w * h, bytes = px * sizeof(float4), nbytes = px * sizeof(float);
    // S, HIT, NORMAL, Hc, Hhit, Hnrm, out | Hn, n_out | xy
    const float* src[6] = {s_rgba, hit, nrm, h_rgba, h_hit, h_nrm};
    hipError_t e;
    {
        Scratch S(c->stream);
        float4* img[7];
        float* cnt[2];
        for (float4*& b : img) b = S.get<float4>(bytes);
        for (float*& b : cnt) b = S.get<float>(nbytes);
        float2* xy = out_xy ? S.get<float2>(px * sizeof(float2)) : nullptr;
        for (int i = 0; i < 6; i++) S.up(img[i], src[i], bytes);
        S.up(cnt[0], h_n, nbytes);
        T.d.in = img[0]; T.d.hit = img[1]; T.d.nrm = img[2];
        T.h_col = img[3]; T.h_hit = img[4]; T.h_nrm = img[5];
        T.d.out = img[6];
        T.h_n = cnt[0]; T.n_out = cnt[1];
        T.xy_out = xy;
        S.run([&] { return rmr::launch_temporal(T, c->stream); });
        S.down(out_rgba, img[6], bytes);
        S.down(out_n, cnt[1], nbytes);
        if (out_xy) S.down(out_xy, xy, px * sizeof(float2));
        e = S.done();
    }
    HIPCHK(c, e);
    return RMR_OK;
}

// ---- tone mapping and histogram auto-exposure (rmr_tonemap.hip, tonemap.cpp) -----------------------
static_assert(sizeof(rmr_tonemap_params) == 32, "rmr_tonemap_params is 32 bytes (include/rmr.h)");
namespace {
// The image a stage source names, with the existing readers' messages. The stages take the accumulator, the
// denoised and the temporal image; bloom_too: the bloom image as well.
int tone_source(rmr_ctx* c, int source, const float4** src, bool bloom_too = false) {
    const int i = c->st.readable(source);
    if (i == rmr::StageState::kNoSource || source == RMR_OUTPUT_TONEMAPPED || (source == RMR_OUTPUT_BLOOM && !bloom_too))
        return fail(c, RMR_E_INVALID, bloom_too ? "bad source (RMR_OUTPUT_ACCUM, RMR_OUTPUT_DENOISED, RMR_OUTPUT_TEMPORAL or RMR_OUTPUT_BLOOM)"
                                                : "bad source (RMR_OUTPUT_ACCUM, RMR_OUTPUT_DENOISED or RMR_OUTPUT_TEMPORAL)");
    if (i < 0) return no_valid(c, source);
    *src = source_image(c, source, i);
    return RMR_OK;
}

// The stage's buffers, at first use: all four or none.
int ensure_tonemap(rmr_ctx* c) {
    if (c->d_tm) return RMR_OK;
    if (const int r = alloc_all(c, {{&c->d_tm, (size_t)c->W * c->H * sizeof(float4)},
                                    {&c->d_tm_slab, (size_t)rmr::kToneSlabRows * rmr::kToneWords * sizeof(uint32_t)},
                                    {&c->d_tm_state, sizeof(rmr::ToneState)}, {&c->d_tm_lc, 255 * sizeof(double)}},
                                "cannot allocate the tonemapped plane (16 bytes per pixel) and the histogram slab"))
        return r;
    // the table and the zeroed state go through the context's stream, ahead of the kernels that read them
    // (the host copy of the table lives in the context, so the queued copy's source outlives this call)
    rmr::tonemap_lc_table(c->tm_lc);
    hipError_t e = hipMemcpyAsync(c->d_tm_lc, c->tm_lc, sizeof c->tm_lc, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_tm_state, 0, sizeof(rmr::ToneState), c->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        free_all({&c->d_tm, &c->d_tm_slab, &c->d_tm_state, &c->d_tm_lc});
        HIPCHK(c, e);
    }
    c->st.tonemap_begin();
    c->tm_used = 0;
    return RMR_OK;
}

// k_lum_hist and k_meter over src on the context's stream.
int tone_meter(rmr_ctx* c, const float4* src, const rmr_tonemap_params& q, bool run_meter) {
    const size_t px = (size_t)c->W * c->H;
    const int blocks = rmr::lum_hist_blocks(px);
    HIPCHK(c, rmr::launch_lum_hist(src, px, c->d_tm_slab, blocks, c->tm_fold, c->stream));
    HIPCHK(c, rmr::launch_meter(c->d_tm_slab, blocks, c->d_tm_state, c->d_tm_lc, rmr::tonemap_meter(q), run_meter, c->stream));
    return RMR_OK;
}
}  // namespace

int rmr_tonemap(rmr_ctx* c, int source, const rmr_tonemap_params* p) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_tonemap_params q;
    rmr_default_tonemap_params(&q);
    if (p) q = *p;
    if (!rmr::tonemap_params_ok(q))
        return fail(c, RMR_E_INVALID, "bad tonemap params (curve 0..2, auto_exposure 0 / 1, |exposure_ev| <= 32, key > 0, "
                                      "0 <= low_pct < high_pct <= 1, 0 < adapt <= 1, white > 0)");
    const float4* src = nullptr;
    int r;
    if ((r = tone_source(c, source, &src, true))) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if ((r = ensure_tonemap(c))) return r;
    c->st.tonemap_begin();   // (until everything below is queued)
    const size_t px = (size_t)c->W * c->H;
    const float iw2 = rmr::tonemap_iw2(q);
    if (q.auto_exposure) {
        if ((r = tone_meter(c, src, q, true))) return r;
        HIPCHK(c, rmr::launch_tonemap(src, c->d_tm, px, c->d_tm_state, 0.0f, q.curve, iw2, c->stream));
        c->tm_used = 2;
    } else {
        c->tm_ev = (double)q.exposure_ev;
        c->tm_scale = (float)std::exp2(c->tm_ev);
        HIPCHK(c, rmr::launch_tonemap(src, c->d_tm, px, nullptr, c->tm_scale, q.curve, iw2, c->stream));
        c->tm_used = 1;
    }
    c->st.tonemap_queued(source);
    return RMR_OK;
}

int rmr_read_tonemapped(rmr_ctx* c, float* rgba, size_t bytes) {
    if (!c || !rgba) return RMR_E_INVALID;
    RMR_FLUSH(c);
    const size_t need = (size_t)c->W * c->H * sizeof(float4);
    if (bytes < need) return fail(c, RMR_E_INVALID, "buffer too small");
    if (c->st.readable(RMR_OUTPUT_TONEMAPPED) < 0) return no_valid(c, RMR_OUTPUT_TONEMAPPED);
    return read_back(c, rgba, c->d_tm, need);
}

void* rmr_tonemapped_device_ptr(rmr_ctx* c) {
    if (!c) return nullptr;
    if (!flushed(c)) return nullptr;
    return c->st.readable(RMR_OUTPUT_TONEMAPPED) < 0 ? nullptr : (void*)c->d_tm;
}

int rmr_read_exposure(rmr_ctx* c, double* log2_scale, float* scale) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (c->tm_used == 0) return fail(c, RMR_E_STATE, "no exposure yet (call rmr_tonemap)");
    double l = c->tm_ev;
    float s = c->tm_scale;
    if (c->tm_used == 2) {
        // (rmr_tonemap_reset clears the state's valid word only: l and scale stay what the last call used)
        struct { double l; float scale; uint32_t valid; } head;
        static_assert(offsetof(rmr::ToneState, scale) == 8 && offsetof(rmr::ToneState, valid) == 12, "ToneState's head");
        if (const int r = read_back(c, &head, c->d_tm_state, sizeof head)) return r;
        l = head.l;
        s = head.scale;
    }
    if (log2_scale) *log2_scale = l;
    if (scale) *scale = s;
    return RMR_OK;
}

int rmr_luminance_histogram(rmr_ctx* c, int source, uint32_t hist[256], uint64_t* skipped) {
    if (!c || !hist) return RMR_E_INVALID;
    RMR_FLUSH(c);
    const float4* src = nullptr;
    int r;
    if ((r = tone_source(c, source, &src, true))) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if ((r = ensure_tonemap(c))) return r;
    rmr_tonemap_params q;
    rmr_default_tonemap_params(&q);
    if ((r = tone_meter(c, src, q, false))) return r;
    unsigned long long sk = 0;
    HIPCHK(c, hipMemcpyAsync(hist, c->d_tm_state->hist, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&sk, &c->d_tm_state->skipped, sizeof sk, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (skipped) *skipped = (uint64_t)sk;
    return RMR_OK;
}

int rmr_tonemap_reset(rmr_ctx* c) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!c->d_tm_state) return RMR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(&c->d_tm_state->valid, 0, sizeof(uint32_t), c->stream));
    return RMR_OK;
}

// ---- HDR bloom ahead of tone mapping (rmr_bloom.hip, bloom.cpp) -------------------------------------
static_assert(sizeof(rmr_bloom_params) == 32, "rmr_bloom_params is 32 bytes (include/rmr.h)");
namespace {
// The result plane and the pyramid (all eight levels, so that every `levels` finds room), at first use:
// both or neither.
int ensure_bloom(rmr_ctx* c) {
    if (c->d_bl) return RMR_OK;
    const rmr::BloomLevels L = rmr::bloom_levels(c->W, c->H, rmr::kBloomMaxLevels);
    if (const int r = alloc_all(c, {{&c->d_bl, (size_t)c->W * c->H * sizeof(float4)}, {&c->d_bl_pyr, L.total * sizeof(float4)}},
                                "cannot allocate the bloom plane (16 bytes per pixel) and its pyramid (a third of that)"))
        return r;
    c->st.bloom_reset();
    return RMR_OK;
}

// The stage's launches for src and q on the context's stream; what: 0 everything, 1 k_bloom_down0 alone,
// 2 k_bloom_compose alone (over the pyramid as it is).
hipError_t bloom_queue(rmr_ctx* c, const float4* src, const rmr_bloom_params& q, int what) {
    const int N = q.levels;
    const rmr::BloomLevels L = rmr::bloom_levels(c->W, c->H, rmr::kBloomMaxLevels);
    float4* pyr = c->d_bl_pyr;
    const float gain = rmr::bloom_gain(q.intensity, q.scatter, N);
    hipError_t e = hipSuccess;
    if (what == 1) return rmr::launch_bloom_down0(src, L.w[0], L.h[0], q.threshold, q.clamp, pyr + L.off[1], c->stream);
    if (what == 2) return rmr::launch_bloom_compose(src, L.w[0], L.h[0], pyr + L.off[1], gain, c->d_bl, c->stream);
    rmr::BloomTail t;
    const bool tail = c->bl_tail > 0 && rmr::bloom_tail_plan(L.w, L.h, N, c->bl_tail, q.threshold, q.clamp, q.scatter, &t);
    const int last_down = tail ? t.k0 - 1 : N;   // the levels the per-level kernels write
    if (last_down >= 1) e = rmr::launch_bloom_down0(src, L.w[0], L.h[0], q.threshold, q.clamp, pyr + L.off[1], c->stream);
    for (int k = 2; k <= last_down && e == hipSuccess; k++)
        e = rmr::launch_bloom_down(pyr + L.off[k - 1], L.w[k - 1], L.h[k - 1], pyr + L.off[k], c->stream);
    if (tail && e == hipSuccess)
        e = rmr::launch_bloom_tail(t.k0 == 1 ? src : pyr + L.off[t.k0 - 1], pyr + L.off[t.k0], t, c->stream);
    for (int k = (tail ? t.k0 - 1 : N - 1); k >= 1 && e == hipSuccess; k--)
        e = rmr::launch_bloom_up(pyr + L.off[k], L.w[k], L.h[k], pyr + L.off[k + 1], q.scatter, c->stream);
    if (e == hipSuccess) e = rmr::launch_bloom_compose(src, L.w[0], L.h[0], pyr + L.off[1], gain, c->d_bl, c->stream);
    return e;
}
}  // namespace

int rmr_bloom(rmr_ctx* c, int source, const rmr_bloom_params* p) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_bloom_params q;
    rmr_default_bloom_params(&q);
    if (p) q = *p;
    if (!rmr::bloom_params_ok(q))
        return fail(c, RMR_E_INVALID, "bad bloom params (levels 1..8, threshold >= 0, clamp >= 0, 0 <= scatter <= 1, "
                                      "intensity >= 0, reserved 0)");
    const float4* src = nullptr;
    int r;
    if ((r = tone_source(c, source, &src))) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if ((r = ensure_bloom(c))) return r;
    c->st.bloom_begin();   // (until everything below is queued; a tonemapped image of the old bloom image goes too)
    HIPCHK(c, bloom_queue(c, src, q, 0));
    c->st.bloom_queued(source);
    return RMR_OK;
}

int rmr_read_bloom(rmr_ctx* c, float* rgba, size_t bytes) {
    if (!c || !rgba) return RMR_E_INVALID;
    RMR_FLUSH(c);
    const size_t need = (size_t)c->W * c->H * sizeof(float4);
    if (bytes < need) return fail(c, RMR_E_INVALID, "buffer too small");
    if (c->st.readable(RMR_OUTPUT_BLOOM) < 0) return no_valid(c, RMR_OUTPUT_BLOOM);
    return read_back(c, rgba, c->d_bl, need);
}

void* rmr_bloom_device_ptr(rmr_ctx* c) {
    if (!c) return nullptr;
    if (!flushed(c)) return nullptr;
    return c->st.readable(RMR_OUTPUT_BLOOM) < 0 ? nullptr : (void*)c->d_bl;
}

#if RMR_DIAG
// Diagnostic library only (not in include/rmr.h; tools/bloom_time.py, tests/test_gpu_bloom.py): the most
// pixels the tail kernel's levels hold together, 0 = per-level launches only, -1 = the default. The
// results are the same either way.
int rmr_diag_bloom_tail(rmr_ctx* c, int max_pixels) {
    if (!c || max_pixels < -1) return RMR_E_INVALID;
    c->bl_tail = max_pixels < 0 ? rmr::kBloomTailDefault : max_pixels;
    return RMR_OK;
}

// Diagnostic library only (not in include/rmr.h; tools/bloom_time.py): *ms = the GPU's time per round of n
// back-to-back rounds of one thing on the accumulator: 0 the whole stage at `levels` as rmr_bloom queues it,
// 1 k_bloom_down0, 2 k_bloom_compose, 3 a device-to-device copy of the accumulator into the bloom plane (the
// yardstick). Queued behind a busy stream and between two events, as rmr_diag_tonemap_time does (32 k_meter
// launches; n <= 64 keeps the host ahead). Synchronises. The bloom image is invalid afterwards.
int rmr_diag_bloom_time(rmr_ctx* c, int which, int levels, int n, float* ms) {
    if (!c || !ms || which < 0 || which > 3 || levels < 1 || levels > rmr::kBloomMaxLevels || n < 1 || n > 64) return RMR_E_INVALID;
    RMR_FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if ((r = ensure_tonemap(c))) return r;
    if ((r = ensure_bloom(c))) return r;
    c->st.bloom_begin();
    const size_t px = (size_t)c->W * c->H;
    rmr_bloom_params q;
    rmr_default_bloom_params(&q);
    q.levels = levels;
    return timed_rounds(c, false, false, n, ms, [&] {
        if (which == 3) return hipMemcpyAsync(c->d_bl, c->d_accum, px * sizeof(float4), hipMemcpyDeviceToDevice, c->stream);
        return bloom_queue(c, c->d_accum, q, which);
    });
}

// Diagnostic library only (not in include/rmr.h; tools/bake_time.py): the radiance bake's own kernels alone,
// k_bake_rays and k_bake_fold of every launch of rmr_bake_points_device's plan without the trace between them
// (the fold reads whatever the planes hold). Queued on the context's stream, no synchronisation.
int rmr_diag_bake_kernels(rmr_ctx* c, const float* d_points, const float* d_normals, size_t n, const float* times,
                          uint32_t nspp, const rmr_bake_params* params, float* d_out_rgba) {
    if (!c || !d_points || !d_normals || !d_out_rgba || n == 0) return RMR_E_INVALID;
    RMR_FLUSH(c);
    rmr_bake_params q;
    int r;
    if ((r = bake_args(c, "rmr_diag_bake_kernels", n, times, nspp, params, q))) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if ((r = ensure_query(c))) return r;
    if ((r = ensure_qbuf(c, &c->d_bake_state, &c->bake_state_cap, n * sizeof(float4)))) return r;
    rmr::BakeList B{d_points, d_normals, (uint64_t)n, q.first_index, nullptr, nspp, q.bias, q.origin_extent};
    if ((r = stage_times(c, times, nspp, &B.times))) return r;
    const size_t n_ts = ((n + 63) / 64) * (size_t)nspp;
    const size_t chunk = rmr::plan_samples(64, (uint32_t)n_ts, c->samp_budget, 0, sizeof(float4) + rmr::kRayRecordBytes).per_launch;
    for (size_t k0 = 0; k0 < n_ts; k0 += chunk) {
        const uint32_t cnt = (uint32_t)std::min(chunk, n_ts - k0);
        if ((r = ensure_samp(c, (size_t)cnt * 64)) || (r = ensure_rays(c, (size_t)cnt * 64))) return r;
        c->last_samp = c->d_samp;
        HIPCHK(c, rmr::launch_bake_rays(B, k0, cnt, c->d_rays, nullptr, c->stream));
        HIPCHK(c, rmr::launch_bake_fold(false, c->d_samp, c->d_rays, (float4*)c->d_bake_state, n, nspp, k0, cnt, d_out_rgba, c->stream));
    }
    return RMR_OK;
}

// Diagnostic library only (not in include/rmr.h; tools/tonemap_time.py): whether k_lum_hist folds equal
// bins inside the wave before the LDS add; the counts are the same either way.
int rmr_diag_tonemap_fold(rmr_ctx* c, int on) {
    if (!c) return RMR_E_INVALID;
    c->tm_fold = on != 0;
    return RMR_OK;
}

// Diagnostic library only (not in include/rmr.h; tools/probe_time.py): the probe fold's mapping, 0 the build's
// default, 1 one thread per (probe, basis function), 2 one thread per probe. The results are the same.
int rmr_diag_probe_fold(rmr_ctx* c, int mapping) {
    if (!c || mapping < 0 || mapping > 2) return RMR_E_INVALID;
    c->probe_fold_mapping = mapping;
    return RMR_OK;
}

// Diagnostic library only (not in include/rmr.h; tools/tonemap_time.py): *ms = the GPU's time per launch of
// n back-to-back launches of one thing on the accumulator: 0 k_lum_hist, 1 k_meter (over the slab the last
// k_lum_hist left), 2 k_tonemap with the state's scale, 3 a device-to-device copy of the accumulator into
// the tonemapped plane (the yardstick), 4 the three kernels as an auto-exposed rmr_tonemap queues them.
// So that the time is the GPU's and not the host's enqueue rate, the stream is first kept busy (32 k_meter
// launches, about 0.9 ms) while the host queues the first event, the n launches and the second event
// behind it; n <= 64 keeps the host ahead. Synchronises. The tonemapped image is invalid afterwards.
int rmr_diag_tonemap_time(rmr_ctx* c, int which, int n, float* ms) {
    if (!c || !ms || which < 0 || which > 4 || n < 1 || n > 64) return RMR_E_INVALID;
    RMR_FLUSH(c);
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if ((r = ensure_tonemap(c))) return r;
    c->st.tonemap_begin();
    const size_t px = (size_t)c->W * c->H;
    const int blocks = rmr::lum_hist_blocks(px);
    rmr_tonemap_params q;
    rmr_default_tonemap_params(&q);
    const rmr::ToneMeter M = rmr::tonemap_meter(q);
    const float iw2 = rmr::tonemap_iw2(q);
    return timed_rounds(c, c->tm_fold, true, n, ms, [&] {
        hipError_t e = hipSuccess;
        if (which == 0 || which == 4) e = rmr::launch_lum_hist(c->d_accum, px, c->d_tm_slab, blocks, c->tm_fold, c->stream);
        if ((which == 1 || which == 4) && e == hipSuccess)
            e = rmr::launch_meter(c->d_tm_slab, blocks, c->d_tm_state, c->d_tm_lc, M, true, c->stream);
        if ((which == 2 || which == 4) && e == hipSuccess)
            e = rmr::launch_tonemap(c->d_accum, c->d_tm, px, c->d_tm_state, 0.0f, q.curve, iw2, c->stream);
        if (which == 3) e = hipMemcpyAsync(c->d_tm, c->d_accum, px * sizeof(float4), hipMemcpyDeviceToDevice, c->stream);
        return e;
    });
}

// Diagnostic library only (not in include/rmr.h; tools/denoise_time.py): which a-trous passes run the
// LDS-tiled form, bit i = the pass of step 2^i (i < 2); the results are the same either way.
int rmr_diag_denoise_tiled(rmr_ctx* c, int mask) {
    if (!c || mask < 0 || mask > 3) return RMR_E_INVALID;
    c->dn_tiled_steps = mask;
    c->dnv_tiled_steps = mask;
    return RMR_OK;
}

// Diagnostic library only (not in include/rmr.h; tools/temporal_time.py): while on, rmr_temporal_accumulate
// runs its kernel against the history it has and leaves that history (image, guides and view) in place,
// so that repeated calls time the kernel alone on one view pair.
int rmr_diag_temporal_keep(rmr_ctx* c, int on) {
    if (!c) return RMR_E_INVALID;
    c->t_keep = on != 0;
    return RMR_OK;
}

// Diagnostic library only (not in include/rmr.h): the escape bound ray_exit at n given rays (rays:
// o.xyz, d.xyz per ray) with the context's scene, view and maxDist, as a launch would use it; out[i]
// = the bound (+inf: none). boxes (optional, 6 floats per box, up to max_boxes) receives the inflated
// escape boxes the kernel read, *n_boxes their number (0: the bound is off for this scene).
int rmr_diag_ray_exit(rmr_ctx* c, const float* rays, int n, float* out, float* boxes, int max_boxes, int* n_boxes) {
    if (!c) return RMR_E_INVALID;
    RMR_FLUSH(c);
    if (!c->scene_loaded) return fail(c, RMR_E_STATE, "no scene loaded");
    if (n < 0 || (n > 0 && (!rays || !out))) return fail(c, RMR_E_INVALID, "bad rays / out");
    if (!c->view_set) default_view(c);
    KParams P{};
    int rr;
    if ((rr = escape_params(c, P))) return rr;
    if (n_boxes) *n_boxes = P.esc_on ? P.n_esc : 0;
    if (boxes && P.esc_on && max_boxes > 0) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(boxes, c->d_esc, sizeof(float) * 6 * (size_t)std::min(max_boxes, P.n_esc), hipMemcpyDeviceToHost));
    }
    if (n == 0) return RMR_OK;
    float *d_rays = nullptr, *d_out = nullptr;
    HIPCHK(c, hipMalloc((void**)&d_rays, sizeof(float) * 6 * (size_t)n));
    HIPCHK(c, hipMalloc((void**)&d_out, sizeof(float) * (size_t)n));
    hipError_t e = hipMemcpyAsync(d_rays, rays, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = rmr::launch_ray_exit(P, d_rays, d_out, n, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_rays);
    (void)hipFree(d_out);
    HIPCHK(c, e);
    return RMR_OK;
}
#endif

int rmr_abi_sizes(int32_t* out, int n) {
    const int32_t s[] = {(int32_t)sizeof(rmr_prim), (int32_t)sizeof(rmr_op), (int32_t)sizeof(rmr_material),
                         (int32_t)sizeof(rmr_spectral), (int32_t)sizeof(rmr_rm2_consts), (int32_t)sizeof(rmr_scene),
                         (int32_t)sizeof(rmr_params), (int32_t)sizeof(rmr_stats)};
    const int m = (int)(sizeof s / sizeof s[0]);
    for (int i = 0; i < n && i < m; i++) out[i] = s[i];
    if (n >= 9) out[8] = (int32_t)sizeof(rmr_denoise_params);   // (beyond the returned count, see rmr.h)
    return m;
}

}  // extern "C"
