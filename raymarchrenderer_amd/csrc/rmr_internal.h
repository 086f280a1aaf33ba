// rmr_internal.h — kernel launch parameters shared by the host API (rmr_api.cpp) and the kernels.
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif
#include "../../include/rmr_tables.h"

namespace rmr {

// One 8x8 pixel tile = one wave's initial 64 paths (the reference RM1 workgroup shape,
// RayMarch.glsl:11). tiles[] holds the tile origin (x, y) in pixels.
struct TileXY { int32_t x, y; };

// Packed primitive for the sphere/box fast paths: one s_load_dwordx8 per prim.
struct DPrim {
    float c[3];
    float r[3];
    int32_t type;  // RMR_PRIM_SPHERE / RMR_PRIM_BOX; 0 = padding (never evaluated)
    float mat_id;
};

// Material shading kind, precomputed on the host from the v1 node program (rmr_material).
enum MatKind : int32_t {
    MAT_NONE = 0,      // no `case` for this id: outputs stay vec3(0) -> path ends black
    MAT_DIFFUSE = 1,   // single shader_diffuse(literal) node, color/dir wired straight out
    MAT_EMISSION = 2,  // single shader_emission(literal, literal) node, dir not written
    MAT_PROGRAM = 3,   // anything else: the generic node interpreter
};
struct DMat {
    int32_t kind;
    float c[3];   // diffuse / emission color literal
    float p[3];   // emission power literal
    float gray1;  // gray_ch(p, -1) = ((p.x + p.y) + p.z) / 3 (host, same float operations)
};

// Bounding-volume node of the exact culling map (NP = -2, scenes of more than 32 spheres/boxes).
// Nodes are in depth-first pre-order: the first child of an internal node is the next node,
// `skip` is the node after the whole subtree. Leaves hold `count` primitives starting at `first`
// in the leaf-ordered DPrim array (DPrim.type carries the original scene index in bits 8..31).
struct BvhNode {
    float lo[3];
    int32_t first;
    float hi[3];
    int32_t count;   // 0 = internal node
    int32_t skip;
    int32_t pad[3];
};

// the trace kernel's work-queue counters (rmr_trace.h RMR_QUEUE_PARTS partitions, 128 B apart; room
// for 64): zero when a trace launch starts. Zeroed once at rmr_create (and at a launch slot's creation),
// then by each launch's fold (fold_main, ordered after its trace) for the next launch on the same queue,
// so a launch costs no separate memset dispatch (the reference's one-sample Graphics::Render calls: one
// dispatch fewer per call)
constexpr size_t kQueueBytes = 8192;
constexpr int kQueueWordStride = 32;   // 32-bit words between two partition counters

// The kernels' raw device counters (KParams::counters; rmr_get_counters_n): kCounterSlots 64-bit words.
// [0..15] as rmr.h documents them (the flop-count and other diagnostic builds use 9..15 as well). From
// 16 up every counter has a slot of its own:
constexpr int kCounterSlots = 74;
constexpr int kCntOverflow = 16;         // lane-slot kernels: events deposited into another lane's empty slot
// lane-slot kernels with trailing steps (rmr_trace.h RMR_TRAIL_STEPS), every build:
constexpr int kCntTrailSteps = 31;       //   trailing steps taken (lane-level; part of counter 0)
constexpr int kCntTrailPasses = 32;      //   trailing passes run (wave-level)
constexpr int kCntTrailLanes = 33;       //   lanes evaluated in those passes (taken + refused)
// ... built with -DRMR_TRAIL_CHECK (a diagnostic; the word is free in the lane-slot kernels' other builds but
// the wave-times one): lanes evaluated in passes at a point whose eps(p) exceeds KParams::trail_eps_hi
constexpr int kCntTrailCheck = 12;
// RMR_PROFILE builds (rmr_trace.h trace_main), zero otherwise:
constexpr int kCntProfClaim = 17;        // refill: cycles in work-queue claims
constexpr int kCntProfRays = 18;         // refill: cycles in the chunk's primary rays
constexpr int kCntProfUhits = 19;        // lane-slot kernels: hits the certificate did not cover
constexpr int kCntProfUhitsCheap = 20;   //   those that end their path
constexpr int kCntProfFullLanes = 21;    // cache kernels: lanes in the full map() batches
constexpr int kCntProfOuter = 22;        // lane-slot kernels: outer-loop passes
constexpr int kCntProfPark = 23;         //   park steps
constexpr int kCntProfParkOvf = 24;      //   park steps with an overflow deposit
constexpr int kCntProfLostFin = 25;      //   map-loop lane-iterations of lanes whose march ended (awaiting the park step)
constexpr int kCntProfLostWait = 26;     //   map-loop lane-iterations of lanes waiting in registers on a full slot
constexpr int kCntProfBatchEv = 27;      //   events in the shading batches (batches: counter 2)
constexpr int kCntProfLostIdle = 28;     //   map-loop lane-iterations of idle lanes while the queue has work
constexpr int kCntProfLostIdleExh = 29;  //   the same once the wave found the queue used up (the drain)
constexpr int kCntProfReadyWait = 30;    //   ready rays waiting in a slot whose lane marches, summed over map-loop iterations
// ... the trailing passes by pass index: kCntProfTrail + ((queue used up ? kCntProfTrailIdx : 0) + min(pass
// index, kCntProfTrailIdx - 1)) * kCntProfTrailWhat + what, what = 0 passes run, 1 lanes taking part, 2 lanes
// accepted, 3 the wave's active lanes at the pass's start, 4 its finished lanes sitting through the pass
constexpr int kCntProfTrail = 34;
constexpr int kCntProfTrailIdx = 4;
constexpr int kCntProfTrailWhat = 5;
static_assert(kCntProfTrail + 2 * kCntProfTrailIdx * kCntProfTrailWhat == kCounterSlots, "the profile build's pass counters end the block");

struct KParams {
    // ---- scene tables (device pointers, read-only) ----
    const rmr_prim* prims;
    const rmr_op* ops;
    const float* consts;
    const rmr_material* mats;
    const rmr_spectral* spec;
    const rmr_rm2_consts* rm2;
    const DPrim* dprims;        // packed prims (fast map paths)
    const DMat* dmats;          // per-id shading kind (RM1)
    const BvhNode* bvh;         // NP = -2: node array (n_nodes), prims in dprims in leaf order
    int32_t n_nodes;
    // approximate minimum below which the exact one is < max_dist (rmr_trace.h am_far); in the four bytes
    // that pad n_nodes to the next pointer, so that no other field moves (a field added further down
    // changed the kernels' scalar-load grouping and SGPR spills: RM3 +25 instructions)
    float am_dmax;
    // candidate grid of the nearest-primitive cache's full map() (rmr_trace.h map_grid_npc; null =
    // none): per cell x = list offset | count << 24 (count 255: no list, take the BVH), y = float bits
    // of a lower bound of every non-listed primitive's float distance in the cell, z / w = the list's
    // first four leaf indices (16 bits each, z low first), inline; lists of leaf indices; leaf indices
    // [0, grid_n_large) are evaluated everywhere (large primitives)
    const uint4* grid;
    const uint16_t* grid_list;
    float grid_lo[3];
    float grid_inv;             // 1 / cell size
    int32_t grid_dim[3];
    float grid_dimf[3];         // the same as floats (the kernel's range test compares against SGPR
                                // operands instead of converted values the allocator would spill)
    int32_t grid_n_large;
    float grid_sbox[6];         // box of the small primitives (lo.xyz, hi.xyz), rounded outward
    float bvh_margin;           // absolute part of the culling margin (scales with the scene extent)
    float am_r2;                // 2 x the largest |sphere radius| (approximate-then-exact map, rmr_trace.h)
    float npc_eps0;             // nearest-primitive cache: 2^-17 E + 2^-60 (rmr_trace.h npc_eps)
    float cert_k;               // certified getNormal probes: the bound of rmr_trace.h am_normal_cert
    int32_t esc_on;             // escape bound (rmr_trace.h ray_exit): sphere/box scenes
    int32_t eye_step;           // primary rays' first march step from map(eye) (rmr_trace.h eye_map)
    // trailing steps: the launch's bound of eps(x) at every point a pass evaluates (rmr_trail_rule.h; +inf:
    // no pass runs); in the four bytes that pad eye_step to the next pointer, so that no other field moves
    float trail_eps_hi;
    const float* esc_boxes;     // n_esc inflated boxes (lo.xyz, hi.xyz) covering every primitive
    int32_t n_esc;
    int32_t full_threshold;     // nearest-primitive cache: bits 0-7 lanes per full map() batch; bits 8-15 R:
                                // also a batch once waiting lanes x R >= 8 x cache-served lanes
    int32_t n_prims;
    int32_t n_mats;
    int32_t v2_begin, v2_end;
    rmr_spectral spec_sky;
    float sky[3];
    const float4* env;          // envTex texels (c / 255, RGBA), row 0 = t 0; used when use_env
    int32_t env_w, env_h, use_env;
    float rm2_light[3];
    float rm2_light_power;
    int32_t rm2_node_id;
    // ---- render parameters (Graphics::Render uniforms) ----
    float max_dist, step_mult;
    int32_t max_steps, max_bounces, separate_channels;
    // ---- view (setView uniforms, shader order) ----
    float eye[3], r00[3], r01[3], r10[3], r11[3];
    int32_t W, H;
    // host-computed uniforms the kernels would otherwise derive per wave with VALU ops (whose results
    // the allocator keeps in VGPRs for the whole kernel, and spills): r01 - r00, r11 - r10 (float
    // subtraction, the same bits), (float)W, (float)H, and the env map's (float) w, h, w - 1, h - 1
    float dr01[3], dr11[3];
    float Wf, Hf;
    float env_wf[4];
    float eye_xy;               // eye.x + eye.y (the first sum of a primary ray's ray_exit NaN check)
    // ---- work ----
    int32_t x0, y0, x1, y1;     // clip rect (pixels inside = rendered)
    const TileXY* tiles;        // n_tiles tiles
    int32_t n_tiles;
    uint32_t nspp;              // samples in this launch
    uint32_t first_sample;      // running-mean index of sample 0
    const float* times;         // [nspp] rand() seed per sample (null when nspp == 1: time1)
    float time1;                // the seed of a one-sample launch, as a kernel argument (no copy)
    uint64_t n_units;           // nspp * n_tiles * 64
    uint32_t chunk_units;       // units a wave takes per claim (0: the kernel's chunk; smaller for small
                                // launches, so they spread over every CU, rmr_api.cpp render_tiles)
    float4* samp;               // [nspp][n_tiles][64] per-sample radiance
    float4* accum;              // W*H running mean
    unsigned long long* queue;  // persistent work counters (kQueueBytes: one per partition, 128 B apart)
    unsigned long long* counters; // [0] map evals, [1] samples traced
    int32_t flops_static;       // count builds (RMR_COUNT_FLOPS): flops of one map() fold without the
    int32_t transc_static;      //   Mandelbulb iterations, and its transcendentals (scene.cpp)
    int32_t shade_threshold;    // deferred-shading batch size (lanes); lane-slot kernels (rmr_trace.h
                                // RMR_LANE_SLOTS): finished marches per park step | slot events per batch << 8
    int32_t refill_threshold;   // idle lanes before a wave fetches new units
};
static_assert(__builtin_offsetof(KParams, trail_eps_hi) + 4 == __builtin_offsetof(KParams, esc_boxes) &&
                  __builtin_offsetof(KParams, esc_boxes) == 192,
              "trail_eps_hi fills the padding ahead of esc_boxes: no other field moves");

// One pass of the a-trous preview filter (rmr_denoise.hip): in -> out (W x H float4 each, never the
// same buffer) guided by the first-hit planes of rmr_guides.hip.
struct DenoisePass {
    const float4* in;
    float4* out;
    const float4* hit;          // (pos.xyz, t)
    const float4* nrm;          // (normal.xyz, id); id < 0: no hit
    int32_t W, H;
    int32_t step;               // 2^i: pixels between taps
    int32_t normal_pow2;        // squarings of max(0, n_p . n_q)
    float sigma_z_step;         // sigma_z * step
    float inv_sigma_c2;         // 1 / (sigma_c 2^-i)^2; 0: no colour term
};

// The variance-guided filter (rmr_denoise_var.hip). The seed: the per-pixel variance
// estimate of the accumulator A from the half image B, W x H floats, -1 where the pixel is not v-live.
struct VarianceSeed {
    const float4* a;
    const float4* b;
    const float4* nrm;          // (normal.xyz, id)
    float* out;
    int32_t W, H;
    int32_t radius;             // the window is (2 radius + 1)^2 pixels, 0..4
};
// One guided pass: DenoisePass's, with the variance plane filtered alongside (never the same buffer in
// and out). A pixel is v-live iff var_in >= 0.
struct DenoiseVarPass {
    DenoisePass d;
    const float* var_in;
    float* var_out;
    float sigma_l;
};
// Temporal reprojection of the preview (rmr_temporal.hip): the source image d.in and
// the current guides d.hit / d.nrm against a history (colour, effective sample count and the guides it
// was made with), into d.out / n_out, never the history's own buffers. d.step is 1, d.sigma_z_step is
// sigma_z and d.inv_sigma_c2 is 0, so rmr_atrous.h's tap_weight is the stage's a_q z_q.
struct TemporalPass {
    DenoisePass d;
    const float4* h_col;
    const float* h_n;           // 0: no history at that pixel
    const float4* h_hit;
    const float4* h_nrm;
    float* n_out;
    float2* xy_out;             // the projected coordinates (NaN: none), or null
    float eye[3];               // the history view's eye
    float minv[9];              // [r01'-r00' | r10'-r00' | r00']^-1, row-major (temporal.hpp view_inverse)
    float twist[3];             // that inverse times (r11'-r10') - (r01'-r00')
    float Wf, Hf;
    float n_cur;                // the source's sample count
    float max_history;
};
// Tone mapping and auto-exposure (rmr_tonemap.hip): what k_meter leaves in device
// memory, the adaptation state (l, scale, valid) and the summed histogram of the last metered plane.
struct ToneState {
    double l;                   // log2 of the scale
    float scale;                // (float)exp2(l): k_tonemap reads this word
    uint32_t valid;             // 0: no previous state
    uint32_t hist[256];
    unsigned long long skipped;
};
constexpr int kToneSlabRows = 512;   // most blocks k_lum_hist runs: rows of the [rows][257] slab
struct ToneMeter;                    // rmr_tonemap_rule.h
constexpr int kBloomTailThreads = 1024;
constexpr int kBloomTailPixels = 12288;   // 12 B each: 144 KiB of the CU's 160 KiB of LDS
// The levels the tail takes by default, in pixels of all of them together (measured, DESIGN.md §4.14: from
// 60x34 down the tail beats the per-level launches, from 120x68 down it loses to them).
constexpr int kBloomTailDefault = 4096;
struct BloomTail {
    int k0, count;              // the levels k0 .. k0 + count - 1 (count >= 2)
    int w_in, h_in;             // the size of level k0 - 1, the tail's input
    int from_source;            // k0 = 1: the input is the source image, read through the bright part
    float threshold, clamp, scatter;
};
#ifndef __HIPCC_RTC__
int lum_hist_blocks(size_t n);
// fold: equal bins are folded inside the wave before the LDS add (the same counts either way)
hipError_t launch_lum_hist(const float4* in, size_t n, uint32_t* slab, int blocks, bool fold, hipStream_t s);
hipError_t launch_meter(const uint32_t* slab, int rows, ToneState* st, const double* lc, const ToneMeter& M, bool run_meter,
                        hipStream_t s);
// st: the state whose scale is applied, or null for `scale` itself
hipError_t launch_tonemap(const float4* in, float4* out, size_t n, const ToneState* st, float scale, int curve, float iw2,
                          hipStream_t s);
// HDR bloom (rmr_bloom.hip). down0: P of the w x h source and the first down, into the
// bloom_half(w) x bloom_half(h) level `out`; down: one level to the next; up: U_k = B_k + s up(U_{k+1}) in
// place on the w x h level `bk`, `uk1` being bloom_half(w) x bloom_half(h); compose: out = src + gain up(u1)
// with the copy rule, u1 being bloom_half(w) x bloom_half(h).
// The tail: the levels k0 .. k0 + count - 1 (the last one the pyramid's last), downs and ups, by one block in
// LDS; `in` is level k0 - 1 (the source image when k0 = 1), `out` level k0, which receives U_k0.
// bloom_tail_plan: the tail of a pyramid of `levels` levels of sizes w[k] x h[k], k0 being the first level
// from which all of them hold at most max_pixels pixels (and kBloomTailPixels) together; false where that is
// fewer than two levels.
hipError_t launch_bloom_tail(const float4* in, float4* out, const BloomTail& t, hipStream_t s);
bool bloom_tail_plan(const int* w, const int* h, int levels, int max_pixels, float threshold, float clamp, float scatter,
                     BloomTail* t);
hipError_t launch_bloom_down0(const float4* src, int w, int h, float threshold, float clamp, float4* out, hipStream_t s);
hipError_t launch_bloom_down(const float4* in, int w, int h, float4* out, hipStream_t s);
hipError_t launch_bloom_up(float4* bk, int w, int h, const float4* uk1, float scatter, hipStream_t s);
hipError_t launch_bloom_compose(const float4* src, int w, int h, const float4* u1, float gain, float4* out, hipStream_t s);
hipError_t launch_temporal(const TemporalPass& T, hipStream_t s);
hipError_t launch_variance_seed(const VarianceSeed& V, hipStream_t s);
// tiled: the LDS form (step 1 or 2 only; other steps run the plain form)
hipError_t launch_atrous_var(const DenoiseVarPass& A, bool tiled, hipStream_t s);
#endif

}  // namespace rmr
