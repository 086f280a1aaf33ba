/*
 * rmr.h — C ABI of the MI355X-native SDF ray-march path tracer (librmr.so).
 *
 * This is the drop-in boundary for the reference's render backend, the static C++ class
 * `Graphics` (RayMarch Renderer/Graphics.h:15-134, Graphics.cpp:215-835), which had no FFI of its
 * own. Each entry point names the reference member it replaces. Conventions:
 *   - plain C, opaque handle, int status (RMR_OK = 0, negative = error), message through
 *     rmr_last_error(ctx); nothing throws across the boundary;
 *   - caller-owned host buffers, library-owned device memory (or caller-bound device memory via
 *     rmr_bind_accum), one context per thread;
 *   - calls are asynchronous w.r.t. the GPU exactly like the reference's glDispatchCompute;
 *     rmr_sync / rmr_read_accum / rmr_save_bmp synchronise.
 * INTEGRATION.md shows the binding a maintainer adds on the reference side.
 */
#ifndef RMR_H
#define RMR_H

#include <stddef.h>
#include <stdint.h>
#include "rmr_tables.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RMR_OK          0
#define RMR_E_INVALID  (-1) /* bad argument                                                  */
#define RMR_E_HIP      (-2) /* HIP runtime error / no device                                  */
#define RMR_E_SCENE    (-3) /* scene does not compile (the reference's shader compile error)  */
#define RMR_E_IO       (-4) /* file I/O                                                        */
#define RMR_E_STATE    (-5) /* call out of order (e.g. render before a scene is loaded)        */
#define RMR_E_NOMEM    (-6)
#define RMR_E_UNSUPPORTED (-7)

typedef struct rmr_ctx rmr_ctx;

/* Render parameters. Defaults = the constants Graphics::Render uploads (Graphics.cpp:326-340). */
typedef struct rmr_params {
    float   max_dist;          /* 1000                                                        */
    int32_t max_steps;         /* 512                                                         */
    int32_t max_bounces;       /* 16                                                          */
    float   step_multiply;     /* 0.5                                                         */
    int32_t separate_channels; /* 0                                                           */
    int32_t use_env_tex;       /* 0 (Graphics.cpp:338); 1 = skyColor from the env map          */
} rmr_params;

/* Kernel statistics for the roofline (accumulated since the last rmr_reset_stats). */
typedef struct rmr_stats {
    uint64_t map_evals;      /* scene-SDF evaluations (the algorithmic work unit)  */
    uint64_t samples;        /* pixel samples traced                                           */
    uint64_t trace_launches; /* trace-kernel launches                                          */
    double   trace_ms;       /* summed trace-kernel time measured with HIP events              */
    double   fold_ms;        /* summed accumulate-kernel time                                  */
    double   flops_per_map;  /* algorithmic flops of one map() for the loaded scene            */
    uint64_t map_iters;      /* wave-level map() iterations: map_evals/(64*map_iters) = lane use */
    uint64_t shade_batches;  /* wave-level deferred-shading batches                             */
    uint64_t jit_launches;   /* trace launches that ran the hipRTC scene-specialised kernel     */
} rmr_stats;

/* ---- lifetime --------------------------------------------------------------------------- */
/* Graphics::Init (Graphics.cpp:263-300): select device, create streams; no GL context needed. */
int  rmr_create(rmr_ctx** out, int device);
void rmr_destroy(rmr_ctx* ctx);
const char* rmr_last_error(const rmr_ctx* ctx);
/* Compile-time kernel configuration string (variants, wave size, build flags). */
const char* rmr_build_info(void);

/* Run kernels on a caller stream (a hipStream_t passed as void*). NULL gives the context a new
 * library-owned non-blocking stream (it does NOT select the legacy null stream): work the caller
 * orders on its own streams (zeroing the accumulator, a collective over it) must then be ordered
 * with rmr_sync, so pass the caller's stream whenever it shares buffers with the renderer. */
int rmr_set_stream(rmr_ctx* ctx, void* hip_stream);

/* ---- image / view / params ------------------------------------------------------------- */
/* Graphics::setImageSize / getImageSize (Graphics.cpp:817-825). The reference applies a new size
 * at the next Init/Reload (Graphics.cpp:744-745); rmr_reload does the same here. */
int rmr_set_image_size(rmr_ctx* ctx, int w, int h);
int rmr_get_image_size(const rmr_ctx* ctx, int* w, int* h);

int rmr_set_params(rmr_ctx* ctx, const rmr_params* p);
int rmr_get_params(const rmr_ctx* ctx, rmr_params* p);
void rmr_default_params(rmr_params* p);

/* Graphics::setView (Graphics.cpp:827-835), arguments in *shader-uniform* order. Note the
 * reference camera calls setView(eye, ray00, ray10, ray01, ray11) (Camera.cpp:101), so its
 * uniform "ray01" holds the camera's ray10. rmr_camera_view() below already applies that swap. */
int rmr_set_view(rmr_ctx* ctx, const float eye[3], const float ray00[3], const float ray01[3],
                 const float ray10[3], const float ray11[3]);

/* Camera::calculateRays (Camera.cpp:25-102) restated: eye/dir/aspect/fov -> the five uniforms in
 * shader order (eye, ray00, ray01, ray10, ray11), i.e. after the setView argument swap. */
void rmr_camera_view(const double eye[3], const double dir[3], float aspect, float fov,
                     float out_eye[3], float out_ray00[3], float out_ray01[3],
                     float out_ray10[3], float out_ray11[3]);

/* ---- scene ------------------------------------------------------------------------------- */
/* Graphics::clearScene/addMaterial/addObject + Reload's code generator (Graphics.cpp:392-752,
 * 801-815): parse a reference scene file (v1 or v2 format, App. C of SURVEY) for `variant` and
 * compile it into tables. Errors the reference would hit as a GLSL compile error (stale arity,
 * unknown node, bad var index) return RMR_E_SCENE with the message in rmr_last_error. */
int rmr_load_scene_json(rmr_ctx* ctx, int variant, const char* json, size_t len);
/* Context-free scene compilation (no GPU needed): compile to a library-owned table set, view it
 * as an rmr_scene, free it. On RMR_E_SCENE the reason is written to err (if errlen > 0). */
typedef struct rmr_scene_blob rmr_scene_blob;
int rmr_scene_compile(int variant, const char* json, size_t len, rmr_scene_blob** out, char* err, size_t errlen);
int rmr_scene_view(const rmr_scene_blob* blob, rmr_scene* out);
void rmr_scene_free(rmr_scene_blob* blob);
/* Load precompiled tables (copied). */
int rmr_load_scene_tables(rmr_ctx* ctx, const rmr_scene* scene);
/* The built-in scenes that the reference hard-codes in its shaders: RM2's one-sphere map
 * (RayMarch2.glsl:133-172, needs a v2 material for id 1 via rmr_load_scene_json) and RM3's
 * three-primitive spectral scene (RayMarch3.glsl:132-143, 251-345). */
int rmr_load_builtin_scene(rmr_ctx* ctx, int variant);

/* Graphics::Reload tail (Graphics.cpp:741-751): apply the pending image size and clear the
 * accumulator to (0,0,0,0). */
int rmr_reload(rmr_ctx* ctx);

/* ---- render ------------------------------------------------------------------------------ */
/* Graphics::Render (Graphics.cpp:314-354): add ONE sample to every pixel with
 * min <= pix < max, as the running mean of RayMarch*.glsl main() using `current_sample` (0
 * overwrites). `time` is the rand() seed uniform. */
int rmr_render(rmr_ctx* ctx, float time, float min_x, float min_y, float max_x, float max_y,
               uint32_t current_sample);
/* Call batching of rmr_render (the reference calls Graphics::Render once per tile and sample,
 * Program.cpp:232-284; one such launch renders one sample of a tile and is bound by its longest path,
 * not by the chip). With batching on, rmr_render records the call (checking its state errors at once)
 * and launches nothing; consecutive samples of a rect, and rects holding the same samples, go out
 * together as one launch when any other entry point is called (rmr_sync, rmr_read_accum, rmr_save_bmp,
 * rmr_display, a setter, ...; rmr_accum_device_ptr included), when an overlapping rect or a
 * non-consecutive sample of a held rect arrives, or when 2^28 units are held. Bitwise equal to
 * unbatched calls (each pixel's samples, their seeds and their running-mean order are the same). Like
 * GL, which also queues the reference's dispatches until something reads their results, the work
 * starts at the next flush: a caller that orders its own stream work on the context's accumulator
 * without calling into rmr must flush first (rmr_sync). mode 1 on, 0 off, -1 auto (default): on while
 * the context owns its stream and its accumulator (no rmr_set_stream / rmr_bind_accum), since only
 * then are all readers inside rmr. rmr_destroy drops calls still held. */
int rmr_set_call_batching(rmr_ctx* ctx, int mode);
/* Launch overlap: n >= 2 (default 2; 4 with 8 or more hardware queues) puts consecutive trace launches round-robin on n private
 * streams, each with its own sample planes and work queue, so one launch's drain (its last long paths)
 * overlaps the next launch's start; n = 0 or 1 runs every launch on the context's stream. Each
 * launch's fold stays on the context's stream, after its trace and in call order, so results are
 * bitwise the same, and work the caller orders after a call on that stream still sees the call's
 * samples. Costs one sample-plane buffer per stream; launches whose planes exceed the plane budget / n
 * run on the context's stream. At most 4. Several contexts that already overlap each other's frames
 * (multi_gpu.FrameRenderer, the device group) set 0: their streams would exceed the GPU's hardware
 * queues (4 per process) and serialise. */
int rmr_set_launch_streams(rmr_ctx* ctx, int n);
/* The context's launch streams (rmr_create's default: 2, or 4 where the process has 8 or more hardware
 * queues, GPU_MAX_HW_QUEUES); -1 for a null context. */
int rmr_get_launch_streams(const rmr_ctx* ctx);
/* Batched fast path: samples first_sample .. first_sample+nspp-1 of every pixel in the integer
 * rect [x0,x1)x[y0,y1), sample k seeded with times[k]. Bitwise equal to nspp rmr_render calls
 * with the same times. */
int rmr_render_spp(rmr_ctx* ctx, const float* times, int x0, int y0, int x1, int y1,
                   uint32_t first_sample, uint32_t nspp);
/* Same as rmr_render_spp but over an explicit tile list (tile_size x tile_size tiles, given as
 * (tx,ty) pairs): the multi-GPU partition unit. Each (tx,ty) may appear at most once (a repeated or
 * negative tile is RMR_E_INVALID: two threads would fold into the same pixel). */
int rmr_render_tiles(rmr_ctx* ctx, const float* times, const int32_t* tiles_xy, int n_tiles,
                     int tile_size, uint32_t first_sample, uint32_t nspp);

/* ---- output ------------------------------------------------------------------------------ */
/* Accumulator as RGBA32F, row 0 = image row 0 (= the top edge). */
int rmr_read_accum(rmr_ctx* ctx, float* rgba, size_t bytes);
int rmr_write_accum(rmr_ctx* ctx, const float* rgba, size_t bytes); /* checkpoint resume */
/* Device pointer of the accumulator (float4 per pixel) for collectives (RCCL reduce). */
void* rmr_accum_device_ptr(rmr_ctx* ctx);
/* Render into caller-owned device memory of w*h*16 bytes instead (e.g. a torch tensor). */
int rmr_bind_accum(rmr_ctx* ctx, void* device_ptr, size_t bytes);
/* Graphics::SaveImage (Graphics.cpp:754-799): 24-bit BMP with the reference's quirks
 * (u8 round, 1.055*c^(1/2.4) without -0.055, truncation, SOIL pink background for alpha 0). */
int rmr_save_bmp(rmr_ctx* ctx, const char* path);
/* The same encoding from a host RGBA32F buffer (no context needed). */
int rmr_encode_bmp(const float* rgba, int w, int h, const char* path);
/* Raw float accumulator checkpoint: "RMRACC1\0", w, h, samples, then RGBA32F. */
int rmr_save_accum(rmr_ctx* ctx, const char* path, uint32_t samples_done);
int rmr_load_accum(rmr_ctx* ctx, const char* path, uint32_t* samples_done);

int rmr_sync(rmr_ctx* ctx);
int rmr_get_stats(rmr_ctx* ctx, rmr_stats* out);
int rmr_reset_stats(rmr_ctx* ctx);
/* Profiling builds only (librmr compiled with -DRMR_PROFILE; zeros otherwise): per-wave shader-clock
 * cycles summed over all waves since rmr_reset_stats, split into [0] refill/ray setup, [1] map()
 * iterations, [2] shading batches, [3] whole trace loop. */
int rmr_get_section_cycles(rmr_ctx* ctx, uint64_t out[4]);
/* Raw kernel counters (diagnostics): [0] map evals, [1] map iterations, [2] shading batches,
 * [3] full map() batches of the nearest-primitive cache, [8] lanes shaded (lane-level shading events),
 * [14] map evals in shading batches (certified getNormal probes, rmr_trace.h cert_normals; part of [0]),
 * [4..7] the section cycles above (or the RMR_JIT_AMBCOUNT fallback counts, tools/amb_rate.py). */
int rmr_get_counters(rmr_ctx* ctx, uint64_t out[16]);
/* The first n of the whole counter block (n <= 74; [34..73]: the profiling build's counts of the trailing
 * passes by pass index, rmr_internal.h kCntProfTrail, zeros in every other build). [0..15] as above; [16] events the lane-slot kernels
 * deposited into another lane's empty slot (the overflow deposit, rmr_trace.h RMR_SLOT_OVERFLOW);
 * [17..30] the profiling build's counters, each in a slot of its own (rmr_internal.h kCntProf*: refill
 * claim / ray cycles, uncertified hits, lanes per full map() batch, and the lane-slot schedule's passes,
 * park steps, lost lane-iterations by cause and events per batch); zeros in every other build;
 * [31..33] the trailing steps of the lane-slot kernels (rmr_set_trail_steps), in every build: steps taken
 * (lane-level; part of [0]), passes run (wave-level), lanes evaluated in the passes (taken + refused);
 * [12] in a lane-slot kernel built with -DRMR_TRAIL_CHECK (a diagnostic): the lanes among those evaluated
 * at a point beyond the launch's eps bound (rmr_trail_rule.h); it must stay 0. */
int rmr_get_counters_n(rmr_ctx* ctx, uint64_t* out, int n);
/* Select kernel implementation (0 = persistent wavefront kernel, 1 = one launch-thread per path). */
int rmr_set_kernel(rmr_ctx* ctx, int kernel);
/* envTex of skyColor (RM1:78-113, RM2:84-107; the reference loads veranda_1k.hdr through SOIL as
 * an RGBA8 texture, Graphics.cpp:287): w x h RGBA8 texels, row 0 = texture coordinate t = 0 (the
 * direction +y). Used when params.use_env_tex != 0; NULL removes it. Sampling: bilinear, level 0,
 * CLAMP_TO_EDGE. */
int rmr_set_env_map(rmr_ctx* ctx, const uint8_t* rgba8, int w, int h);

/* ---- first-hit guides and the preview denoiser ------------------------------------------- */
/* No counterpart in the reference (its only output is the noisy running mean): the per-pixel geometry
 * of the first hit, and an edge-avoiding a-trous filter over the accumulator guided by it, for a
 * usable image after a few samples. Additive: nothing here changes a render's result. All of it runs
 * on the context's stream after the work queued before it, flushes held rmr_render calls first like
 * every other entry point, and works with a caller stream and a bound accumulator. The five W x H
 * float4 buffers (three guide planes, two filter images) are allocated at first use (RMR_E_NOMEM if
 * that fails) and freed by rmr_reload / rmr_destroy; a context that never calls these allocates none.
 *
 * Guide planes: W x H float4, row 0 = top, laid out like the accumulator. Each pixel's ray is main()'s
 * corner-ray interpolation at the pixel centre (u = px / W + 0.5 / W, v = py / H + 0.5 / H; no rand()),
 * marched with march(eye, dir, +1) under the context's max_dist / max_steps / step_multiply. A pixel
 * is a hit iff t < max_dist (a hit march() returns at t >= max_dist is a miss, as in trace()).
 *   RMR_GUIDE_RAY     (dir.xyz, 0)
 *   RMR_GUIDE_HIT     (pos.xyz, t), pos = fma(dir, t, eye), for hits and misses alike
 *   RMR_GUIDE_NORMAL  hit: (getNormal(pos).xyz, material id); miss: (0, 0, 0, -1) */
#define RMR_GUIDE_RAY 0
#define RMR_GUIDE_HIT 1
#define RMR_GUIDE_NORMAL 2
/* Render the guides of the integer rect [x0,x1) x [y0,y1) (clamped to the image); writes only inside
 * the rect. The guides become valid when one call covers the whole image; rmr_set_view, a scene load,
 * rmr_set_params and rmr_reload invalidate them. RMR_E_STATE without a scene. */
int rmr_render_guides(rmr_ctx* ctx, int x0, int y0, int x1, int y1);
/* One plane to the host (synchronises): what the rmr_render_guides calls so far wrote, zeros elsewhere.
 * RMR_E_STATE before the first rmr_render_guides since rmr_create / rmr_reload. */
int rmr_read_guide(rmr_ctx* ctx, int plane, float* rgba, size_t bytes);
/* Device pointer of a plane (allocates the planes if need be; NULL for a bad plane or on failure). */
void* rmr_guide_device_ptr(rmr_ctx* ctx, int plane);

/* Filter parameters. Pass i = 0 .. iterations-1 is the 5x5 B3-spline kernel (1/16, 1/4, 3/8, 1/4, 1/16)^2
 * with taps 2^i pixels apart; a tap q of a centre p weighs, besides the kernel,
 *   [id_q == id_p] * max(0, n_p.n_q)^(2^normal_pow2) * exp(-|n_p.(x_q - x_p)| / (sigma_z 2^i max(t_p, FLT_MIN)))
 *   * (sigma_c > 0 ? exp(-|c_q - c_p|^2 / (sigma_c 2^-i)^2) : 1),
 * the centre tap 1 exactly, a tap off the image or not live 0. A pixel is live iff its guide id >= 0,
 * its accumulator alpha != 0 and its current rgb is finite; a pixel that is not live (sky, not yet
 * rendered, NaN) passes through every pass bit for bit. Alpha is never changed. */
typedef struct rmr_denoise_params {
    int32_t iterations;  /* 5     0..8; 0 copies the accumulator                                  */
    int32_t normal_pow2; /* 5     0..7: squarings of the normal term (exponent 2^normal_pow2)      */
    float   sigma_z;     /* 0.02  finite, > 0: plane distance, relative to the centre's t and step */
    float   sigma_c;     /* 0     finite, >= 0: colour distance; 0 = term off                      */
} rmr_denoise_params;
void rmr_default_denoise_params(rmr_denoise_params* p);
/* Filter the accumulator into the context's denoised image (the accumulator is never written).
 * p NULL = the defaults; values outside the ranges above are RMR_E_INVALID. Renders full-image guides
 * first when they are not valid. The denoised image stays valid until a render call, rmr_write_accum /
 * rmr_load_accum, rmr_bind_accum, rmr_reload or anything that invalidates the guides. */
int rmr_denoise(rmr_ctx* ctx, const rmr_denoise_params* p);
/* The denoised image as RGBA32F (synchronises); RMR_E_STATE without a valid one. */
int rmr_read_denoised(rmr_ctx* ctx, float* rgba, size_t bytes);
/* Its device pointer (W x H float4; the next rmr_denoise may return another); NULL without a valid one. */
void* rmr_denoised_device_ptr(rmr_ctx* ctx);
/* What rmr_save_bmp / rmr_display / rmr_display_device read: the accumulator (default) or the denoised
 * image; with RMR_OUTPUT_DENOISED and no valid denoised image those calls return RMR_E_STATE. */
#define RMR_OUTPUT_ACCUM 0
#define RMR_OUTPUT_DENOISED 1
int rmr_set_output_source(rmr_ctx* ctx, int source);
/* Float image file from a host RGBA32F buffer (no context needed, like rmr_encode_bmp): a colour PFM
 * ("PF", RGB float32, scale -1.0 = little-endian, rows bottom to top; alpha is dropped). With
 * rmr_read_guide / rmr_read_accum / rmr_read_denoised the float output path for planes and HDR images. */
int rmr_encode_pfm(const float* rgba, int w, int h, const char* path);

/* ---- per-tile error estimate and adaptive sampling ----------------------------------------- */
/* No counterpart in the reference (it spends the same samples on every pixel). Additive: with the
 * estimate off every launch runs the kernels it ran before, and the accumulator's bits never depend on it.
 *
 * While the estimate is on, each launch's running-mean fold also maintains the half image B (W x H
 * float4, library-owned, laid out like the accumulator): a sample of odd global index n goes into B with
 * running-mean index n >> 1, so after samples 0..N-1 B is bitwise the render of seeds 1, 3, 5, ... alone
 * and its alpha is 1 where an odd sample has landed. B is allocated when the estimate is enabled (and
 * again by rmr_reload for a new size); rmr_reload zeroes it; the setting survives rmr_reload like the
 * params. The estimate is valid when it was enabled while nothing had been rendered since the last
 * rmr_reload (rmr_create counts as one); rmr_write_accum / rmr_load_accum / rmr_bind_accum, switching it
 * off, and rmr_trace_samples make it invalid until the next rmr_reload (or until it is enabled again on
 * an accumulator nothing has been rendered into). */
int rmr_set_error_estimate(rmr_ctx* ctx, int on);
/* B as RGBA32F (synchronises) and its device pointer (NULL while the estimate is off); RMR_E_STATE
 * while the estimate is off. */
int rmr_read_half_accum(rmr_ctx* ctx, float* rgba, size_t bytes);
void* rmr_half_device_ptr(rmr_ctx* ctx);
/* The tile errors, ceil(H / 8) x ceil(W / 8) floats row-major, to the host (synchronises). Tile (tx, ty)
 * covers pixels [8 tx, 8 tx + 8) x [8 ty, 8 ty + 8); with A the accumulator, every float32 operation
 * rounded on its own, a pixel inside the image contributes
 *   v = ((|A.r - B.r| + |A.g - B.g|) + |A.b - B.b|) / (offset + sqrt(max((A.r + A.g) + A.b, 0))),
 * v = 0 when any of A.rgb, B.rgb is not finite, and the tile's error is the pairwise-tree sum of its 64
 * lanes (pixels outside the image: 0) divided by its pixel count inside the image; +inf when a pixel of
 * the tile inside the image has A.a == 0 or B.a == 0 (fewer than two samples). RMR_E_STATE when the
 * estimate is not valid, RMR_E_INVALID unless offset is finite and > 0 and bytes covers the map. */
int rmr_tile_error(rmr_ctx* ctx, float offset, float* out, size_t bytes);
/* Test hook: the same kernel on two host images (w x h RGBA32F each) uploaded for the call; out:
 * ceil(h / 8) x ceil(w / 8) floats. Needs no scene and no valid estimate. */
int rmr_tile_error_images(rmr_ctx* ctx, const float* a_rgba, const float* b_rgba, int w, int h, float offset,
                          float* out);

/* Adaptive sampling: render until every decision block's error is at most `threshold`, at most
 * max_samples samples per pixel. */
typedef struct rmr_adaptive_params {
    float    threshold;     /* 0.1   finite, >= 0: a block is open while its error > threshold     */
    float    offset;        /* 1e-4  finite, > 0                                                   */
    uint32_t min_samples;   /* 16    >= 2: rendered everywhere before the first estimate           */
    uint32_t pass_samples;  /* 16    >= 1: samples per further pass on the open blocks             */
    uint32_t max_samples;   /* no default (0): the length of times[]; >= min_samples               */
    int32_t  block_tiles;   /* 2     1..8: a decision block is block_tiles x block_tiles 8x8 tiles */
} rmr_adaptive_params;
typedef struct rmr_adaptive_result {
    uint32_t passes;        /* render passes, the first included                                   */
    uint32_t tiles_open;    /* 8x8 tiles whose error is still > threshold at the stop              */
    uint64_t samples;       /* pixel samples rendered: sum of count x pixels inside the image      */
    float    max_error;     /* the largest tile error at the stop                                  */
} rmr_adaptive_result;
void rmr_default_adaptive_params(rmr_adaptive_params* p);
/* RMR_OK when every field is in its range, else RMR_E_INVALID (no context, no GPU). */
int rmr_check_adaptive_params(const rmr_adaptive_params* p);
/* Needs a scene and an accumulator nothing has been rendered into since rmr_reload (else RMR_E_STATE);
 * switches the estimate on. Samples [0, min_samples) go to the whole image; then, until no block is open
 * or max_samples is reached, the tile errors are read back, every open block whose largest tile error is
 * not > threshold closes for good, and the next min(pass_samples, max_samples - done) samples go to the
 * open blocks' tiles. Sample n is seeded with times[n] everywhere, so every pixel is bit for bit the
 * render of the first n seeds, n its tile's count (rmr_read_sample_counts). Runs on the context's stream
 * and synchronises once per pass. Continuing after the call returns is not supported. */
int rmr_render_adaptive(rmr_ctx* ctx, const float* times, const rmr_adaptive_params* p, rmr_adaptive_result* result);
/* Samples per 8x8 tile of the last rmr_render_adaptive since rmr_reload, ceil(H / 8) x ceil(W / 8)
 * row-major; RMR_E_STATE without one. */
int rmr_read_sample_counts(rmr_ctx* ctx, uint32_t* out, size_t bytes);
/* The decision rule alone (no context, no GPU): err is ty x tx tile errors, open_io one byte per decision
 * block, ceil(ty / block_tiles) x ceil(tx / block_tiles) row-major, non-zero = open. A block that is open
 * stays open iff one of its tiles has an error > threshold; a closed block stays closed. Returns the
 * number of blocks still open, or RMR_E_INVALID. */
int rmr_adaptive_select(const float* err, int tx, int ty, int block_tiles, float threshold, uint8_t* open_io);

/* ---- variance-guided mode of the preview denoiser ------------------------------------------ */
/* rmr_denoise's filter with one more edge-stopping weight, on luminance, scaled by a per-pixel variance
 * estimate taken from the accumulator A and the half image B: it backs off where the render has converged
 * and works hard where it has not. Additive: rmr_denoise and every other call compute what they did, and
 * a context that never calls rmr_denoise_variance allocates nothing for it.
 *
 * lum(v) = (0.2126 v.r + 0.7152 v.g) + 0.0722 v.b, always applied to a difference of two colours taken
 * per channel first. A pixel is v-live iff it is live in rmr_denoise's sense for A (guide id >= 0,
 * A.w != 0, A.rgb finite) and B.w != 0 and B.rgb is finite; this is settled once, from A and B. A pixel
 * that is not v-live (so also a live pixel with fewer than two samples) passes through every pass bit for
 * bit, contributes to no tap and no window, and has variance -1 in both variance planes.
 *   Seed: d(p) = lum(A(p).rgb - B(p).rgb); var_0(p) = sum_q d(q)^2 / n_p over the n_p pixels q with
 *     |dx|, |dy| <= var_radius that are on the image, v-live and have id_q == id_p (the centre is one).
 *     (A - B)^2 is an unbiased estimate of Var(A) for an even sample count n; for odd n it overestimates
 *     by at most 1 + 2 / (n - 1).
 *   Pass i = 0 .. iterations-1, step 2^i, c_0 = A: for a v-live centre p, w_q is rmr_denoise's tap weight
 *     (rmr_denoise_params above, "live" read as "v-live") times
 *       l_q = exp(-|lum(c_i(q).rgb - c_i(p).rgb)| / (sigma_l sqrt(max(var_i(p), 0)) + 1e-8)),
 *     the centre tap 1 exactly, and
 *       c_{i+1}(p).rgb = sum_q k_q w_q c_i(q).rgb / sum_q k_q w_q,     alpha unchanged,
 *       var_{i+1}(p)   = sum_q (k_q w_q)^2 var_i(q) / (sum_q k_q w_q)^2.
 *   iterations = 0 copies A, and the filtered variance is then the seed. */
typedef struct rmr_variance_params {
    float   sigma_l;     /* 4     finite, > 0: luminance distance in standard deviations           */
    int32_t var_radius;  /* 3     0..4: the seed's window is (2 var_radius + 1)^2 pixels           */
} rmr_variance_params;
void rmr_default_variance_params(rmr_variance_params* p);
/* RMR_OK when both fields are in their ranges, else RMR_E_INVALID (no context, no GPU). */
int rmr_check_variance_params(const rmr_variance_params* p);
/* Filter the accumulator into the context's denoised image, as rmr_denoise does and with its validity
 * rules: rmr_read_denoised, rmr_denoised_device_ptr, RMR_OUTPUT_DENOISED, rmr_save_bmp and rmr_display*
 * then read the guided image. NULL = the defaults, for either struct; RMR_E_INVALID outside the ranges.
 * RMR_E_STATE when the error estimate is not valid (it is valid when rmr_set_error_estimate was on before
 * the first render since rmr_reload, or after rmr_render_adaptive). Renders full-image guides first when
 * they are not valid (RMR_E_STATE under the equirect and ortho camera models). Three W x H float planes
 * (the seed and two filter planes) are allocated at the first call (RMR_E_NOMEM if that fails) and freed
 * with the guide planes by rmr_reload / rmr_destroy. The accumulator, B, the guides, the tile errors and
 * the sample counts are not written. Runs on the context's stream. */
int rmr_denoise_variance(rmr_ctx* ctx, const rmr_denoise_params* p, const rmr_variance_params* v);
/* The variance planes, W x H floats laid out like the accumulator: the seed var_0, and the filtered
 * variance var_iterations that belongs to the denoised image. Valid exactly while a denoised image made
 * by rmr_denoise_variance is valid (a later rmr_denoise makes them invalid), else RMR_E_STATE / NULL.
 * rmr_read_variance synchronises. */
#define RMR_VARIANCE_SEED 0
#define RMR_VARIANCE_FILTERED 1
int rmr_read_variance(rmr_ctx* ctx, int which, float* out, size_t bytes);
void* rmr_variance_device_ptr(rmr_ctx* ctx, int which);
/* Test hook: the same kernels on four host images (w x h RGBA32F each: A, B, RMR_GUIDE_HIT,
 * RMR_GUIDE_NORMAL) uploaded for the call; out_rgba: w x h RGBA32F, out_seed / out_var: w x h floats
 * (either may be NULL). Needs no scene, no valid estimate and no guides, and leaves every image of the
 * context as it was. */
int rmr_denoise_variance_images(rmr_ctx* ctx, const float* a_rgba, const float* b_rgba, const float* hit_rgba,
                                const float* nrm_rgba, int w, int h, const rmr_denoise_params* p,
                                const rmr_variance_params* v, float* out_rgba, float* out_seed, float* out_var);

/* ---- temporal reprojection of the preview across camera moves ------------------------------ */
/* No counterpart in the reference, whose setView starts again from noise. A history image (colour and
 * an effective sample count per pixel, with the guides and the view it was made with) is re-projected into
 * the current view through the current guides' hit points, validated against the history's own guides and
 * blended with the current frame by sample count. The scene is static between scene loads, so the previous
 * position of a surface point is a projection, not a motion-vector guess. Additive: no other entry point
 * computes anything else, and a context that never calls rmr_temporal_accumulate allocates nothing for it.
 *
 * S: the source image (accumulator or denoised image) with the caller's sample count n_cur; HIT, NORMAL:
 * the current guides; Hc, Hn, Hhit, Hnrm: the history's colour, count (0 = none) and guides; eye', r00',
 * r01', r10', r11': the history's view. Host, in double from the float view (rmr_temporal_view_inverse):
 *   a = r01' - r00', b = r10' - r00', c = (r11' - r10') - a, Minv = [a | b | r00']^-1, k = Minv c,
 * both rounded to float. The history's guide ray at image coordinates (u, v) is r00' + u a + v b + u v c
 * (primary_dir with both horizontal jitters equal); c = 0 for rmr_camera_view's views up to rounding.
 * Per pixel p, every float32 operation rounded on its own except where fma() is written:
 *  1. p is live iff its guide id >= 0, S.a != 0 and S.rgb is finite (rmr_denoise's rule). A pixel that is
 *     not live: out = S bit for bit, n_out = 0.
 *  2. x = HIT.xyz, n = NORMAL.xyz, id = NORMAL.w, t = HIT.w; d = x - eye';
 *       (U0, V0, w0)_i = fma(Minv_i0, d.x, fma(Minv_i1, d.y, Minv_i2 * d.z))
 *     lambda (r00' + u a + v b + u v c) = d with U = lambda u, V = lambda v, w = lambda reads
 *     (U, V, w) = (U0, V0, w0) - T k, T = U V / w: the root of A T^2 - B T + C = 0 next to C / B,
 *       A = fma(k0, k1, k2), B = fma(U0, k1, fma(V0, k0, w0)), C = U0 * V0
 *       T = C / B, then three times T = T - fma(fma(A, T, -B), T, C) / fma(A + A, T, -B)
 *       U = fma(-T, k0, U0), V = fma(-T, k1, V0), w = fma(-T, k2, w0)
 *       fx = (U / w) * W, fy = (V / w) * H              (pixel q's centre is at q + 0.5)
 *     No history for p when !(w > 0) or fx or fy is not finite.
 *     Accuracy: with e = 2^-24, a_i = sum_j |Minv_ij| |d_j|, K_i = |k_i| and, where |A C| <= B^2 / 16,
 *       Ta = (a_0 a_1 + |T| (a_2 + a_0 K_1 + a_1 K_0) + T^2 (K_0 K_1 + K_2)) / |B|
 *       |fx - fx*| <= 20 e W ((a_0 + K_0 Ta) + |U / w| (a_2 + K_2 Ta)) / w      (fy: a_1, K_1, V, H)
 *     against the exact solution fx* of the float view and hit point. Count: each product Minv_ij d_j
 *     carries 5 roundings (Minv, d, the product, two sums), B 8, C 11, A 3; the Newton steps correct
 *     themselves, so T carries the residual's 14 over |2 A T - B| >= 0.875 |B|: 16; U, V, w then 16 of
 *     their own terms; the two quotients' and the scale's roundings bring (16 + 2); 20 leaves room for the
 *     second-order terms. After the three steps the iteration's own error is below (1/16)^15.
 *  3. g = (fx, fy) - 0.5, q0 = floor(g), (tx, ty) = g - q0; the taps q = q0 + (i, j), i, j in {0, 1}, in
 *     the order (0,0) (1,0) (0,1) (1,1), b_q = (i ? tx : 1 - tx) * (j ? ty : 1 - ty). A tap counts iff it
 *     is on the image, Hn(q) > 0 and Hid(q) == id; its weight is g_q = b_q * (a_q z_q) with rmr_denoise's
 *       a_q = max(0, fma(n.x, n_q.x, fma(n.y, n_q.y, n.z * n_q.z))) squared normal_pow2 times
 *       z_q = exp(-|fma(n.x, x_q.x - x.x, fma(n.y, x_q.y - x.y, n.z * (x_q.z - x.z)))|
 *                 * min(1 / (sigma_z * max(t, FLT_MIN)), FLT_MAX))
 *     Every discrete test multiplies a b_q that is 0 where the tap set changes: the result is continuous
 *     in (fx, fy).
 *  4. G = sum g_q, h = (sum g_q Hc(q).rgb) / G (sums by fma(g_q, value, sum) in tap order),
 *     m = min(max_history, sum g_q Hn(q)) (not divided by G: a half-trusted history counts for half)
 *       out.rgb = (m * h + n_cur * S.rgb) / (m + n_cur), out.a = S.a, n_out = min(m + n_cur, max_history)
 *     No history, !(G > 0), !(m > 0) or h not finite: out = S bit for bit, n_out = min(n_cur, max_history). */
typedef struct rmr_temporal_params {
    float   max_history;  /* 64    finite, >= 1: cap of the effective sample count              */
    float   sigma_z;      /* 0.02  finite, > 0: plane distance, relative to the centre's t      */
    int32_t normal_pow2;  /* 5     0..7: squarings of the normal term                           */
} rmr_temporal_params;
void rmr_default_temporal_params(rmr_temporal_params* p);
/* RMR_OK when every field is in its range, else RMR_E_INVALID (no context, no GPU). */
int rmr_check_temporal_params(const rmr_temporal_params* p);
/* The host's part of the projection (no context, no GPU): out[0..8] = Minv row-major, out[9..11] = k, in
 * double, of view = eye', r00', r01', r10', r11'. RMR_E_INVALID for a view that is not finite, has a zero
 * corner ray or whose |det [a | b | r00']| <= 1e-9 |a| |b| |r00'| (corner rays coplanar with the eye). */
int rmr_temporal_view_inverse(const float view[15], double out[12]);
/* One step of the stage: S = the accumulator (source RMR_OUTPUT_ACCUM) or the valid denoised image
 * (RMR_OUTPUT_DENOISED; RMR_E_STATE without one), `samples` = n_cur, finite and > 0; p NULL = the defaults;
 * RMR_E_INVALID outside the ranges. Renders full-image guides first when they are not valid; RMR_E_STATE
 * under the equirect and ortho camera models and without a scene. The result becomes the new history (it
 * is written to the other of two buffer pairs, never in place), and the current guides (a device copy of
 * the two planes; rmr_guide_device_ptr keeps returning what it returned) and view become the history's.
 * With no history (the first call, after rmr_temporal_reset, a scene load or rmr_reload, or a history view
 * rmr_temporal_view_inverse refuses) every Hn is 0, so the call stores S with count min(samples,
 * max_history) (0 where the pixel is not live). rmr_set_view, rmr_set_params, a camera-model change and
 * rendering keep the history; rmr_reload also frees the stage's buffers (two colour, two count and two
 * guide planes, 72 bytes per pixel, allocated at the first call; RMR_E_NOMEM if that fails). The
 * accumulator, the guides, the denoised image and every other image of the context are not written. Runs on
 * the context's stream without synchronising, after flushing held rmr_render calls. */
int rmr_temporal_accumulate(rmr_ctx* ctx, int source, float samples, const rmr_temporal_params* p);
/* Drop the history (the buffers stay); RMR_OUTPUT_TEMPORAL has no valid image until the next step. */
int rmr_temporal_reset(rmr_ctx* ctx);
/* The temporal image as RGBA32F and its counts as W x H floats (both synchronise), and the image's device
 * pointer (the next step returns the other buffer); RMR_E_STATE / NULL without a valid one. */
int rmr_read_temporal(rmr_ctx* ctx, float* rgba, size_t bytes);
int rmr_read_temporal_count(rmr_ctx* ctx, float* out, size_t bytes);
void* rmr_temporal_device_ptr(rmr_ctx* ctx);
/* rmr_set_output_source: rmr_save_bmp / rmr_display* read the temporal image. Without a valid one
 * rmr_set_output_source(RMR_OUTPUT_TEMPORAL) returns RMR_E_STATE and leaves the source as it was, and those
 * calls return RMR_E_STATE when the image has become invalid since (rmr_temporal_reset, a scene load,
 * rmr_reload). */
#define RMR_OUTPUT_TEMPORAL 2
/* Test hook: the same kernel on host images uploaded for the call (w x h RGBA32F each, h_n w x h floats):
 * S, RMR_GUIDE_HIT, RMR_GUIDE_NORMAL of the current view, the history's colour, count and guides, and the
 * history's view. `view`, the current view, is not read (the hit points carry it) and may be NULL. out_n:
 * w x h floats; out_xy (may be NULL): w x h x 2 floats, (fx, fy) of step 2, NaN where the pixel is not
 * live or has no projection. Needs no scene and leaves every image of the context as it was.
 * RMR_E_INVALID for an h_view rmr_temporal_view_inverse refuses. Synchronises. */
int rmr_temporal_images(rmr_ctx* ctx, const float* s_rgba, const float* hit, const float* nrm, const float view[15],
                        const float* h_rgba, const float* h_n, const float* h_hit, const float* h_nrm,
                        const float h_view[15], int w, int h, float samples, const rmr_temporal_params* p,
                        float* out_rgba, float* out_n, float* out_xy);

/* ---- tone mapping and histogram auto-exposure ---------------------------------------------- */
/* No counterpart in the reference. Additive: with nothing below called, every other entry point reads
 * the planes it reads today. The stage scales an HDR image (the accumulator, the denoised or the
 * temporal image) by an exposure, applies a curve per colour channel and leaves the result, values in
 * [0, 1], in a W x H RGBA32F plane of its own, which rmr_save_bmp / rmr_display* then sRGB-encode as
 * they encode any other source. The exposure is given, or metered from the image's luminance histogram
 * on the GPU (no host round trip). DESIGN.md §4.13.
 *
 * The rule (csrc/rmr_tonemap_rule.h, compiled by the kernels and by the host functions below). Every
 * float operation is float32, each product and sum rounded on its own (no fused multiply-add); `/` is
 * the correctly rounded division.
 *
 * Luminance bin of a pixel (r, g, b, a):
 *   L = (0.2126f r + 0.7152f g) + 0.0722f b
 *   the pixel is counted when a != 0, r, g, b and L are finite and L >= 0; otherwise it is skipped.
 *   bin = clamp(((bits(L) & 0x7fffffff) >> 20) - ((127 - 16) << 3), 0, 255)   (the mask: L = -0 is bin 0)
 *   i.e. 8 bins per octave: bin b in 1..254 covers [2^e (1 + m/8), 2^e (1 + (m+1)/8)), e = (b >> 3) - 16,
 *   m = b & 7; bin 0 is everything below 2^-16 1.125 (zero and denormals included) and is never metered;
 *   bin 255 is everything from 2^15 1.875 up.
 * Metering (double, each operation rounded on its own), n_b = the counts of bins 1..255, N = their sum:
 *   lo = (double)low_pct N, hi = (double)high_pct N; C = 0, sw = 0, swl = 0; for b = 1..255 in order:
 *     w = max(0, min(C + n_b, hi) - max(C, lo)); swl += w lc_b; sw += w; C += n_b
 *   lc_b = e + log2(1 + (m + 0.5) / 8)                       (a table made on the host)
 *   l_target = (log2((double)key) - swl / sw) + (double)exposure_ev
 *   l = l_prev + (double)adapt (l_target - l_prev) with a valid previous state, else l = l_target
 *   N == 0: l = l_prev with a valid previous state, else (double)exposure_ev
 *   scale = (float)exp2(l); the state is (l, valid) from then on.
 * Curve, per colour channel c (alpha passes through):
 *   x = fmaxf(c scale, 0), a -0 product read as +0; so NaN gives 0
 *   RMR_TONE_LINEAR:   v = x
 *   RMR_TONE_REINHARD: v = (x (1 + x iw2)) / (1 + x), iw2 = (float)(1.0 / ((double)white white))
 *   RMR_TONE_ACES:     v = (x (2.51f x + 0.03f)) / (x (2.43f x + 0.59f) + 0.14f)      (Narkowicz's fit)
 *   result = fmaxf(fminf(v, 1), 0) with fminf's rule for NaN (the other operand): a channel so bright
 *   that v is inf / inf (+inf, or x^2 past FLT_MAX) gives 1, as every curve's limit is; v >= 0 otherwise. */
enum { RMR_TONE_LINEAR = 0, RMR_TONE_REINHARD = 1, RMR_TONE_ACES = 2 };
#define RMR_OUTPUT_TONEMAPPED 3
typedef struct rmr_tonemap_params {   /* 32 bytes */
    int32_t curve;          /* RMR_TONE_*;            default RMR_TONE_ACES */
    int32_t auto_exposure;  /* 0 / 1;                 default 0    */
    float exposure_ev;      /* finite, |ev| <= 32;    default 0    */
    float key;              /* finite > 0;            default 0.18 */
    float low_pct, high_pct;/* 0 <= low < high <= 1;  default 0.10, 0.90 */
    float adapt;            /* 0 < adapt <= 1;        default 1    */
    float white;            /* finite > 0;            default 4    */
} rmr_tonemap_params;
void rmr_default_tonemap_params(rmr_tonemap_params* p);
/* RMR_OK, or RMR_E_INVALID for a field outside the ranges above (NaN included) and for NULL. */
int rmr_check_tonemap_params(const rmr_tonemap_params* p);
/* The stage: source RMR_OUTPUT_ACCUM, RMR_OUTPUT_DENOISED or RMR_OUTPUT_TEMPORAL (anything else:
 * RMR_E_INVALID; a source with no valid image: RMR_E_STATE), p NULL = the defaults. With auto_exposure 0
 * scale = (float)exp2((double)exposure_ev), computed on the host; the meter does not run and the
 * adaptation state is left alone. With auto_exposure 1 the histogram, the meter and the curve run one
 * after the other on the GPU and the state becomes this call's l. The planes are allocated at the first
 * call (RMR_E_NOMEM, with nothing left allocated, when that fails). Queued on the context's stream
 * without synchronising, after flushing held rmr_render calls. The source image is not changed.
 * The tonemapped image is valid from then until any point where a denoised image would become invalid
 * (a render or rmr_write_accum, rmr_set_view, rmr_set_params, a scene load, rmr_reload, rmr_bind_accum,
 * rmr_denoise, rmr_denoise_variance), or, when it was made from the temporal image, until the next
 * rmr_temporal_accumulate. */
int rmr_tonemap(rmr_ctx* ctx, int source, const rmr_tonemap_params* p);
/* The tonemapped image as RGBA32F (synchronises) and its device pointer; RMR_E_STATE / NULL without a
 * valid one, never a stale image. */
int rmr_read_tonemapped(rmr_ctx* ctx, float* rgba, size_t bytes);
void* rmr_tonemapped_device_ptr(rmr_ctx* ctx);
/* What the last rmr_tonemap used: l (auto_exposure 0: (double)exposure_ev) and scale. Either pointer may be
 * NULL. RMR_E_STATE before the first rmr_tonemap (and after rmr_reload). Synchronises. */
int rmr_read_exposure(rmr_ctx* ctx, double* log2_scale, float* scale);
/* The luminance histogram of a source (as rmr_tonemap's), by the stage's own kernels: hist[b] = pixels in
 * bin b, *skipped (may be NULL) = pixels not counted; their sum is W H. Leaves the adaptation state and
 * the tonemapped image as they are. Synchronises. */
int rmr_luminance_histogram(rmr_ctx* ctx, int source, uint32_t hist[256], uint64_t* skipped);
/* Drop the adaptation state: the next auto-exposed rmr_tonemap uses its own l_target. rmr_set_image_size
 * and rmr_reload do the same. */
int rmr_tonemap_reset(rmr_ctx* ctx);
/* rmr_set_output_source(RMR_OUTPUT_TONEMAPPED): rmr_save_bmp / rmr_display* encode the tonemapped image.
 * Without a valid one the call returns RMR_E_STATE and leaves the source as it was, and those calls
 * return RMR_E_STATE when the image has become invalid since. */
/* Context-free, host only (no GPU needed): the rule above on host arrays.
 * bins[i] = the bin of pixel i of n RGBA pixels, -1: skipped. */
int rmr_luminance_bins(const float* rgba, size_t n, int32_t* bins);
/* *l_out = l of the metering rule for a histogram; l_prev NaN: no previous state (+-inf: RMR_E_INVALID).
 * p NULL = the defaults; RMR_E_INVALID for params rmr_check_tonemap_params refuses. */
int rmr_exposure_from_histogram(const uint32_t hist[256], const rmr_tonemap_params* p, double l_prev, double* l_out);
/* out = the curve p->curve (and p->white) of n RGBA pixels at `scale` (used as it is, whatever it is). */
int rmr_tonemap_pixels(const rmr_tonemap_params* p, float scale, const float* rgba, size_t n, float* out);

/* ---- HDR bloom ahead of tone mapping --------------------------------------------------------- */
/* No counterpart in the reference. Additive: with nothing below called, every other entry point reads
 * the planes it reads today. The stage spreads the part of an HDR image (the accumulator, the denoised
 * or the temporal image) above a threshold over a Gaussian-like pyramid, adds the spread part back to
 * the source and leaves the sum in a W x H RGBA32F plane of its own, RMR_OUTPUT_BLOOM, which rmr_tonemap,
 * rmr_luminance_histogram, rmr_save_bmp and rmr_display* read like any other source. The source image
 * is not written. DESIGN.md §4.14.
 *
 * The rule (csrc/rmr_bloom_rule.h, compiled by the kernels and by rmr_bloom_pixels). Every operation is
 * float32 and rounded on its own (no fused multiply-add); `/` is the correctly rounded division; every
 * select is a comparison.
 *
 * Sizes: w_0 = W, h_0 = H, w_k = (w_{k-1} + 1) >> 1, h_k likewise; a level may be 1 x 1.
 * Bright part P(p) of a source pixel (r, g, b, a):
 *   a == 0, or one of r, g, b not finite: the pixel is invalid and P = (0, 0, 0)
 *   c = (x > 0 ? x : +0) per channel        (either zero and every negative read as +0: P has no -0)
 *   L = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b;  L not finite: P = 0
 *   e = L - T;  !(e > 0): P = 0;  clamp > 0 and e > clamp: e = clamp
 *   f = e / L;  P = c f per channel
 * Down, one dimension, n values to m = (n + 1) >> 1, cl clamping an index to [0, n-1], i = 2j:
 *   d_j = ((a[cl(i-1)] + a[cl(i+2)]) + 3 (a[cl(i)] + a[cl(i+1)])) 0.125f
 * Down, two dimensions: along x of every row, then along y of the result.
 * Up, one dimension, m values to n, cl clamping to [0, m-1], j = i >> 1:
 *   u_i = (3 b[j] + b[cl(i odd ? j+1 : j-1)]) 0.25f
 * Up, two dimensions: along x, then along y.
 * Pyramid: B_1 = down(P(S)), B_k = down(B_{k-1}) for k = 2..N; U_N = B_N,
 *   U_k = B_k + s up(U_{k+1}) for k = N-1..1 (the product rounded, then the sum); G = up(U_1), W x H.
 *   gain = (float)((double)I / sum), sum = p_0 + p_1 + ... + p_{N-1} added in that order in double,
 *   p_0 = 1, p_j = p_{j-1} (double)s; computed on the host.
 * Result: a valid pixel gets out.rgb = S.rgb + gain G (the product rounded, then the sum) and out.a = S.a;
 * an invalid pixel is copied bit for bit. */
#define RMR_OUTPUT_BLOOM 4
typedef struct rmr_bloom_params {   /* 32 bytes */
    int32_t levels;         /* N, 1..8;               default 5   */
    float threshold;        /* T, finite >= 0;        default 1   */
    float clamp;            /* finite >= 0, 0 = off;  default 0   */
    float scatter;          /* s, 0 <= s <= 1;        default 0.7 */
    float intensity;        /* I, finite >= 0;        default 0.2 */
    int32_t reserved[3];    /* must be 0 */
} rmr_bloom_params;
void rmr_default_bloom_params(rmr_bloom_params* p);
/* RMR_OK, or RMR_E_INVALID for a field outside the ranges above (NaN included) and for NULL. */
int rmr_check_bloom_params(const rmr_bloom_params* p);
/* The stage: source RMR_OUTPUT_ACCUM, RMR_OUTPUT_DENOISED or RMR_OUTPUT_TEMPORAL (anything else,
 * RMR_OUTPUT_TONEMAPPED and RMR_OUTPUT_BLOOM included: RMR_E_INVALID; a source with no valid image:
 * RMR_E_STATE), p NULL = the defaults. The pyramid (about a third of a plane) and the result plane are
 * allocated at the first call, both or neither (RMR_E_NOMEM); rmr_reload (which is where a size given to
 * rmr_set_image_size takes effect) and rmr_destroy free them. Queued on the context's stream without synchronising, after flushing held
 * rmr_render calls.
 * The bloom image is valid from then until any point where a tonemapped image would become invalid (a
 * render, rmr_write_accum, rmr_bind_accum, rmr_set_view, rmr_set_params, a scene load, rmr_reload,
 * rmr_denoise, rmr_denoise_variance), or, when it was made from the temporal image, until the next
 * rmr_temporal_accumulate. A tonemapped image made from the bloom image becomes invalid when the bloom
 * image does, and at the next rmr_bloom; rmr_bloom leaves a tonemapped image of any other source and the
 * exposure adaptation state alone. */
int rmr_bloom(rmr_ctx* ctx, int source, const rmr_bloom_params* p);
/* The bloom image as RGBA32F (synchronises) and its device pointer; RMR_E_STATE / NULL without a valid
 * one, never a stale image. rmr_tonemap and rmr_luminance_histogram accept RMR_OUTPUT_BLOOM as a source
 * (RMR_E_STATE without a valid image); rmr_set_output_source(RMR_OUTPUT_BLOOM) is refused (RMR_E_STATE,
 * the source unchanged) while there is none, as RMR_OUTPUT_TONEMAPPED is. */
int rmr_read_bloom(rmr_ctx* ctx, float* rgba, size_t bytes);
void* rmr_bloom_device_ptr(rmr_ctx* ctx);
/* Context-free, host only (no GPU needed): the whole rule on a w x h RGBA32F host image; p NULL = the
 * defaults. RMR_E_INVALID for NULL images, w or h < 1 and params rmr_check_bloom_params refuses. */
int rmr_bloom_pixels(const rmr_bloom_params* p, const float* rgba, int w, int h, float* out);

/* ---- camera models and caller-supplied rays ------------------------------------------------ */
/* No counterpart in the reference, whose only camera is main()'s jittered interpolation of the four
 * corner rays from one point, the eye (RM1:569-584). Additive: with RMR_CAMERA_VIEW (the default) every
 * launch runs the kernels it ran before.
 *
 * A ray is trace()'s arguments and the state of the invocation's rand() chain when trace() starts:
 * origin o, unit direction d, the invocation (gx, gy) and seed `time` (rand()'s gl_GlobalInvocationID +
 * time terms), and rc, the chain value (randChange) at that point, 0 for a fresh chain. */
typedef struct rmr_ray {
    float   o[3], time;
    float   d[3], rc;
    int32_t gx, gy;
} rmr_ray;

/* With a model other than RMR_CAMERA_VIEW set, each launch of rmr_render / rmr_render_spp /
 * rmr_render_tiles / rmr_trace_samples / rmr_render_adaptive first writes one ray per pixel sample into a
 * device ray buffer (3 x 16 bytes per sample, counted against the per-launch plane budget of
 * rmr_set_tuning together with the sample's 16 bytes), then runs the ray-source form of the scene's trace
 * kernel on it, then the unchanged running-mean fold. Such launches take no launch streams
 * (rmr_set_launch_streams), are not call-batched (rmr_set_call_batching: rmr_render launches at once)
 * and run without lane slots, the once-per-wave eye step and batch probes; a pixel's samples do not
 * depend on how a frame is cut into launches.
 *
 * Every model starts a pixel sample's chain as main() does: rc = 0, seeds gxt = px + time, gyt =
 * py + time, rand(co) = the reference's rand() (RM1:49-56). All arithmetic is float32, each operation
 * rounded on its own except where fma() is written; sqrt is correctly rounded, sin / cos are the
 * kernels' own (oracle/detmath.h det_sin / det_cos). W, H: the image size. U, V, FWD: rmr_camera_frame
 * of the view. The first three calls are main()'s jitters:
 *   j1 = rand(gxt, gyt), j2 = rand(gxt, gyt), j3 = rand(gyt, gxt)
 *   dir0 = normalize(mix(mix(r00, r01, px / W + j1 / W), mix(r10, r11, px / W + j2 / W), py / H + j3 / H))
 *   u = px / W + j1 / W,  v = py / H + j3 / H
 * The ray's rc is the chain value after the model's last call.
 *
 * RMR_CAMERA_VIEW       o = eye, d = dir0 (computed inside the trace kernel: today's path).
 * RMR_CAMERA_THIN_LENS  aperture >= 0 (the lens radius), focus > 0, both finite.
 *     aperture == 0: o = eye, d = dir0, no further rand(): the same image as RMR_CAMERA_VIEW, bit for bit.
 *     aperture > 0:  r1 = rand(gxt, gyt), r2 = rand(gyt, gxt)
 *                    rad = sqrt(r1), phi = 6.28318548202514648438f * r2
 *                    lx = rad * cos(phi), ly = rad * sin(phi)
 *                    F = fma(dir0, focus, eye)          (the sphere of radius focus about the eye is sharp)
 *                    o = fma(V, aperture * ly, fma(U, aperture * lx, eye))
 *                    d = normalize(F - o)
 * RMR_CAMERA_EQUIRECT   a full panorama about the eye: image column = longitude about V (0 at FWD, towards
 *     U), row = polar angle from -V (row 0 is the top; V points down the image).
 *                    lon = 6.28318548202514648438f * (u - 0.5f), pol = 3.14159274101257324219f * v
 *                    a = sin(pol) * sin(lon), b = sin(pol) * cos(lon), m = -cos(pol)
 *                    o = eye, d = normalize(fma(U, a, fma(FWD, b, V * m)))
 * RMR_CAMERA_ORTHO      width, height > 0, finite: the extent of the image plane along U and V.
 *                    o = fma(V, (v - 0.5f) * height, fma(U, (u - 0.5f) * width, eye)), d = FWD
 * (fma(A, s, B) on vectors is componentwise; normalize(a) = a * (1 / sqrt(dot(a, a))) as in the kernels.) */
#define RMR_CAMERA_VIEW 0
#define RMR_CAMERA_THIN_LENS 1
#define RMR_CAMERA_EQUIRECT 2
#define RMR_CAMERA_ORTHO 3
typedef struct rmr_camera_model {
    int32_t model;      /* RMR_CAMERA_VIEW                                                       */
    float   aperture;   /* 0   RMR_CAMERA_THIN_LENS: lens radius, finite, >= 0                   */
    float   focus;      /* 1   RMR_CAMERA_THIN_LENS: focus distance from the eye, finite, > 0    */
    float   width;      /* 1   RMR_CAMERA_ORTHO: finite, > 0                                     */
    float   height;     /* 1   RMR_CAMERA_ORTHO: finite, > 0                                     */
} rmr_camera_model;
void rmr_default_camera_model(rmr_camera_model* m);
/* RMR_OK when the model is known and its own fields are in range (the other models' fields are not
 * looked at), else RMR_E_INVALID (no context, no GPU). */
int rmr_check_camera_model(const rmr_camera_model* m);
/* The setting survives rmr_reload, like the params. Setting a model flushes held rmr_render calls. */
int rmr_set_camera_model(rmr_ctx* ctx, const rmr_camera_model* m);
int rmr_get_camera_model(const rmr_ctx* ctx, rmr_camera_model* m);
/* The camera frame of a view (eye, ray00, ray01, ray10, ray11 in shader order, as rmr_set_view takes
 * them): out = U.xyz, V.xyz, FWD.xyz, orthonormal, computed in double and rounded to float. U along
 * ray01 - ray00 (the image's x); V along ray10 - ray00 made orthogonal to U (down the image); FWD along
 * ((ray00 + ray01) + ray10) + ray11 made orthogonal to both. RMR_E_INVALID for a view that is not finite
 * or whose U, V or FWD vanishes (below 1e-9 of the vector it is taken from). No context, no GPU. */
int rmr_camera_frame(const float view[15], float out[9]);
/* RMR_OK iff every float of every ray is finite, |d.d - 1| <= 1e-5 (in double) and 0 <= gx, gy < 2^24
 * (so that gx + time is one rounding); no context, no GPU. The work-skipping bounds of the kernels
 * (rmr_set_culling) assume unit directions to float precision, as normalize() gives for every bounce
 * ray: pass directions normalised in float or double, not merely within this check's 1e-5. */
int rmr_check_rays(const rmr_ray* rays, size_t n);
/* The radiance along each ray: out_rgba[i] = (trace(o, d).rgb, 1) of ray i, RGBA32F, with the loaded
 * scene, the params and the env map, bit for bit the reference's trace() for that invocation and chain
 * state. Any n >= 0 (the list's last 64-unit tile is padded with "no ray" records); the per-launch
 * plane budget cuts the list into launches (64 bytes per ray). Runs on the context's stream and
 * synchronises; the accumulator, the half image, the error estimate and the guides are left as they are.
 * RMR_E_INVALID for a list rmr_check_rays rejects; RMR_E_STATE without a scene and with
 * params.separate_channels set (a caller's ray has no channel passes: use three calls). */
int rmr_trace_rays(rmr_ctx* ctx, const rmr_ray* rays, size_t n, float* out_rgba);
/* The current model's rays (RMR_CAMERA_VIEW: the view's own) of samples seeded times[0 .. nspp) over the
 * integer rect [x0,x1) x [y0,y1) (clamped to the image; out is sized for the clamped rect), as
 * out[k][y - y0][x - x0], generated by the same kernel the render launches use. Synchronises. */
int rmr_camera_rays(rmr_ctx* ctx, const float* times, uint32_t nspp, int x0, int y0, int x1, int y1, rmr_ray* out);
/* rmr_render_guides / rmr_denoise under a model: unchanged for RMR_CAMERA_VIEW and RMR_CAMERA_THIN_LENS
 * (the guide ray is the lens centre's, i.e. the view's); RMR_E_STATE for RMR_CAMERA_EQUIRECT and
 * RMR_CAMERA_ORTHO. */

/* ---- first-hit and distance queries, device-resident lists -------------------------------- */
/* No counterpart in the reference. Additive: no other entry point changes.
 *
 * The first hit of a ray: the guide planes' HIT and NORMAL (rmr_render_guides) for one ray. */
typedef struct rmr_hit {
    float pos[3], t;
    float n[3], id;
} rmr_hit;
#define RMR_CAST_NORMALS 1
/* out[i] = the first hit of ray i: the guide pass's statement with the ray's origin o where the guide
 * pass has the eye, and its direction d. With maxDist, maxSteps, stepMultiply of the context's params:
 *   t = 0, id = -1; then up to maxSteps times: m = map(fma(d, t, o));
 *       if m.x < 0.001: the march ends with id = m.y
 *       else if t >= maxDist: it ends with t = maxDist
 *       else t = fma(m.x, stepMultiply, t)
 *   a march that falls out of the loop is (maxDist, -1).
 *   It is a hit iff t < maxDist (a far hit, an id found at t >= maxDist, is a miss that keeps march's t).
 *   pos = fma(d, t, o), for hits and misses alike.
 *   With RMR_CAST_NORMALS in flags, a hit gets n = getNormal(pos): the six probes map(pos +- 0.001 e_k)
 *   in the reference's order (+x, -x, +y, -y, +z, -z; the other two coordinates get +0 / -0 added, as
 *   the reference's vector sum does), n_k = plus_k - minus_k, then normalize. A miss gets n = (0, 0, 0)
 *   and id = -1. Without the flag n = (0, 0, 0), id is still given and no probe is evaluated (the
 *   visibility-query form).
 * The ray's time, rc, gx and gy are not used (but rmr_check_rays looks at them). map() is the scene's
 * table-driven map: no escape bound, no approximate map, no hipRTC kernel, so every kernel class gives
 * the same bits (those of the guide planes for the same ray). rays, out: host memory. Flushes held
 * rmr_render calls, runs on the context's stream and synchronises; the accumulator, the half image, the
 * error estimate, the guides and the denoised image are left as they are. The list is uploaded as it
 * is and checked on the GPU: RMR_E_INVALID, naming the first failing index, for a list rmr_check_rays
 * rejects (out is then not written) and for unknown flags; RMR_E_STATE without a scene. */
int rmr_cast_rays(rmr_ctx* ctx, const rmr_ray* rays, size_t n, int flags, rmr_hit* out);
/* out_dist_id[2 i], [2 i + 1] = map(xyz[3 i .. 3 i + 2]) as (distance, id): the fold over the scene's
 * primitives that starts from (maxDist, -1), as the reference's map() does. Points are not checked (a
 * NaN gives what map() gives). Host memory; state rules as rmr_cast_rays. */
int rmr_eval_map(rmr_ctx* ctx, const float* xyz, size_t n, float* out_dist_id);
/* The device forms: every pointer is device memory of the context's device (d_out_dist_id and d_xyz
 * float arrays, d_rays / d_out arrays of the structs, any 4-byte alignment). The work is queued on the
 * context's stream and the call returns without synchronising: order the producer of the inputs and the
 * consumer of the outputs against that stream (rmr_set_stream), as with a bound accumulator. Not
 * capturable into a graph: buffers are allocated at first use (and when a list outgrows them).
 * Nothing is validated on the host, so the rule moves to the GPU: a ray is rejected iff rmr_check_rays
 * would reject it, and for rmr_trace_rays_device also iff some |o_k| > origin_extent. A rejected ray's
 * result is (0, 0, 0, 0) for trace (alpha 0 marks it: every traced ray has alpha 1) and pos = 0, t = -1,
 * n = 0, id = -2 for cast; every other ray's result is what the host form gives, bit for bit. Each
 * rejected ray adds one to the context's counter (rmr_query_rejects).
 * origin_extent: the caller's bound on |origin coordinate| over the list, where rmr_trace_rays takes
 * the list's maximum (the inflation of the escape bound's boxes). The bound is exact work skipping, so
 * any value at least the true maximum gives the same bits; finite and >= 0, else RMR_E_INVALID.
 * rmr_trace_rays_device keeps rmr_trace_rays' plan (64 bytes per ray of the plane budget, launches of
 * whole 64-ray tiles), kernels and state rules: RMR_E_STATE without a scene and with
 * params.separate_channels, RMR_E_INVALID for n >= 2^37. */
int rmr_trace_rays_device(rmr_ctx* ctx, const rmr_ray* d_rays, size_t n, float origin_extent, float* d_out_rgba);
int rmr_cast_rays_device(rmr_ctx* ctx, const rmr_ray* d_rays, size_t n, int flags, rmr_hit* d_out);
int rmr_eval_map_device(rmr_ctx* ctx, const float* d_xyz, size_t n, float* d_out_dist_id);
/* *out = the rays the device forms rejected since the last call of it (or since rmr_create).
 * Synchronises the context's stream. */
int rmr_query_rejects(rmr_ctx* ctx, uint64_t* out);
/* Caps the grid of the cast and eval kernels at `blocks` workgroups of 256 threads (0, the default: one
 * thread per ray / point). A tuning knob like rmr_set_grid_reserve: scheduling only, results do not
 * depend on it. RMR_E_INVALID for blocks < 0. */
int rmr_set_query_grid(rmr_ctx* ctx, int blocks);

/* ---- sampled AOVs: coverage, depth, normal, position and id mattes per pixel ------------------ */
/* No counterpart in the reference. Additive: no other entry point changes.
 *
 * Per pixel, the first hits of the beauty samples' own primary rays, folded in sample order. Sample k
 * of a call is seeded times[k], as in rmr_render_spp, and its ray is the context's camera model's: bit
 * for bit what rmr_camera_rays returns and what the render of the same schedule traces first. Its hit is
 * rmr_cast_rays' with RMR_CAST_NORMALS (pos, t, n, id), bit for bit; id < 0 is a miss (a far hit, an id
 * found at t >= maxDist, is one).
 *
 * State: five W x H float4 planes (row 0 = top), 80 bytes per pixel.
 *   RMR_AOV_STATS     (n, h, sum_t, min_t)  samples folded, hits among them, sum and min of t over the hits
 *   RMR_AOV_NORMAL    (sum n.x, sum n.y, sum n.z, other)  other: hits whose id found no slot
 *   RMR_AOV_POSITION  (sum pos.x, sum pos.y, sum pos.z, 0)
 *   RMR_AOV_IDS01     (id0, c0, id1, c1)    four (material id, hit count) slots in the order the ids
 *   RMR_AOV_IDS23     (id2, c2, id3, c3)    were first seen
 * Initial state: every sum and count 0, min_t = +inf, every slot (-1, 0). Counts are float32, exact up
 * to 2^24.
 * Fold of one sample: n = n + 1; for a miss nothing else; for a hit h = h + 1, sum_t = sum_t + t,
 * min_t = (t < min_t ? t : min_t), each component of sum n and sum pos gets its addend (one float32
 * addition each, no fma); then the first slot j with id_j == id gets c_j = c_j + 1, else the first slot
 * with id_j == -1 becomes (id, 1), else other = other + 1. The state is a function of the pixel's hit
 * sequence alone: cutting a frame into calls, rects or launches does not change a bit of it.
 *
 * Resolve: five W x H float4 planes, float32, one IEEE operation per step:
 *   RMR_AOV_R_DEPTH     (mean_t, min_t, alpha, n): alpha = n > 0 ? h / n : 0; mean_t = h > 0 ? sum_t / h
 *                       : maxDist; min_t = h > 0 ? min_t : maxDist
 *   RMR_AOV_R_NORMAL    (N / len, alpha) with N = sum n, len = sqrt((N.x N.x + N.y N.y) + N.z N.z), each
 *                       component divided by len; (0, 0, 0, alpha) when h == 0 or len is 0 or not finite
 *   RMR_AOV_R_POSITION  (sum pos / h, h), each component divided by h; (0, 0, 0, 0) when h == 0
 *   RMR_AOV_R_IDS01, RMR_AOV_R_IDS23  the four slots sorted by count descending, then id ascending, each
 *                       as (id, c / n); empty slots stay (-1, 0) and sort last
 * maxDist: the context's params at the time of the resolve. */
#define RMR_AOV_STATS 0
#define RMR_AOV_NORMAL 1
#define RMR_AOV_POSITION 2
#define RMR_AOV_IDS01 3
#define RMR_AOV_IDS23 4
#define RMR_AOV_R_DEPTH 0
#define RMR_AOV_R_NORMAL 1
#define RMR_AOV_R_POSITION 2
#define RMR_AOV_R_IDS01 3
#define RMR_AOV_R_IDS23 4
/* Folds the nspp samples seeded times[0 .. nspp) into the pixels of the integer rect [x0,x1) x [y0,y1)
 * (clamped to the image; only pixels inside it are touched). restart != 0: the rect's pixels start from
 * the initial state. nspp == 0 with times null: only the restart, if any. Works under all four camera
 * models. Queued on the context's stream after the held rmr_render calls; does not synchronise. The
 * accumulator, the half image, the estimate, the guides and every output stage are left as they are.
 * The planes are allocated, in the initial state, at first use (RMR_E_NOMEM); rmr_reload, a scene load,
 * rmr_set_image_size and rmr_destroy free them; rmr_set_view, rmr_set_params and rmr_set_camera_model
 * keep them (the caller restarts, as with the accumulator).
 * RMR_E_STATE without a scene; RMR_E_INVALID for nspp == 0 with times non-null, nspp > 0 with times null,
 * and for a call that could take a pixel's n past 2^24 (counted as the samples of every call since the
 * last rmr_aov_reset or whole-image restart). */
int rmr_render_aov(rmr_ctx* ctx, const float* times, uint32_t nspp, int x0, int y0, int x1, int y1, int restart);
/* The initial state everywhere; the planes are kept (nothing to do while there are none). */
int rmr_aov_reset(rmr_ctx* ctx);
/* One raw state plane (RMR_AOV_*) / one resolved plane (RMR_AOV_R_*), W x H x 4 floats; synchronise.
 * RMR_E_STATE before the first rmr_render_aov since the planes were freed; RMR_E_INVALID for a bad
 * plane or bytes != W x H x 16. */
int rmr_read_aov(rmr_ctx* ctx, int plane, float* rgba, size_t bytes);
int rmr_read_aov_resolved(rmr_ctx* ctx, int which, float* rgba, size_t bytes);
/* The planes in device memory (null for a bad plane or a failed allocation). rmr_aov_device_ptr allocates
 * the state at first use. rmr_aov_resolved_device_ptr queues the resolve of the current state on the
 * context's stream (the resolved planes, 80 bytes per pixel more, are allocated at the first resolve) and
 * is null before the first rmr_render_aov; the pointer's contents are valid until the next rmr_render_aov
 * or rmr_aov_reset. No synchronisation. */
void* rmr_aov_device_ptr(rmr_ctx* ctx, int plane);
void* rmr_aov_resolved_device_ptr(rmr_ctx* ctx, int which);
/* A call is cut into launches of at most n samples each (default 6), so that a launch stays short on a
 * shared device. Scheduling only: the state does not depend on it. RMR_E_INVALID for n < 1. */
int rmr_set_aov_launch_samples(rmr_ctx* ctx, int n);
/* The rule on the host, no context and no GPU. state: [5][n_px][4] floats (the raw planes one after the
 * other); hits[k][pixel], rmr_hit as rmr_cast_rays gives them with RMR_CAST_NORMALS; out: [5][n_px][4].
 * rmr_aov_fold folds each pixel's nspp hits in the order k = 0, 1, ...; RMR_E_INVALID (nothing written)
 * if a pixel's n would pass 2^24. */
int rmr_aov_init(float* state, size_t n_px);
int rmr_aov_fold(float* state, const rmr_hit* hits, size_t n_px, uint32_t nspp);
int rmr_aov_resolve(const float* state, size_t n_px, float max_dist, float* out);

/* ---- SDF volume sampling and surface-nets mesh extraction ---------------------------------- */
/* No counterpart in the reference. Additive: no other entry point changes.
 *
 * A lattice of n[0] x n[1] x n[2] points. Point (ix, iy, iz) has the float32 coordinates
 *   origin[a] + (float)i_a * spacing       (the product rounded, then the sum rounded: no fused multiply-add)
 * and the linear index ix + n[0] * (iy + n[1] * iz), x fastest. */
typedef struct rmr_volume_desc {
    float origin[3];
    float spacing;
    int32_t n[3];
} rmr_volume_desc;
/* No context and no GPU. RMR_OK iff every number is finite, spacing > 0, 2 <= n[a] <= 4096 and the point
 * count is <= 2^30; otherwise RMR_E_INVALID, and *bad_field (when bad_field is not NULL) names the first
 * failing field: "origin", "spacing", "n" or "points" (a static string; NULL for RMR_OK, "desc" for a
 * NULL descriptor). */
int rmr_check_volume(const rmr_volume_desc* desc, const char** bad_field);
/* dist[k], id[k] = map(point k) as rmr_eval_map states it (the fold from (maxDist, -1); a NaN gives what
 * map() gives), by one kernel through the scene's table-driven map class that computes its points itself:
 * no point list, 4 bytes written per point, 8 with id. id may be NULL. Host memory, n[0] n[1] n[2] floats
 * each. State rules as rmr_cast_rays: flushes held rmr_render calls, runs on the context's stream and
 * synchronises; the accumulator, the half image, the estimate, the guides, every stage image, the sampled
 * AOVs and the reject counter are left as they are; rmr_set_query_grid caps its grid too. RMR_E_INVALID,
 * naming the field, for a descriptor rmr_check_volume rejects; RMR_E_STATE without a scene. */
int rmr_sample_volume(rmr_ctx* ctx, const rmr_volume_desc* desc, float* dist, float* id);
/* The same into device memory of the context's device, queued on the context's stream without
 * synchronising (as rmr_eval_map_device). */
int rmr_sample_volume_device(rmr_ctx* ctx, const rmr_volume_desc* desc, float* d_dist, float* d_id);

/* Surface nets over the sampled volume. With dist the lattice's distances and iso the level:
 *   A point is inside iff dist < iso (a NaN is outside, dist == iso is outside).
 *   A cell is the cube of 8 neighbouring points, at cell coordinates 0 .. n[a] - 2; it is active iff its
 *   corners are not all inside and not all outside. Each active cell has exactly one vertex; vertices are
 *   numbered in the order of the cells' linear index cx + (n[0] - 1) * (cy + (n[1] - 1) * cz).
 *   On a cell edge whose ends differ in inside-ness the crossing is t = (iso - d0) / (d1 - d0), from the
 *   lower end (d0) to the upper end (d1); a t that is not finite or outside [0, 1] is 0.5.
 *   The cell's 12 edges in order: axis a = x, y, z; with u = a + 1, v = a + 2 (cyclic) the edge at offsets
 *   (ou, ov) = (0, 0), (1, 0), (0, 1), (1, 1) on u and v. A crossing contributes t on axis a, ou on u and
 *   ov on v. s = the float32 sum of the contributions in that order, per axis; count = their number.
 *   vertex_a = (origin[a] + (float)c_a * spacing) + spacing * (s_a / (float)count).
 *   A lattice edge runs from point p along axis ax; with (ax, u, v) a cyclic permutation of (x, y, z) it is
 *   interior iff 1 <= p[u] <= n[u] - 2 and 1 <= p[v] <= n[v] - 2. An interior edge whose ends differ emits
 *   one quad (a boundary edge none: a surface that leaves the lattice is cut open there) of the vertices
 *   of the cells at (c[u], c[v]) = (p[u]-1, p[v]-1), (p[u], p[v]-1), (p[u], p[v]), (p[u]-1, p[v]), c[ax] =
 *   p[ax], in that order when the lower end is inside and in the reverse order otherwise: by the right-hand
 *   rule the quad's normal points from inside to outside. Quads are ordered by the linear index of the
 *   edge's lower point, then by axis x, y, z.
 *   RMR_MESH_NORMALS: normals[v] = getNormal(vertex v) as rmr_cast_rays states it (six probes, normalize);
 *   RMR_MESH_IDS: ids[v] = map(vertex v).y; both at the float32 vertex position, bit for bit what
 *   rmr_cast_rays / rmr_eval_map give there. */
#define RMR_MESH_NORMALS 1
#define RMR_MESH_IDS 2
typedef struct rmr_mesh_params {
    float iso;
    int32_t flags;   /* RMR_MESH_* */
} rmr_mesh_params;
typedef struct rmr_mesh_info {
    uint64_t n_vertices, n_quads;
} rmr_mesh_info;
/* Samples the lattice (as rmr_sample_volume_device, into memory of the library's) and extracts the mesh:
 * classify and count, an exclusive scan of the block totals (which alone decides every element's place: two
 * calls give the same bytes), then vertices, quads and attributes. Everything is queued on the context's
 * stream; the call synchronises once, after the scan, for the counts, sizes the mesh's buffers exactly and
 * queues the rest. The buffers belong to the library; the working memory (9 bytes per point and the
 * distances) is kept for the next extraction. State rules as rmr_sample_volume. RMR_E_INVALID for a bad
 * descriptor (naming the field), a non-finite iso, unknown flags and for 2^32 or more vertices or quads;
 * RMR_E_STATE without a scene; RMR_E_NOMEM when an allocation fails. After any error there is no mesh. */
int rmr_extract_mesh(rmr_ctx* ctx, const rmr_volume_desc* desc, const rmr_mesh_params* params, rmr_mesh_info* info);
/* The last extraction's mesh to host memory: vertices [n_vertices][3] floats, normals [n_vertices][3]
 * floats or NULL, ids [n_vertices] floats or NULL, quads [n_quads][4] uint32. Synchronises. RMR_E_STATE
 * before a valid extraction and for an attribute that was not extracted. */
int rmr_read_mesh(rmr_ctx* ctx, float* vertices, float* normals, float* ids, uint32_t* quads);
/* The mesh's device buffers (NULL: no mesh, not extracted, or empty); written by work queued on the
 * context's stream. No synchronisation. */
#define RMR_MESH_BUF_VERTICES 0
#define RMR_MESH_BUF_NORMALS 1
#define RMR_MESH_BUF_IDS 2
#define RMR_MESH_BUF_QUADS 3
void* rmr_mesh_device_ptr(rmr_ctx* ctx, int which);
/* Releases the mesh and the extraction's working memory (synchronises). The mesh lives until the next
 * rmr_extract_mesh, rmr_mesh_free, rmr_reload or rmr_destroy; a render, a view change or a parameter change
 * does not drop it. */
int rmr_mesh_free(rmr_ctx* ctx);
/* The same rule on a host volume, no context and no GPU, in count-then-fill form: *info always receives
 * the counts; with vertices and quads NULL nothing else happens; otherwise both are filled, or, where
 * vertex_cap (vertices) or quad_cap (quads) is too small, nothing is written and the result is
 * RMR_E_INVALID. RMR_E_INVALID also for a bad descriptor or a non-finite iso. */
int rmr_surface_nets(const float* dist, const rmr_volume_desc* desc, float iso, float* vertices, size_t vertex_cap,
                     uint32_t* quads, size_t quad_cap, rmr_mesh_info* info);
/* Wavefront OBJ: "v x y z" (9 significant digits: the float32 values read back exactly), with normals
 * "vn x y z" and faces "f a//a b//b c//c d//d", without them "f a b c d"; indices from 1. RMR_E_IO when
 * the file cannot be written, RMR_E_INVALID for an index >= n_vertices. */
int rmr_encode_obj(const char* path, const float* vertices, const float* normals, size_t n_vertices,
                   const uint32_t* quads, size_t n_quads);
/* PLY, binary little-endian: vertex properties float x y z, with normals float nx ny nz, with ids float
 * material; faces "list uchar uint vertex_indices" of 4. */
int rmr_encode_ply(const char* path, const float* vertices, const float* normals, const float* ids, size_t n_vertices,
                   const uint32_t* quads, size_t n_quads);

/* ---- light baking at surface points and mesh vertices --------------------------------------- */
/* No counterpart in the reference. Additive: no other entry point changes. DESIGN.md §4.17.
 *
 * For n points p_i with unit normals n_i (float32 [n][3] each) and the seeds times[0 .. nspp): the light
 * that reaches each point over the hemisphere about its normal, as the radiance a white Lambertian surface
 * would leave there (irradiance / pi) and / or as cosine-weighted ambient occlusion. Sample k of point i
 * is one ray; what it returns is the reference's trace() / march() bit for bit, and the samples of a point
 * are folded in ascending k, so the result does not depend on how the work is cut into launches.
 *
 * The rule (csrc/rmr_bake_rule.h holds the parts the host and the kernels share). All arithmetic is
 * float32, each operation rounded on its own except where fma() is written; `/` is the correctly rounded
 * division; every select is a comparison.
 *
 * Invocation: idx = first_index + i (idx < 2^36), gx = idx & 4095, gy = idx >> 12 (< 2^24, so that gy +
 *   time is one rounding): a 4096-wide image of points. first_index lets a caller bake a slice of a longer
 *   list and get the bits of the whole.
 * Reject: a point is rejected iff a coordinate of p or n is not finite or |n.n - 1| > 1e-6 (in double, each
 *   product and sum rounded on its own; tighter than rmr_check_rays' 1e-5, so that the generated directions
 *   are unit to float precision). Every output of a rejected point is 0, alpha included; it adds one to the
 *   counter rmr_query_rejects reads (once per call that takes the list, whatever the flags and nspp); the
 *   rays rmr_bake_rays_device generates for it carry gx = -1 (and gy = 0, o = d = 0, the sample's time).
 * Direction of sample k: a fresh chain (rc = 0) with the seeds gxt = gx + times[k], gyt = gy + times[k],
 *   started as main() starts a pixel's, with its first jitter call rand(gxt, gyt) (the value is not used);
 *   then d = randHemisphere((p.x, p.y), (p.z, p.x), m) as the kernels' hemisphere() (csrc/rmr_trace.h;
 *   RM1:270-304) states it: the seeds of the reference's diffuse bounce. (Without the first call the co of
 *   randHemisphere's first rand() would be (p.x, p.y) + (gxt, gyt) * 0: the same theta for every seed, all
 *   of a point's directions in one plane and a biased estimate. In the reference the three jitter calls of
 *   main() always precede a bounce.) m = n, except where n.x == 0 && n.z == 0: the
 *   reference's frame vanishes for every such n other than exactly (0, 1, 0) (a Cornell ceiling is one), so
 *   there m = (0, 1, 0), and d.y is negated if n.y < 0.
 * Ray: o = fma(n, bias, p) per component, direction d. The trace's own chain is again fresh: rc = 0 with the
 *   same seeds. It is NOT continued from the direction's three rand() calls: the oracle's trace entry starts
 *   at rc = 0 only, and the first rand() inside trace() has other `co` arguments (the first hit's
 *   coordinates, which move with d), so the two chains differ from their first value on.
 * Cosine: c_k = fma(n.z, d.z, fma(n.y, d.y, n.x * d.x)); c_k = c_k > 0 ? c_k : 0.
 * Radiance (RMR_BAKE_RADIANCE): L_k = trace(o, d).rgb as rmr_trace_rays_device gives it. A sample with a
 *   non-finite component of L_k is skipped. Over the used samples in ascending k: S = S + L_k * c_k per
 *   channel (the product rounded, then the sum: no fma). out.rgb = (S + S) / (float)n_used, out.a =
 *   (float)n_used; n_used == 0: rgb = 0. (The uniform hemisphere has pdf 1 / 2 pi, so this estimates
 *   irradiance / pi: under a constant sky of radiance L it is L itself.)
 * Occlusion (RMR_BAKE_AO): v_k = 0 iff the march of (o, d), as rmr_cast_rays states it (without normals:
 *   the table-driven map, so every kernel class gives the same bits), is a hit with t < ao_distance, else
 *   v_k = 1. ao = (sum c_k v_k) / (sum c_k), both sums in ascending k; a denominator of 0: ao = 1. */
#define RMR_BAKE_RADIANCE 1
#define RMR_BAKE_AO 2
typedef struct rmr_bake_params {   /* 24 bytes */
    int32_t flags;          /* RMR_BAKE_*, at least one;                      default RMR_BAKE_RADIANCE */
    float bias;             /* finite;                                        default 0.002             */
    float ao_distance;      /* > 0 or +inf (= the params' maxDist), not NaN;  default +inf              */
    float origin_extent;    /* the device forms: a bound on |o coordinate| over the list (as
                             * rmr_trace_rays_device's: finite, >= 0; any value at least the true maximum
                             * gives the same bits; a point whose ray origin exceeds it is rejected as
                             * well); the host forms compute it;               default 0                 */
    uint64_t first_index;   /* first_index + n <= 2^36;                       default 0                 */
} rmr_bake_params;
void rmr_default_bake_params(rmr_bake_params* p);
/* RMR_OK, or RMR_E_INVALID for a field outside the ranges above (origin_extent is not looked at) and NULL. */
int rmr_check_bake_params(const rmr_bake_params* p);
/* The reject rule on the host: RMR_OK iff no point is rejected; otherwise RMR_E_INVALID and *first_bad (when
 * not NULL) is the first rejected index (RMR_OK: n). No context, no GPU. */
int rmr_bake_check_points(const float* points, const float* normals, size_t n, size_t* first_bad);
/* The fold on host arrays laid out [k][i] (L_rgb [nspp][n][3], c and cv [nspp][n]): out_rgba [n][4] from L_rgb
 * and c, out_ao [n] from c and cv = c_k v_k; either output (with its inputs) may be NULL. No reject rule: every
 * point is used. RMR_E_INVALID for nspp == 0, nspp > 2^24 or a missing input. No context, no GPU. */
int rmr_bake_fold(const float* L_rgb, const float* c, const float* cv, size_t n, uint32_t nspp, float* out_rgba,
                  float* out_ao);
/* out[3 i + k] = the display's exact sRGB encode (rmr_display, rmr_srgb_thresholds) of rgb[3 i + k]: the number
 * of thresholds <= the value (a NaN: 0). No context, no GPU. */
int rmr_srgb8_pixels(const float* rgb, size_t n, uint8_t* out);
/* rmr_encode_ply with "property uchar red / green / blue" (rgb8 [n_vertices][3]) after the other vertex
 * properties; rgb8 NULL writes rmr_encode_ply's file. */
int rmr_encode_ply_colors(const char* path, const float* vertices, const float* normals, const float* ids,
                          const uint8_t* rgb8, size_t n_vertices, const uint32_t* quads, size_t n_quads);
/* The bake of a host list: out_rgba [n][4] with RMR_BAKE_RADIANCE, out_ao [n] with RMR_BAKE_AO (the other may
 * be NULL). params NULL = the defaults; origin_extent is taken from the list. Runs on the context's stream and
 * synchronises. A bake is a render over a 1-D image of points: a tile is 64 consecutive points, a sample is k,
 * and the per-launch plane budget (rmr_set_tuning, 64 bytes per ray) cuts the tile-samples into launches of
 * the ray-source trace kernel (the scene-specialised one under rmr_set_jit's rule), within a point's sample
 * set and within the point list alike; there are no launch slots. Occlusion launches hold 8 bytes per ray and
 * rmr_set_query_grid caps their grid. State rules as rmr_trace_rays_device: RMR_E_STATE without a scene and
 * with params.separate_channels; the accumulator, the half image, the estimate, the guides, every stage image,
 * the sampled AOVs and the mesh are left as they are. RMR_E_INVALID for params rmr_check_bake_params refuses,
 * nspp == 0, nspp > 2^24, first_index + n > 2^36 and ceil(n / 64) nspp >= 2^32. */
int rmr_bake_points(rmr_ctx* ctx, const float* points, const float* normals, size_t n, const float* times,
                    uint32_t nspp, const rmr_bake_params* params, float* out_rgba, float* out_ao);
/* The same with device pointers (any 4-byte alignment; times stays a host array), queued on the context's
 * stream without synchronising, as the other device forms; params->origin_extent is required (RMR_E_INVALID
 * unless finite and >= 0). The per-point state between launches (16 bytes per point) is the library's. */
int rmr_bake_points_device(rmr_ctx* ctx, const float* d_points, const float* d_normals, size_t n, const float* times,
                           uint32_t nspp, const rmr_bake_params* params, float* d_out_rgba, float* d_out_ao);
/* The generated rays as d_out[k][i] (device memory, n nspp rays), for rmr_cast_rays_device,
 * rmr_trace_rays_device or a caller's own use; flags, ao_distance and origin_extent are not used. Needs no
 * scene. Queued on the context's stream without synchronising. */
int rmr_bake_rays_device(rmr_ctx* ctx, const float* d_points, const float* d_normals, size_t n, const float* times,
                         uint32_t nspp, const rmr_bake_params* params, rmr_ray* d_out);
/* The bake at the last extraction's vertices and normals (RMR_E_STATE without a mesh or without
 * RMR_MESH_NORMALS), as rmr_bake_points_device with origin_extent taken from the lattice's box: its largest
 * |coordinate| plus twice |bias|, times 1 + 2^-20, rounded up to the next float (any bound at least the true one
 * gives the same bits).
 * The results go to buffers that live and die with the mesh: colours [V][4] (RMR_BAKE_RADIANCE) and ao [V]
 * (RMR_BAKE_AO); a second bake replaces what its flags name. No synchronisation.
 * Surface-nets vertices lie off the surface by a fraction of a cell, inside a convex shape (on a unit sphere
 * at spacing 3 / 16 by up to 0.065 of the spacing): with a bias below that every ray of such a vertex starts
 * inside the shape, where the march ends at once. rmr_cli --mesh-bake uses 0.002 + spacing / 8. */
int rmr_bake_mesh(rmr_ctx* ctx, const float* times, uint32_t nspp, const rmr_bake_params* params);
/* The mesh's bake to host memory (either may be NULL); synchronises. RMR_E_STATE for what was not baked. */
int rmr_read_mesh_bake(rmr_ctx* ctx, float* rgba, float* ao);
#define RMR_MESH_BAKE_RGBA 0
#define RMR_MESH_BAKE_AO 1
/* Their device pointers (NULL: no mesh, not baked, or empty). No synchronisation. */
void* rmr_mesh_bake_device_ptr(rmr_ctx* ctx, int which);

/* ---- irradiance probes: SH light baking on a lattice and its lookup ----------------------------- */
/* No counterpart in the reference. Additive: no other entry point changes. DESIGN.md §4.18.
 *
 * The companion of the vertex bake for what moves through a scene: radiance over the whole sphere is sampled
 * at probe points and projected onto nine spherical-harmonic functions per colour channel; irradiance / pi for
 * any position and normal is then looked up by trilinear interpolation over a lattice of probes. This lookup has
 * no visibility or back-face weights: light leaks through walls thinner than a cell (rmr_probe_irradiance_vis,
 * below, is the lookup with them).
 *
 * The rule (csrc/rmr_probe_rule.h holds the parts the host and the kernels share). All arithmetic is float32,
 * each operation rounded on its own (no fma); `/` is the correctly rounded division; every select is a
 * comparison.
 *
 * Probes: a probe is a point p. The list form takes n points (float32 [n][3]) and first_index; its invocation
 *   is the bake's: idx = first_index + i (idx < 2^36), gx = idx & 4095, gy = idx >> 12. The field form takes an
 *   lattice descriptor that rmr_check_volume accepts; probe j is lattice point j by that header's position rule and linear
 *   index, and first_index is 0.
 * Reject: a probe is rejected iff a coordinate of p is not finite or, in the device forms, |p coordinate| >
 *   origin_extent. Rejects are counted once per call into the counter rmr_query_rejects reads.
 * Buried: a probe is buried iff !(map(p).x >= clearance), map as rmr_eval_map states it (the table-driven map
 *   class, so every kernel class gives the same bits); a NaN distance buries the probe. Buried probes are not
 *   counted. Rejected and buried probes trace nothing; all 28 of their outputs are 0.
 * Sample k of a used probe: a fresh chain (rc = 0) with the seeds gxt = gx + times[k], gyt = gy + times[k],
 *   started with main()'s first jitter call rand(gxt, gyt) (the value is not used; rmr_bake_points has the
 *   reason); then d = randHemisphere((p.x, p.y), (p.z, p.x), (0, 0, 0)): the zero-normal branch, a uniform
 *   direction on the sphere (the reference's volume-scatter path). The ray is (o = p, d); the trace's own
 *   chain is fresh again (rc = 0, the same seeds). L_k = trace(o, d).rgb as rmr_trace_rays_device gives it. A
 *   sample with a non-finite component of L_k is skipped.
 * Basis of a unit vector (x, y, z):
 *   Y0 = 0.282095f              Y1 = 0.488603f * y          Y2 = 0.488603f * z          Y3 = 0.488603f * x
 *   Y4 = 1.092548f * (x * y)    Y5 = 1.092548f * (y * z)    Y6 = 0.315392f * ((3.0f * (z * z)) - 1.0f)
 *   Y7 = 1.092548f * (x * z)    Y8 = 0.546274f * ((x * x) - (y * y))
 * Fold: over the used samples in ascending k, for m = 0..8 and channel c: S[m][c] = S[m][c] + (L_k[c] *
 *   Y_m(d_k)), the product rounded, then the sum. n_used counts the used samples (float32, exact up to 2^24).
 *   sh[m][c] = (S[m][c] * 12.566371f) / n_used; n_used == 0: everything 0. A probe's output is 28 floats:
 *   sh[9][3], then n_used. A probe is valid iff n_used > 0. Each coefficient meets its samples in ascending k,
 *   so the result does not depend on how the work is cut into launches or mapped to threads.
 * Lookup: a lattice desc, its field sh[n][28], a point q and a unit normal nrm; a query is rejected as
 *   rmr_bake_check_points rejects a point (result (0, 0, 0, 0), counted). Per axis a: f_a = (q_a - origin_a) /
 *   spacing; c_a = floor(f_a) clamped to [0, n_a - 2] (as a float, then converted); w_a = f_a - (float)c_a
 *   clamped to [0, 1]: a point outside the box takes the boundary's value. The cell's eight corners in the
 *   order dx + 2 dy + 4 dz: u_a = d_a ? w_a : 1 - w_a; g = (u_x * u_y) * u_z, or 0 if that probe is not valid;
 *   W = the sum of g in corner order; B[m][c] = the sum of g * sh[m][c] in corner order (each product rounded,
 *   then each sum). With Y_m = Y_m(nrm), per channel: t0 = B0 * Y0; t1 = (((B1 * Y1) + (B2 * Y2)) + (B3 * Y3))
 *   * 0.6666667f; t2 = (((((B4 * Y4) + (B5 * Y5)) + (B6 * Y6)) + (B7 * Y7)) + (B8 * Y8)) * 0.25f; e = (t0 +
 *   t1) + t2; v = e / W; out.rgb = W > 0 ? (v > 0 ? v : 0) : 0 and out.a = W. (1, 2/3 and 1/4 are the
 *   clamped-cosine lobe's band factors over pi: the output has rmr_bake_points' unit, irradiance / pi; under a
 *   constant radiance L it is L.) */
typedef struct rmr_probe_params {   /* 16 bytes */
    float clearance;        /* finite, >= 0;                                   default 0 */
    float origin_extent;    /* the device list forms: a bound on |p coordinate| (finite, >= 0; a probe beyond
                             * it is rejected); the host and field forms compute it;  default 0 */
    uint64_t first_index;   /* first_index + n <= 2^36; the field form: 0;      default 0 */
} rmr_probe_params;
void rmr_default_probe_params(rmr_probe_params* p);
/* RMR_OK, or RMR_E_INVALID for a field outside the ranges above (origin_extent is not looked at) and NULL. */
int rmr_check_probe_params(const rmr_probe_params* p);
/* out[i][0 .. 9) = Y_0 .. Y_8 of dirs[i] (float32 [n][3]; not normalised, not checked). No context, no GPU. */
int rmr_sh_basis(const float* dirs, size_t n, float* out);
/* The fold and resolve on host arrays laid out [k][i] (L_rgb and dirs [nspp][n][3]): out [n][28]. No reject or
 * buried rule: every probe is used. RMR_E_INVALID for nspp == 0, nspp > 2^24 or a missing array. No context,
 * no GPU. */
int rmr_probe_fold(const float* L_rgb, const float* dirs, size_t n, uint32_t nspp, float* out);
/* The lookup on the host: out_rgba [n][4] over the field sh [points of desc][28]. Every query's result is
 * written; RMR_OK iff no query is rejected, otherwise RMR_E_INVALID and *first_bad (when not NULL) is the first
 * rejected index (RMR_OK: n). RMR_E_INVALID, nothing written, for a descriptor rmr_check_volume rejects or a
 * missing array. No context, no GPU. */
int rmr_probe_irradiance_host(const rmr_volume_desc* desc, const float* sh, const float* points, const float* normals,
                              size_t n, float* out_rgba, size_t* first_bad);
/* The generated rays as d_out[k][i] (device memory, n nspp rays), for rmr_trace_rays_device or a caller's own
 * use. A rejected or buried probe's rays: gx = -1, the sample's time, everything else 0 (rmr_bake_rays_device's
 * convention). origin_extent is not used (no bound). Needs a scene (the buried test): RMR_E_STATE without one.
 * Queued on the context's stream without synchronising. */
int rmr_probe_rays_device(rmr_ctx* ctx, const float* d_points, size_t n, const float* times, uint32_t nspp,
                          const rmr_probe_params* params, rmr_ray* d_out);
/* The bake of a host list: out_sh [n][28]. params NULL = the defaults; origin_extent is taken from the list.
 * Runs on the context's stream and synchronises. State rules, error codes, limits and the cut into launches
 * are rmr_bake_points': RMR_E_STATE without a scene and with params.separate_channels; RMR_E_INVALID for params
 * rmr_check_probe_params refuses, nspp == 0, nspp > 2^24, first_index + n > 2^36 and ceil(n / 64) nspp >= 2^32.
 * The accumulator, the half image, the estimate, the guides, every stage image, the sampled AOVs, the mesh and
 * its bake are left as they are (by every function of this section). */
int rmr_bake_probes(rmr_ctx* ctx, const float* points, size_t n, const float* times, uint32_t nspp,
                    const rmr_probe_params* params, float* out_sh);
/* The same with device pointers (times stays a host array), queued on the context's stream without
 * synchronising; params->origin_extent is required (RMR_E_INVALID unless finite and >= 0). The per-probe state
 * between launches (144 bytes per probe: a float4 per coefficient) is the library's. */
int rmr_bake_probes_device(rmr_ctx* ctx, const float* d_points, size_t n, const float* times, uint32_t nspp,
                           const rmr_probe_params* params, float* d_out_sh);
/* The field, owned by the context: one lattice and its [points][28] floats in device memory. It is freed by
 * rmr_probe_field_free, rmr_reload and rmr_destroy; before a field exists the readers and the lookup return
 * RMR_E_STATE (rmr_probe_field_device_ptr: NULL).
 * rmr_bake_probe_field bakes the lattice's points (as rmr_bake_probes_device over them with first_index 0; the
 * extent is the lattice box's largest |coordinate| times 1 + 2^-20, rounded up; params->first_index must be 0)
 * and replaces the field; no synchronisation. RMR_E_INVALID, naming the field, for a descriptor
 * rmr_check_volume rejects. */
int rmr_bake_probe_field(rmr_ctx* ctx, const rmr_volume_desc* desc, const float* times, uint32_t nspp,
                         const rmr_probe_params* params);
/* Loads a saved or synthetic field (sh: host memory, [points of desc][28]); replaces the field; synchronises.
 * Needs no scene. */
int rmr_write_probe_field(rmr_ctx* ctx, const rmr_volume_desc* desc, const float* sh);
/* The field's lattice and / or floats to host memory (either may be NULL); synchronises. */
int rmr_read_probe_field(rmr_ctx* ctx, rmr_volume_desc* desc_out, float* sh);
void* rmr_probe_field_device_ptr(rmr_ctx* ctx);
int rmr_probe_field_free(rmr_ctx* ctx);
/* The lookup over the context's field: out_rgba [n][4] for n points and unit normals (float32 [n][3] each). The
 * host form copies, runs on the context's stream and synchronises; the device form is queued without
 * synchronising. Rejected queries are counted (rmr_query_rejects). Needs no scene. */
int rmr_probe_irradiance(rmr_ctx* ctx, const float* points, const float* normals, size_t n, float* out_rgba);
int rmr_probe_irradiance_device(rmr_ctx* ctx, const float* d_points, const float* d_normals, size_t n, float* d_out_rgba);

/* -- the probes' visibility: octahedral depth moments per probe, and the lookup weighted by them -- */
/* No counterpart in the reference. Additive: rmr_probe_irradiance, the probe bake, the field and its file are as
 * they were; this is a second lookup over the same field. DESIGN.md §4.19.
 *
 * rmr_probe_irradiance blends a cell's eight probes by position alone, so light leaks through a wall thinner
 * than a cell. Here each probe also holds a small map of how far it sees, and the lookup weighs a corner down
 * when the point lies behind what that probe sees (a Chebyshev bound on the two moments of distance) or faces
 * away from it.
 *
 * The rule (csrc/rmr_probe_vis_rule.h holds the parts the host and the kernels share). As above: float32, each
 * operation rounded on its own (no fma), `/` and sqrt correctly rounded, every select a comparison. |x| is
 * x < 0 ? -x : x and sgn(x) is x >= 0 ? 1 : -1.
 *
 * The map: 8 x 8 texels per probe, two floats (m1, m2) per texel: vis[64][2], 128 floats. Texel j = iy * 8 +
 *   ix has the direction D_j, the octahedral decode of its centre: u = (((float)ix + 0.5) / 8) * 2 - 1, v
 *   likewise from iy (all exact); n = (u, v, (1 - |u|) - |v|); for n.z < 0: n.x = (1 - |v|) * sgn(u) and n.y =
 *   (1 - |u|) * sgn(v); len = sqrt(((n.x * n.x) + (n.y * n.y)) + (n.z * n.z)); D_j = (n.x / len, n.y / len,
 *   n.z / len). The poles are +-z.
 * Samples: sample k of probe i has the direction d_k of rmr_bake_probes (the same invocation, seeds, first
 *   jitter call and zero-normal randHemisphere), and the distance t_k = the t of rmr_cast_rays' march for the
 *   ray (o = p, d_k) without RMR_CAST_NORMALS (maxDist, maxSteps and stepMultiply from the context's params;
 *   the ray is not put through rmr_check_rays). A sample whose t_k is not finite is skipped; otherwise r_k =
 *   t_k < range ? t_k : range. range is finite and > 0.
 * Fold, for texel j over the samples in ascending k: c = ((D.x * d.x) + (D.y * d.y)) + (D.z * d.z); if
 *   !(c > 0) the sample does not touch the texel; otherwise c2 = c * c, c4 = c2 * c2, c8 = c4 * c4, c16 = c8 *
 *   c8, w = c16 * c16 (c^32; no powf); A = A + w; M1 = M1 + (w * r); M2 = M2 + (w * (r * r)).
 *   Resolve: A > 0: m1 = M1 / A and m2 = M2 / A; otherwise m1 = range and m2 = range * range (a texel nobody
 *   sampled sees as far as the range). Each texel meets its samples in ascending k as one sequential sum, so
 *   neither the cut into launches nor the mapping to threads changes a bit.
 * Which probes: the list forms use rmr_probe_params and the probe bake's reject and buried rules; a rejected or
 *   buried probe casts nothing and all 128 of its floats are 0; rejects are counted as in the probe bake. The
 *   field form bakes for the context's field: probe j is used iff it is valid there (sh[j][27] > 0; no buried
 *   test of its own); every other probe gets 128 zeros.
 * Lookup: the cell, the factors g0 = (u_x * u_y) * u_z, the corner order, the SH resolve and the reject rule
 *   are rmr_probe_irradiance's. bias is finite and >= 0. qb_a = q_a + (bias * nrm_a). Per corner with a valid
 *   probe, at P = the lattice position of the corner's indices (origin_a + ((float)index_a * spacing)):
 *   v = qb - P; r = sqrt(((v.x * v.x) + (v.y * v.y)) + (v.z * v.z)).
 *   r == 0: wb = 1 and wv = 1. Otherwise:
 *   back face: dn = ((v.x * nrm.x) + (v.y * nrm.y)) + (v.z * nrm.z); b = (-dn) / r (the cosine between the
 *     normal and the direction from the point to the probe); h = (b + 1) * 0.5; wb = (h * h) + 0.2f.
 *   visibility: dir = (v.x / r, v.y / r, v.z / r). Its texel under the octahedral encode: s = (|x| + |y|) +
 *     |z|; ox = x / s; oy = y / s; for z < 0 (so z = -0 is the upper half): (ox, oy) = ((1 - |oy|) * sgn(x),
 *     (1 - |ox|) * sgn(y)), both from the old values; per axis f = floor(((o * 0.5) + 0.5) * 8); f = f > 0 ? f
 *     : 0; f = f < 7 ? f : 7 (a NaN gives 0); ix = (int)f from ox, iy from oy. (m1, m2) = vis[iy * 8 + ix].
 *     r <= m1: wv = 1. Otherwise var = |m2 - (m1 * m1)|; dl = r - m1; ch = var / (var + (dl * dl)); wv = (ch *
 *     ch) * ch; wv < 0.05f: wv = 0.05f (the floor keeps a point that every probe calls occluded from dividing
 *     by nothing).
 *   g = (g0 * wb) * wv, or 0 for a probe that is not valid. W, B, the SH resolve, the clamp at 0 and out.a = W
 *   follow as in rmr_probe_irradiance. */
/* out[j] = D_j. RMR_E_INVALID for NULL. No context, no GPU. */
int rmr_probe_vis_dirs(float out[64][3]);
/* The fold and resolve on host arrays laid out [k][i]: d_and_t [nspp][n][4] = (d.xyz, t); out [n][128]. No reject
 * or buried rule: every probe is used. RMR_E_INVALID for nspp == 0, nspp > 2^24, a range that is not finite and
 * > 0, or a missing array. No context, no GPU. */
int rmr_probe_vis_fold(const float* d_and_t, size_t n, uint32_t nspp, float range, float* out);
/* The lookup on the host over sh [points of desc][28] and vis [points of desc][128]; results, return value and
 * *first_bad as rmr_probe_irradiance_host's; also RMR_E_INVALID, nothing written, for a bias that is not finite
 * and >= 0. No context, no GPU. */
int rmr_probe_irradiance_vis_host(const rmr_volume_desc* desc, const float* sh, const float* vis, const float* points,
                                  const float* normals, size_t n, float bias, float* out_rgba, size_t* first_bad);
/* The maps of a host list of probes: out_vis [n][128]. Runs on the context's stream and synchronises. State
 * rules, error codes and limits are rmr_bake_probes', except that params.separate_channels does not matter:
 * nothing is traced. Also RMR_E_INVALID for a range that is not finite and > 0. The samples are cut into runs
 * of k under rmr_set_tuning's samp_budget at 16 bytes per (probe, sample); the running sums between launches
 * (768 bytes per probe) are the library's. */
int rmr_bake_probe_visibility(rmr_ctx* ctx, const float* points, size_t n, const float* times, uint32_t nspp,
                              const rmr_probe_params* params, float range, float* out_vis);
/* The same with device pointers (times stays a host array), queued on the context's stream without
 * synchronising; params->origin_extent is required, as in rmr_bake_probes_device. */
int rmr_bake_probe_visibility_device(rmr_ctx* ctx, const float* d_points, size_t n, const float* times, uint32_t nspp,
                                     const rmr_probe_params* params, float range, float* d_out_vis);
/* The maps of the context's field, stored with it ([points][128] floats and range); no synchronisation.
 * RMR_E_STATE without a field or without a scene. rmr_bake_probe_field, rmr_write_probe_field,
 * rmr_probe_field_free, rmr_reload and rmr_destroy drop the visibility (a new field has none). */
int rmr_bake_probe_field_visibility(rmr_ctx* ctx, const float* times, uint32_t nspp, float range);
/* Loads saved or synthetic maps for the context's field (vis: host memory, [points][128]); synchronises.
 * RMR_E_STATE without a field; needs no scene. */
int rmr_write_probe_field_visibility(rmr_ctx* ctx, const float* vis, float range);
/* The maps and / or the range to host memory (either may be NULL); synchronises. RMR_E_STATE without them. */
int rmr_read_probe_field_visibility(rmr_ctx* ctx, float* vis, float* range_out);
void* rmr_probe_field_visibility_device_ptr(rmr_ctx* ctx);
/* The weighted lookup over the context's field and its visibility; as rmr_probe_irradiance otherwise.
 * RMR_E_STATE without a field or without its visibility; RMR_E_INVALID for a bias that is not finite and >= 0. */
int rmr_probe_irradiance_vis(rmr_ctx* ctx, const float* points, const float* normals, size_t n, float bias,
                             float* out_rgba);
int rmr_probe_irradiance_vis_device(rmr_ctx* ctx, const float* d_points, const float* d_normals, size_t n, float bias,
                                    float* d_out_rgba);

/* ---- display ---------------------------------------------------------------------------- */
/* Graphics::Display(centre, zoom, min, max) (Graphics.cpp:356-390 with createFQ 227-258 and
 * FullQuad.vs / FullQuad.fs), headless: draws the accumulator into a screen_w x screen_h RGBA8 image
 * (row 0 = top, the window's coordinates; Screen::getScreenSize() is the image size) the way the
 * reference's textured quad does: quad [centre - size/2 zoom, centre + size/2 zoom), nearest texel
 * (GL_NEAREST, Graphics.h:90-91), alpha 1 inside [min, max] and 0 elsewhere, GL_FRAMEBUFFER_SRGB
 * encode (byte = round(255 srgb(clamp(c, 0, 1))), exact; rmr_srgb_thresholds) and the
 * SRC_ALPHA / ONE_MINUS_SRC_ALPHA blend: pixels drawn with alpha 1 are replaced, every other pixel
 * keeps the caller's content (the GUI behind the image). rgba8 is a host buffer (in/out) of nbytes
 * bytes; RMR_E_INVALID unless nbytes >= screen_w * screen_h * 4. */
int rmr_display(rmr_ctx* ctx, float centre_x, float centre_y, float zoom, float min_x, float min_y, float max_x,
                float max_y, int screen_w, int screen_h, uint8_t* rgba8, size_t nbytes);
/* The same into a device buffer of nbytes bytes (e.g. a torch uint8 tensor or an interop surface), on
 * the context's stream, without host copies or a sync. */
int rmr_display_device(rmr_ctx* ctx, float centre_x, float centre_y, float zoom, float min_x, float min_y,
                       float max_x, float max_y, int screen_w, int screen_h, void* rgba8_dev, size_t nbytes);
/* The 256 sRGB decision points rmr_display uses: out[k] = the smallest float c with byte(c) >= k. */
int rmr_srgb_thresholds(float out[256]);
/* Test hook, no GPU needed: the candidate grid a context builds for a BVH scene's nearest-primitive
 * cache (rmr_trace.h map_grid_npc). prims: n rows of 8 floats in leaf order (c.xyz, r.xyz, type
 * RMR_PRIM_SPHERE / RMR_PRIM_BOX as a float value, mat_id); rows [0, n_large) are evaluated everywhere
 * (large primitives), the rest are gridded. E = max |c|_inf + |r|_inf over the scene. target / pad:
 * cell count / region growth (<= 0: the context's defaults). Out: idims = (dim.xyz, list length,
 * built 0/1); geom = (lo.xyz, 1 / cell size, small-primitive box lo.xyz hi.xyz, eps, margin); cells:
 * 2 words per cell (offset | count << 24, bound bits); list: leaf indices. Returns RMR_E_INVALID with
 * idims filled when cells_cap (words) or list_cap is too small. */
int rmr_candidate_grid(const float* prims, int n, int n_large, double E, double target, double pad, int32_t idims[5],
                       float geom[12], uint32_t* cells, size_t cells_cap, uint16_t* list, size_t list_cap);
/* Per-scene kernel specialisation (the reference recompiles its shader per scene, Graphics::Reload):
 * the scene's map() is generated as HIP source with the primitives as literals and compiled by
 * hipRTC for gfx950 at the first render that uses it (code objects cached in-process and under
 * $RMR_JIT_CACHE or ~/.cache/rmr-jit). Results are bit-identical to the table-driven kernels.
 * mode 0 = off, 1 = always (errors are returned), 2 = auto (default: launches of >= 2^16 units;
 * a failed compile falls back to the table-driven kernel). (The diagnostic build librmr_diag.so also
 * reads env RMR_JIT at rmr_create; the release librmr.so reads no environment but RMR_JIT_CACHE.) */
int rmr_set_jit(rmr_ctx* ctx, int mode);
/* Exact work-skipping in the trace kernels (all results bit-identical; only the count of map()
 * calls changes), default all on (librmr_diag.so: env RMR_ESC=0 / RMR_NPC=0 / RMR_JIT_APPROX=0 /
 * RMR_EYE=0 clear a bit at rmr_create):
 *   RMR_CULL_ESCAPE: a march past the exit of the inflated scene box ends as its miss
 *   RMR_CULL_NPC:    nearest-primitive cache of the BVH map (scenes of > 32 spheres/boxes)
 *   RMR_CULL_APPROX: approximate-then-exact map() of sphere/box scenes (one exact sqrt)
 *   RMR_CULL_EYE:    every primary ray's first march step is map(eye): evaluated once per wave
 *                    (RM1 sphere/box/Mandelbulb kernels and RM3) */
#define RMR_CULL_ESCAPE 1
#define RMR_CULL_NPC 2
#define RMR_CULL_APPROX 4
#define RMR_CULL_EYE 8
int rmr_set_culling(rmr_ctx* ctx, int flags);
/* Instrumented specialised kernels (measurement only; the images are the same bits):
 *   RMR_INSTR_COUNT_FLOPS: the hipRTC kernel built with -DRMR_COUNT_FLOPS (rmr_trace.h count_work):
 *     executed SDF flops / transcendentals per map() into rmr_get_counters [11] / [12] / [13], one
 *     atomic per wave and counted event (so it is slower; bench.py's count pass, never timed).
 * Applies to the hipRTC kernels (rmr_set_jit 1); 0 restores the production kernel. */
#define RMR_INSTR_COUNT_FLOPS 1
int rmr_set_instrument(rmr_ctx* ctx, int flags);
/* Compile the specialised kernel of a scene without a GPU (json NULL = the variant's built-in
 * scene). On success `log` receives the code-object key, otherwise the compiler log. */
int rmr_jit_compile_scene(int variant, const char* json, size_t len, char* log, size_t loglen);
/* The same for the scene's ray-source kernel (rmr_jit_trace_rays: the specialised kernel of launches
 * under a camera model and of rmr_trace_rays). */
int rmr_jit_compile_scene_rays(int variant, const char* json, size_t len, char* log, size_t loglen);
/* Tuning knobs (<= 0 / < 0 keeps the current value): deferred-shading batch size in lanes (1..64),
 * persistent workgroups per CU (0 = occupancy), per-launch sample-plane budget in bytes. Until a
 * batch size is set (here, or by env RMR_SHADE_T in librmr_diag.so) it is chosen per kernel: 8 for general maps
 * without material programs, 16 otherwise. Results do not depend on any of these (scheduling only). */
int rmr_set_tuning(rmr_ctx* ctx, int shade_threshold, int grid_per_cu, long long samp_budget_bytes);
/* (shade_threshold bits 8..15, when non-zero, set the refill threshold separately: idle lanes a
 * wave collects before it fetches new units; default (and when zero) = half the shading
 * threshold, at least 2. Bits 0..7 zero leave the batch size as it is. With bit 23 set the value
 * also carries the settings of the kernels with lane slots — a second path per lane waiting in LDS,
 * RM1's certified sphere/box kernels: bits 16..22 the finished marches a wave collects before it
 * parks them (0: the kernel class's default; 127: the schedule off), bits 24..30 the waiting events
 * per shading batch (0: the class's default); with bits 0..15 zero it sets nothing else.) */
/* Persistent-grid reserve: the trace launch leaves `blocks` workgroups of its occupancy grid
 * unlaunched (default 0; the grid stays >= 1 workgroup). For two contexts that alternate frames on
 * one GPU (multi_gpu.FrameRenderer): a persistent trace kernel holds every slot it gets until its
 * queue runs out, so the other context's running-mean fold (and the next frame's zeroing) would
 * wait for that trace's drain, and the next trace behind them; a few free slots let them run beside
 * it. Scheduling only: results do not depend on it. RMR_E_INVALID for blocks < 0. */
int rmr_set_grid_reserve(rmr_ctx* ctx, int blocks);
/* Trailing steps of the lane-slot kernels (rmr_trace.h RMR_TRAIL_STEPS): behind each map-loop iteration's
 * whole map, up to `steps` (0..15) further march steps that evaluate the map's nearest primitive alone,
 * wherever a distance bound proves it the whole map's result: a fixed number of passes, without the pass
 * rule below. -1 (the default): the kernel class's own tuning. Takes effect only in kernels specialised with
 * the steps compiled in, and only with a positive stepMultiply. Scheduling only: every sample and
 * rmr_stats::map_evals are the same for every value. RMR_E_INVALID outside -1..15. */
int rmr_set_trail_steps(rmr_ctx* ctx, int steps);
/* The trailing passes chosen per wave: after each pass a wave takes another one if and only if fewer than
 * `k_max` (0..15) have run in this iteration, the lanes still taking part are at least `ratio_eighths` / 8
 * (0..8; 0: no lane test) of its active lanes, and, with `park_exit` (0 or 1), its finished lanes are still
 * fewer than the park threshold that ends the iteration. (k, 0, 0) is rmr_set_trail_steps(k). Replaces an
 * earlier rmr_set_trail_steps and is replaced by a later one. A tuning with a ratio or the park exit runs a
 * code object of its own, specialised with the rule compiled in at the next launch (the rule's scalar state
 * is not free in the kernel without it); a fixed schedule runs the one every other launch runs. Scheduling
 * only, as above. RMR_E_INVALID, with the offending argument in rmr_last_error, outside those ranges. */
int rmr_set_trail_tuning(rmr_ctx* ctx, int k_max, int ratio_eighths, int park_exit);
/* Test hook: per-sample radiance (before the running mean) of the integer rect, written as
 * out[k][y-y0][x-x0][4]; sample k is seeded with times[k]. The accumulator is left unchanged. */
int rmr_trace_samples(rmr_ctx* ctx, const float* times, int x0, int y0, int x1, int y1, uint32_t nspp, float* out);
/* sizeof of the ABI structs (prim, op, material, spectral, rm2_consts, scene, params, stats): writes
 * the first min(n, 8) and returns 8. With n >= 9 it also writes out[8] = sizeof(rmr_denoise_params);
 * the returned count stays 8 for callers that compare it with their own list of those eight. */
int rmr_abi_sizes(int32_t* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* RMR_H */
