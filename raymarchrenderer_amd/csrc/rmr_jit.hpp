// rmr_jit.hpp — per-scene specialisation of the trace kernel with hipRTC.
//
// The reference recompiles its compute shader whenever the scene changes: Graphics::Reload
// generates GLSL for every object and material and hands it to the GL driver (Graphics.cpp:
// 392-752). rmr does the MI355X equivalent: the scene's map() is emitted as straight-line HIP with
// every primitive's centre, size and material id as literals, compiled by hipRTC for gfx950 against
// the same device code as the ahead-of-time kernels (rmr_trace.h), and launched in their place. The
// arithmetic is the same expression for expression, so the results are bit-identical; what goes
// away is the per-primitive scalar loads and type branches (measured +14% on Cornell-5).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "rmr_trail_rule.h"
#include "scene.hpp"

// Environment switches (RMR_GRID, RMR_JIT_OPTS, RMR_JIT_BAKE, ...: A/B experiments, tools/) exist only
// in the diagnostic build librmr_diag.so (`make diag`, -DRMR_DIAG=1). The release librmr.so reads no
// environment variable but RMR_JIT_CACHE (and HOME for its default) and GPU_MAX_HW_QUEUES (rmr_create:
// the number of launch slots): a drop-in renderer's results and kernels do not depend on an inherited
// environment. RMR_ENV("X") is nullptr there, and the name does not reach the binary. Only rmr_api.cpp
// and rmr_jit.cpp, the two files built twice, use RMR_ENV; other units take the switches as arguments.
#ifndef RMR_DIAG
#define RMR_DIAG 0
#endif
#if RMR_DIAG
#define RMR_ENV(name) std::getenv(name)
#else
#define RMR_ENV(name) ((const char*)nullptr)
#endif

namespace rmr {

struct JitKernel {
    std::string key;            // hash of source + options
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
    int blocks_per_cu = 0;
    int shade_t = 16;           // default shading batch size for this kernel (rmr_api.cpp)
    int block = 256;            // workgroup size
    int chunk = 128;            // units a wave takes from the work queue at a time (rmr_trace.h
                                // RMR_CHUNK; the nearest-primitive cache kernels: RMR_CHUNK_CACHE)
    bool slots = false;         // the lane-slot schedule (rmr_trace.h RMR_LANE_SLOTS)
    int park_t = 0, slot_t = 0; // its default thresholds (JitFacts)
    int slot_t_small = 0;       // ... the batch threshold of launches under kSlotSmallClaims claims per wave
    bool trail = false;         // the source has the trailing steps (rmr_trace.h RMR_TRAIL_STEPS)
    bool trail_rule = false;    // ... and the pass rule (RMR_TRAIL_RULE: the code object of rmr_set_trail_tuning's rule)
    int trail_word = 0;         // ... and runs its passes by this tuning unless told otherwise (rmr_trail_rule.h
    int trail_word_small = 0;   //     trail_word; launches under kSlotSmallClaims claims per wave: the second)
};

// What jit_source decided about the kernel class (the launch settings follow from these, not from
// the text of the source): the nearest-primitive cache map (TableMap<-3>: 64-unit chunks), a general
// map (Mandelbulb / node-program objects), node-program materials, certified getNormal probes.
struct JitFacts {
    int variant = 0;
    bool cache = false, general = false, prog = false, cert = false;
    // the lane-slot schedule (rmr_trace.h RMR_LANE_SLOTS): the class can run it (RM1's certified
    // sphere/box kernels) / this source has it on
    bool slots_ok = false, slots = false;
    bool overflow = false;   // ... with the park step's overflow deposit (rmr_trace.h RMR_SLOT_OVERFLOW)
    bool trail = false;      // ... with the trailing steps compiled in (rmr_trace.h RMR_TRAIL_STEPS)
    // the trailing passes' tuning where the source has them (rmr_trail_rule.h trail_word: at most k_max passes
    // per map-loop iteration, the pass rule's ratio in eighths, its park exit),
    // and the same for launches under kSlotSmallClaims claims per wave. Fixed schedules: the class's own code
    // object has no pass rule (rmr_trace.h RMR_TRAIL_RULE). Three passes: same process, 1080p 64 spp, K = 2 / 3 / 4
    // / 5 at 35.23 / 34.51 / 34.53 / 34.95 ms, and 480x270 1 spp 0.719 / 0.658 ms at K = 2 / 3
    // (profiles/trail_adaptive_sweep.log, trail_adaptive_small.log)
    int trail_word() const { return trail ? rmr::trail_word(3, 0, false) : 0; }
    int trail_word_small() const { return trail ? rmr::trail_word(3, 0, false) : 0; }
    int chunk() const { return (cache || slots) ? 64 : 128; }   // rmr_trace.h RMR_CHUNK_CACHE / RMR_CHUNK_SLOTS / RMR_CHUNK
    // lane slots: finished marches per park step, slot events per shading batch (Cornell-5 1080p 64 spp:
    // flat over 8-10 / 28-40, +10% and more outside 6-12 / 24-48)
    int park_t() const { return 8; }
    // With the overflow deposit a lane no longer waits on its own full slot, and the batch pays up to
    // 48 events (same process, 64 spp: (8, 32) -1.9%, (8, 40) -2.9%, (8, 48) -3.3% against (8, 32) without
    // it; at 56 the wave runs out of empty slots, +7.7%; profiles/slot_overflow_sweep.log)
    int slot_t() const { return overflow ? 48 : 32; }
    // Launches that give a wave fewer than kSlotSmallClaims work claims keep 32: the end of the launch,
    // where batches fire only once no lane is active, is a larger share of them, and a larger batch makes
    // it longer (same process, overflow on, (8, 32) / (8, 48) against the parent: 480x270 1 spp +0.6 / +4.5%,
    // 640x360 4 spp -8.6 / -1.6%, 1080p 1 spp -9.6 / -6.3%, 4 spp -4.4 / -3.9%, 8 spp -5.1 / -4.8%, 16 spp
    // -2.6 / -3.4%, 32 spp -2.0 / -3.1%, 64 spp -1.9 / -3.3%; profiles/slot_overflow_sweep.log)
    int slot_t_small() const { return 32; }
    static constexpr int kSlotSmallClaims = 64;
    // default shading batch: general maps without material programs, whose map() dwarfs the shading
    // (the Mandelbulb): 10 (C3: 8 / 12 within 0.6%, 6 / 16 +3%, profiles/r05_c3_shade_ab.log); node-program materials, the cache kernels and the certified
    // sphere/box kernels (their batches run the certified probes): 20; otherwise 16 (rmr_api.cpp)
    int shade_t() const {
        if (variant == RMR_VARIANT_RM1 && general && !prog) return 10;
        if (prog || cache || cert) return 20;
        return 16;
    }
};

// HIP source of the specialised trace kernel for `s` (entry point "rmr_jit_trace"). bake: the
// primitives' numbers are literals (fastest: +6-12% over loading them); otherwise only the scene's
// structure is compiled and the numbers are scalar loads, so a scene that only moves (an animation)
// reuses one kernel instead of recompiling per frame.
// cull: RMR_CULL_* bits of the context (rmr.h): approximate-then-exact map, nearest-primitive cache.
// live (with bake): primitives j with live[j] != 0 are loaded even so (an animation's moving
// primitives; the rest stay literals).
// npc_k: primitives per lane in the nearest-primitive cache (RMR_NPC_K: 1 or 2) of BVH scenes.
// npc_spheres: every primitive the candidate grid lists is a sphere (RMR_NPC_SPHERES: the full
// map's candidates take the sphere distance, the same value as the general form for a sphere).
// facts (optional): the kernel class, for the launch settings.
// slots: the lane-slot schedule where the class can run it: 1 on, 0 off, -1 the class's default.
// rays: the ray-source kernel (entry point "rmr_jit_trace_rays(KParams, const float4* rays)", the source
// defines RMR_RAY_SRC): primary rays from a ray buffer, no lane slots. With rays off the source is
// what it was without the switch.
std::string jit_source(const CompiledScene& s, bool prog, bool bake = true, int cull = 7,
                       const std::vector<char>* live = nullptr, int npc_k = 2, bool npc_spheres = false,
                       JitFacts* facts = nullptr, int slots = -1, bool rays = false);
// Compile `src` for gfx950 (no GPU needed). Code-object cache: in-process, then the directory
// $RMR_JIT_CACHE (default $HOME/.cache/rmr-jit). Returns false with the compiler log in `log`.
// opts: further compiler options, part of the key (the instrumented build of rmr_set_instrument:
// -DRMR_COUNT_FLOPS).
bool jit_compile(const std::string& src, std::vector<char>& code, std::string& key, std::string& log,
                 const std::vector<std::string>& opts = {});

}  // namespace rmr
