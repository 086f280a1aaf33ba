// Which of the output stages' images are valid: the guides, the denoised image and its
// variance planes, the temporal image, the bloom image and the tonemapped image. The context (rmr_api.cpp)
// holds one StageState and tells it what happens; nothing else assigns these fields. No HIP here, so the
// rule runs on a CPU (stage_state_test.cpp, tests/test_stage_state_cpu.py).
//
// What depends on what: the denoised, bloom and tonemapped images are made from the accumulator or from
// each other (denoised <- accumulator; temporal <- accumulator | denoised, and its own history; bloom <-
// accumulator | denoised | temporal; tonemapped <- any of those | bloom). An event that changes the
// accumulator drops the three of them whatever their sources (conservative: also a tonemapped image of the
// temporal image); the temporal image only goes with its scene, its planes or a reset.
#pragma once
#include "../../include/rmr.h"

namespace rmr {

struct StageState {
    bool guides_valid = false;         // one guide pass covered the image with the current view / scene / params
    int dn_result = -1;                // d_dn[] index of the valid denoised image, -1: none
    bool dn_guided = false;            // the valid denoised image is rmr_denoise_variance's
    int var_result = 0;                // d_var[] index of its filtered variance (0: the seed itself)
    int t_cur = -1;                    // the pair that holds the history (= the temporal image), -1: none
    bool tm_valid = false;             // d_tm holds the image of tm_source as it is now
    int tm_source = RMR_OUTPUT_ACCUM;
    bool bl_valid = false;             // d_bl holds the bloom of bl_source as it is now
    int bl_source = RMR_OUTPUT_ACCUM;

    // ---- what a source answers to a reader ----
    enum : int { kNotValid = -1, kNoSource = -2 };
    // The buffer index (0 where the image has one buffer) of a valid RMR_OUTPUT_* image, kNotValid, or
    // kNoSource for a value that names no image.
    int readable(int source) const {
        switch (source) {
        case RMR_OUTPUT_ACCUM: return 0;
        case RMR_OUTPUT_DENOISED: return dn_result >= 0 ? dn_result : kNotValid;
        case RMR_OUTPUT_TEMPORAL: return t_cur >= 0 ? t_cur : kNotValid;
        case RMR_OUTPUT_TONEMAPPED: return tm_valid ? 0 : kNotValid;
        case RMR_OUTPUT_BLOOM: return bl_valid ? 0 : kNotValid;
        default: return kNoSource;
        }
    }
    // The d_var[] index of a variance plane (RMR_VARIANCE_*) of the valid guided denoise, or kNotValid.
    int variance_plane(int which) const {
        if (dn_result < 0 || !dn_guided) return kNotValid;
        return which == RMR_VARIANCE_SEED ? 0 : var_result;
    }

    // ---- events ----
    // The accumulator changed (a render, rmr_write_accum, rmr_bind_accum).
    void accum_changed() { dn_result = -1; tm_valid = false; bl_valid = false; }
    // The view or the parameters changed.
    void inputs_changed() { guides_valid = false; accum_changed(); }
    // A scene was loaded: the temporal history is of the old scene.
    void scene_loaded() { inputs_changed(); t_cur = -1; }

    // A guide pass covered the whole image.
    void guides_rendered() { guides_valid = true; }
    // The guide planes and filter images were freed / freshly allocated.
    void guides_freed() { inputs_changed(); }
    void guides_allocated() { guides_valid = false; dn_result = -1; }

    // A denoise begins (either form); its last launch is queued, the result in d_dn[img] (and d_var[vres]).
    void denoise_begin() { accum_changed(); dn_guided = false; }
    void denoise_queued(int img) { dn_result = img; }
    void denoise_guided_queued(int img, int vres) { dn_result = img; var_result = vres; dn_guided = true; }

    // The history is dropped (rmr_temporal_reset, its planes freed or freshly allocated).
    void temporal_reset() { t_cur = -1; }
    // A temporal step begins: no temporal image until temporal_queued, and every valid image made from
    // the old one goes: the bloom of it, and what was tonemapped from it or from that bloom.
    void temporal_begin() {
        t_cur = -1;
        if (tm_source == RMR_OUTPUT_TEMPORAL) tm_valid = false;
        if (bl_source == RMR_OUTPUT_TEMPORAL) bloom_begin();
    }
    void temporal_queued(int pair) { t_cur = pair; }

    // A bloom begins: no bloom image until bloom_queued, nor a tonemapped image made from the old one.
    void bloom_begin() {
        bl_valid = false;
        if (tm_source == RMR_OUTPUT_BLOOM) tm_valid = false;
    }
    void bloom_queued(int source) { bl_source = source; bl_valid = true; }
    // The bloom planes were freed or freshly allocated (a tonemapped image of the bloom image goes with the
    // tonemap stage's planes, freed at the same points).
    void bloom_reset() { bl_valid = false; }

    // A tonemap begins (also: its planes were freed or freshly allocated); its last launch is queued.
    void tonemap_begin() { tm_valid = false; }
    void tonemap_queued(int source) { tm_source = source; tm_valid = true; }
};

}  // namespace rmr
