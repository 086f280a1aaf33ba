// stage_state_test.cpp — host checks of the output stages' validity rule (stage_state.hpp; tests/
// test_stage_state_cpu.py builds and runs this program, plain and under the address and undefined-behaviour
// sanitizers).
//
// 1. Equivalence: namespace old_sites below is the assignments rmr_api.cpp made by hand before the rule had
//    one place, transcribed literally, one function per site, on nine loose variables. Random sequences of
//    1 to 40 entry-point calls run through both; after every call all nine fields are equal. A call the API
//    would refuse in the current state is skipped, as the API would.
// 2. Invariants after every call of the same walks: a valid tonemapped image of the bloom image implies a valid
//    bloom image; a valid bloom or tonemapped image of the temporal or denoised image implies that image is valid
//    (but for rmr_temporal_reset, which drops the history alone); the variance planes are readable only with a
//    valid denoised image; after the planes are freed nothing is valid.
// 3. The pinned cases the GPU tests walk (tests/test_gpu_bloom.py), as a table of calls and the validity
//    expected after them.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "stage_state.hpp"

using rmr::StageState;

static int g_fail = 0;
#define CHECK(c, ...)                                                     \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (g_fail++ < 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                 \
    } while (0)

struct Rng {
    uint64_t s;
    uint64_t next() {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        return s;
    }
    uint32_t below(uint32_t n) { return (uint32_t)((next() >> 11) % n); }
};

// ---- the oracle: the earlier hand-kept assignments, site by site -------------------------------------
namespace old_sites {
bool guides_valid;
int dn_result;
bool dn_guided;
int var_result;
int t_cur;
bool tm_valid;
int tm_source;
bool bl_valid;
int bl_source;

void create() {
    guides_valid = false; dn_result = -1; dn_guided = false; var_result = 0; t_cur = -1;
    tm_valid = false; tm_source = RMR_OUTPUT_ACCUM; bl_valid = false; bl_source = RMR_OUTPUT_ACCUM;
}
void free_guides() {
    guides_valid = false;
    dn_result = -1; tm_valid = false; bl_valid = false;
}
void free_temporal() { t_cur = -1; }
void free_tonemap() { tm_valid = false; }
void free_bloom() { bl_valid = false; }
void upload_scene() {
    guides_valid = false;
    t_cur = -1;
    dn_result = -1; tm_valid = false; bl_valid = false;
}
void render_tiles() { dn_result = -1; tm_valid = false; bl_valid = false; }
void rmr_render_deferred() { dn_result = -1; tm_valid = false; bl_valid = false; }
void rmr_write_accum() { dn_result = -1; tm_valid = false; bl_valid = false; }
void rmr_bind_accum() { dn_result = -1; tm_valid = false; bl_valid = false; }
void rmr_set_params() {
    guides_valid = false;
    dn_result = -1; tm_valid = false; bl_valid = false;
}
void rmr_set_view() {
    guides_valid = false;
    dn_result = -1; tm_valid = false; bl_valid = false;
}
void ensure_guides_fresh() { guides_valid = false; dn_result = -1; }
void render_guides_full() { guides_valid = true; }
void rmr_denoise_begin() {
    dn_result = -1; tm_valid = false; bl_valid = false;
    dn_guided = false;
}
void rmr_denoise_queued(int img) { dn_result = img; }
void rmr_denoise_variance_begin() {
    dn_result = -1; tm_valid = false; bl_valid = false;
    dn_guided = false;
}
void rmr_denoise_variance_queued(int img, int vres) {
    dn_result = img;
    var_result = vres;
    dn_guided = true;
}
void temporal_planes_fresh() { t_cur = -1; }
// rmr_temporal_accumulate from `bool have = ...` to the launch; returns `from`
int rmr_temporal_accumulate_begin(bool view_ok) {
    bool have = t_cur >= 0 && view_ok;
    if (!have) t_cur = 0;
    const int from = t_cur;
    t_cur = -1;
    if (tm_source == RMR_OUTPUT_TEMPORAL) tm_valid = false;
    if (bl_source == RMR_OUTPUT_TEMPORAL) {
        if (bl_valid && tm_source == RMR_OUTPUT_BLOOM) tm_valid = false;
        bl_valid = false;
    }
    return from;
}
void rmr_temporal_accumulate_queued(int from, bool t_keep) {
    const int to = 1 - from;
    if (t_keep) {
        t_cur = from;
        return;
    }
    t_cur = to;
}
void rmr_temporal_reset() { t_cur = -1; }
void ensure_tonemap_fresh() { tm_valid = false; }
void rmr_tonemap_begin() { tm_valid = false; }
void rmr_tonemap_queued(int source) {
    tm_source = source;
    tm_valid = true;
}
void rmr_diag_tonemap_time() { tm_valid = false; }
void ensure_bloom_fresh() { bl_valid = false; }
void rmr_bloom_begin() {
    bl_valid = false;
    if (tm_source == RMR_OUTPUT_BLOOM) tm_valid = false;
}
void rmr_bloom_queued(int source) {
    bl_source = source;
    bl_valid = true;
}
void rmr_diag_bloom_time() {
    bl_valid = false;
    if (tm_source == RMR_OUTPUT_BLOOM) tm_valid = false;
}
}  // namespace old_sites

// ---- the entry points, as far as the rule sees them ---------------------------------------------------
enum Kind {
    kRender, kRenderDeferred, kWriteAccum, kBindAccum, kSetView, kSetParams, kLoadScene, kReload, kRenderGuides,
    kDenoise, kDenoiseVariance, kTemporal, kTemporalReset, kBloom, kTonemap, kDiagBloomTime, kDiagTonemapTime, kKinds
};
struct Call {
    int kind;
    int source;       // kTemporal, kBloom, kTonemap
    int img, vres;    // the denoisers' result buffers
    bool fails;       // a launch between "begin" and "queued" fails (the stages with both)
    bool view_ok;     // kTemporal: the history's view has an inverse
    bool keep;        // kTemporal: the diagnostic library's t_keep
};
// which planes are allocated (the ensure_* functions reset their stage's part after a fresh allocation)
struct Planes { bool guides = false, temporal = false, tonemap = false, bloom = false; };

// A source a stage would refuse in this state (the callers' checks: tone_source, rmr_temporal_accumulate).
static bool refused(const StageState& s, const Call& c) {
    if (c.kind != kTemporal && c.kind != kBloom && c.kind != kTonemap) return false;
    return s.readable(c.source) < 0;
}

static void old_guides(Planes& p) {   // render_guides over the whole image
    if (!p.guides) { old_sites::ensure_guides_fresh(); p.guides = true; }
    old_sites::render_guides_full();
}
static void run_old(const Call& c, Planes& p) {
    using namespace old_sites;
    switch (c.kind) {
    case kRender: render_tiles(); break;
    case kRenderDeferred: rmr_render_deferred(); break;
    case kWriteAccum: rmr_write_accum(); break;
    case kBindAccum: rmr_bind_accum(); break;
    case kSetView: rmr_set_view(); break;
    case kSetParams: rmr_set_params(); break;
    case kLoadScene: upload_scene(); break;
    case kReload: free_guides(); free_temporal(); free_tonemap(); free_bloom(); p = Planes(); break;
    case kRenderGuides: old_guides(p); break;
    case kDenoise:
        rmr_denoise_begin();
        if (!guides_valid) old_guides(p);
        if (!c.fails) rmr_denoise_queued(c.img);
        break;
    case kDenoiseVariance:
        rmr_denoise_variance_begin();
        if (!guides_valid) old_guides(p);
        if (!c.fails) rmr_denoise_variance_queued(c.img, c.vres);
        break;
    case kTemporal: {
        if (!guides_valid) old_guides(p);
        if (!p.temporal) { temporal_planes_fresh(); p.temporal = true; }
        const int from = rmr_temporal_accumulate_begin(c.view_ok);
        if (!c.fails) rmr_temporal_accumulate_queued(from, c.keep);
        break;
    }
    case kTemporalReset: rmr_temporal_reset(); break;
    case kBloom:
        if (!p.bloom) { ensure_bloom_fresh(); p.bloom = true; }
        rmr_bloom_begin();
        if (!c.fails) rmr_bloom_queued(c.source);
        break;
    case kTonemap:
        if (!p.tonemap) { ensure_tonemap_fresh(); p.tonemap = true; }
        rmr_tonemap_begin();
        if (!c.fails) rmr_tonemap_queued(c.source);
        break;
    case kDiagBloomTime:
        if (!p.tonemap) { ensure_tonemap_fresh(); p.tonemap = true; }
        if (!p.bloom) { ensure_bloom_fresh(); p.bloom = true; }
        rmr_diag_bloom_time();
        break;
    case kDiagTonemapTime:
        if (!p.tonemap) { ensure_tonemap_fresh(); p.tonemap = true; }
        rmr_diag_tonemap_time();
        break;
    }
}

static void new_guides(StageState& s, Planes& p) {
    if (!p.guides) { s.guides_allocated(); p.guides = true; }
    s.guides_rendered();
}
static void run_new(StageState& s, const Call& c, Planes& p) {   // as rmr_api.cpp calls the rule
    switch (c.kind) {
    case kRender: case kRenderDeferred: case kWriteAccum: case kBindAccum: s.accum_changed(); break;
    case kSetView: case kSetParams: s.inputs_changed(); break;
    case kLoadScene: s.scene_loaded(); break;
    case kReload: s.guides_freed(); s.temporal_reset(); s.tonemap_begin(); s.bloom_reset(); p = Planes(); break;
    case kRenderGuides: new_guides(s, p); break;
    case kDenoise:
        s.denoise_begin();
        if (!s.guides_valid) new_guides(s, p);
        if (!c.fails) s.denoise_queued(c.img);
        break;
    case kDenoiseVariance:
        s.denoise_begin();
        if (!s.guides_valid) new_guides(s, p);
        if (!c.fails) s.denoise_guided_queued(c.img, c.vres);
        break;
    case kTemporal: {
        if (!s.guides_valid) new_guides(s, p);
        if (!p.temporal) { s.temporal_reset(); p.temporal = true; }
        const bool have = s.t_cur >= 0 && c.view_ok;
        const int from = have ? s.t_cur : 0;
        s.temporal_begin();
        if (!c.fails) s.temporal_queued(c.keep ? from : 1 - from);
        break;
    }
    case kTemporalReset: s.temporal_reset(); break;
    case kBloom:
        if (!p.bloom) { s.bloom_reset(); p.bloom = true; }
        s.bloom_begin();
        if (!c.fails) s.bloom_queued(c.source);
        break;
    case kTonemap:
        if (!p.tonemap) { s.tonemap_begin(); p.tonemap = true; }
        s.tonemap_begin();
        if (!c.fails) s.tonemap_queued(c.source);
        break;
    case kDiagBloomTime:
        if (!p.tonemap) { s.tonemap_begin(); p.tonemap = true; }
        if (!p.bloom) { s.bloom_reset(); p.bloom = true; }
        s.bloom_begin();
        break;
    case kDiagTonemapTime:
        if (!p.tonemap) { s.tonemap_begin(); p.tonemap = true; }
        s.tonemap_begin();
        break;
    }
}

static bool equal_to_old(const StageState& s) {
    using namespace old_sites;
    return s.guides_valid == guides_valid && s.dn_result == dn_result && s.dn_guided == dn_guided &&
           s.var_result == var_result && s.t_cur == t_cur && s.tm_valid == tm_valid && s.tm_source == tm_source &&
           s.bl_valid == bl_valid && s.bl_source == bl_source;
}

// reset_since: rmr_temporal_reset ran since the last temporal step. It drops the history and nothing else, as it
// always did: a bloom or tonemapped image made from the dropped temporal image stays readable until the next step.
static void check_invariants(const StageState& s, int kind, bool reset_since) {
    CHECK(!(s.tm_valid && s.tm_source == RMR_OUTPUT_BLOOM) || s.bl_valid, "a tonemapped image of no bloom image (after %d)", kind);
    const int made_from[2] = {s.bl_valid ? s.bl_source : -1, s.tm_valid ? s.tm_source : -1};
    for (int src : made_from)
        if ((src == RMR_OUTPUT_TEMPORAL && !reset_since) || src == RMR_OUTPUT_DENOISED)
            CHECK(s.readable(src) >= 0, "an image made from source %d, which is not valid (after %d)", src, kind);
    // (as its readers see it: the field itself outlives the image, e.g. across a render, as it always did,
    // and every reader tests it together with dn_result, now inside variance_plane)
    for (int which : {RMR_VARIANCE_SEED, RMR_VARIANCE_FILTERED})
        CHECK((s.variance_plane(which) >= 0) == (s.dn_guided && s.dn_result >= 0) && (s.variance_plane(which) < 0 || s.dn_result >= 0),
              "guided without a denoised image (after %d)", kind);
    if (kind == kReload)
        CHECK(!s.guides_valid && s.dn_result < 0 && s.t_cur < 0 && !s.tm_valid && !s.bl_valid, "valid after the planes were freed");
}

static Call random_call(Rng& g) {
    static const int kTemporalSources[2] = {RMR_OUTPUT_ACCUM, RMR_OUTPUT_DENOISED};
    static const int kBloomSources[3] = {RMR_OUTPUT_ACCUM, RMR_OUTPUT_DENOISED, RMR_OUTPUT_TEMPORAL};
    static const int kToneSources[4] = {RMR_OUTPUT_ACCUM, RMR_OUTPUT_DENOISED, RMR_OUTPUT_TEMPORAL, RMR_OUTPUT_BLOOM};
    Call c{};
    // the stages twice as often as the rest, so that chains of images get long
    const uint32_t k = g.below(kKinds + 5);
    static const int kMore[5] = {kDenoise, kDenoiseVariance, kTemporal, kBloom, kTonemap};
    c.kind = k < (uint32_t)kKinds ? (int)k : kMore[k - kKinds];
    if (c.kind == kTemporal) c.source = kTemporalSources[g.below(2)];
    if (c.kind == kBloom) c.source = kBloomSources[g.below(3)];
    if (c.kind == kTonemap) c.source = kToneSources[g.below(4)];
    c.img = (int)g.below(2);
    c.vres = c.kind == kDenoiseVariance ? (int)g.below(3) : 0;   // 0: the seed itself (no iterations)
    c.fails = g.below(16) == 0;
    c.view_ok = g.below(8) != 0;
    c.keep = g.below(8) == 0;
    return c;
}

static void walks(int n_walks) {
    Rng g{0x9e3779b97f4a7c15ull};
    long calls = 0, skipped = 0;
    for (int w = 0; w < n_walks; w++) {
        old_sites::create();
        StageState s;
        Planes p_old, p_new;
        CHECK(equal_to_old(s), "a fresh context");
        const int len = 1 + (int)g.below(40);
        bool reset_since = false;
        for (int i = 0; i < len; i++) {
            const Call c = random_call(g);
            if (refused(s, c)) { skipped++; continue; }
            run_old(c, p_old);
            run_new(s, c, p_new);
            calls++;
            CHECK(equal_to_old(s), "walk %d call %d kind %d source %d", w, i, c.kind, c.source);
            if (c.kind == kTemporal || c.kind == kTemporalReset) reset_since = c.kind == kTemporalReset;
            check_invariants(s, c.kind, reset_since);
        }
    }
    std::printf("walks: %d\ncalls: %ld\nskipped: %ld\n", n_walks, calls, skipped);
}

// ---- the pinned cases -------------------------------------------------------------------------------------
struct Valid { bool denoised, temporal, bloom, tonemapped; };
struct Pinned { const char* what; int n; Call calls[8]; Valid want; };
static Call call(int kind, int source = RMR_OUTPUT_ACCUM) { return Call{kind, source, 0, 1, false, true, false}; }

static void pinned() {
    const Call bloom = call(kBloom), tone_bloom = call(kTonemap, RMR_OUTPUT_BLOOM);
    const Pinned cases[] = {
        {"the chain", 2, {bloom, tone_bloom}, {false, false, true, true}},
        {"a render", 3, {bloom, tone_bloom, call(kRender)}, {false, false, false, false}},
        {"a deferred rmr_render", 3, {bloom, tone_bloom, call(kRenderDeferred)}, {false, false, false, false}},
        {"rmr_write_accum", 3, {bloom, tone_bloom, call(kWriteAccum)}, {false, false, false, false}},
        {"rmr_set_view", 3, {bloom, tone_bloom, call(kSetView)}, {false, false, false, false}},
        {"rmr_set_params", 3, {bloom, tone_bloom, call(kSetParams)}, {false, false, false, false}},
        {"rmr_denoise", 3, {bloom, tone_bloom, call(kDenoise)}, {true, false, false, false}},
        {"rmr_denoise_variance", 3, {bloom, tone_bloom, call(kDenoiseVariance)}, {true, false, false, false}},
        {"a scene load", 3, {bloom, tone_bloom, call(kLoadScene)}, {false, false, false, false}},
        {"rmr_reload", 3, {bloom, tone_bloom, call(kReload)}, {false, false, false, false}},
        {"rmr_bind_accum", 3, {bloom, tone_bloom, call(kBindAccum)}, {false, false, false, false}},
        // the next temporal step replaces the image the bloom image was made from
        {"a temporal step under bloom(temporal) -> tonemap(bloom)", 5,
         {call(kDenoise), call(kTemporal, RMR_OUTPUT_DENOISED), call(kBloom, RMR_OUTPUT_TEMPORAL), tone_bloom,
          call(kTemporal, RMR_OUTPUT_DENOISED)}, {true, true, false, false}},
        {"a temporal step leaves a bloom image of the denoised image", 3,
         {call(kDenoise), call(kBloom, RMR_OUTPUT_DENOISED), call(kTemporal, RMR_OUTPUT_DENOISED)}, {true, true, true, false}},
        {"a temporal step drops a tonemapped image of the temporal image", 3,
         {call(kTemporal), call(kTonemap, RMR_OUTPUT_TEMPORAL), call(kTemporal)}, {false, true, false, false}},
        {"the next rmr_bloom drops a tonemapped image of the bloom image", 3, {bloom, tone_bloom, bloom}, {false, false, true, false}},
        {"and leaves one of another source", 3, {bloom, call(kTonemap), bloom}, {false, false, true, true}},
        {"rmr_temporal_reset", 2, {call(kTemporal), call(kTemporalReset)}, {false, false, false, false}},
        {"a render leaves the temporal image", 2, {call(kTemporal), call(kRender)}, {false, true, false, false}},
    };
    int n = 0;
    for (const Pinned& c : cases) {
        StageState s;
        Planes p;
        for (int i = 0; i < c.n; i++) {
            CHECK(!refused(s, c.calls[i]), "%s: call %d refused", c.what, i);
            run_new(s, c.calls[i], p);
        }
        const Valid got = {s.readable(RMR_OUTPUT_DENOISED) >= 0, s.readable(RMR_OUTPUT_TEMPORAL) >= 0,
                           s.readable(RMR_OUTPUT_BLOOM) >= 0, s.readable(RMR_OUTPUT_TONEMAPPED) >= 0};
        CHECK(std::memcmp(&got, &c.want, sizeof got) == 0, "%s: denoised %d temporal %d bloom %d tonemapped %d", c.what,
              got.denoised, got.temporal, got.bloom, got.tonemapped);
        n++;
    }
    std::printf("pinned: %d\n", n);
}

static void query() {
    StageState s;
    CHECK(s.readable(RMR_OUTPUT_ACCUM) == 0, "the accumulator is always readable");
    CHECK(s.readable(-1) == StageState::kNoSource && s.readable(5) == StageState::kNoSource, "no such source");
    for (int src = RMR_OUTPUT_DENOISED; src <= RMR_OUTPUT_BLOOM; src++) CHECK(s.readable(src) == StageState::kNotValid, "source %d", src);
    s.denoise_guided_queued(1, 2);
    s.temporal_queued(1);
    CHECK(s.readable(RMR_OUTPUT_DENOISED) == 1 && s.readable(RMR_OUTPUT_TEMPORAL) == 1, "the buffer index");
    CHECK(s.variance_plane(RMR_VARIANCE_SEED) == 0 && s.variance_plane(RMR_VARIANCE_FILTERED) == 2, "the variance planes");
}

int main() {
    walks(250000);
    pinned();
    query();
    if (g_fail) {
        std::printf("FAIL: %d checks\n", g_fail);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
