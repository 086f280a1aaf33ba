// Program.cpp — headless driver (rmr_cli): the reference's main loop (Program.cpp:86-323) and the
// console commands of CLI.cpp:190-218, without the SFML window / GUI.
//
//  * fixed-spp mode (samples > 0, Program.cpp:232-299): tiles of a gridW x gridH grid in the
//    outward spiral order of Program.cpp:113-115/203-222, each tile rendered to `samples` samples
//    before moving on;
//  * progressive mode (samples == 0, Program.cpp:184-231): every pass renders ONE sample of every
//    tile in spiral order, `--passes` passes;
//  * the seed uniform follows the deterministic schedule time(f, s) = 1000 f + 0.016 s (SURVEY
//    §8d) instead of the wall clock the reference passes (Program.cpp:319);
//  * by default a tile's samples go to the GPU in one batched call (Graphics::RenderSamples,
//    bitwise equal to the per-sample calls); --per-sample issues one Graphics::Render per sample
//    per tile exactly like the reference;
//  * save() writes output/<%Y-%m-%d_%H-%M-%S>.bmp (Program.cpp:71-84) unless --out is given;
//  * --gpus N / --devices a,b,..: the frame tile-partitioned over several GPUs of the node from this one
//    process (Graphics::setDevices -> librmr_group.so, one RCCL reduce per frame): the whole image
//    rendered as one frame of `samples` samples (or `passes` in progressive mode), bitwise the image
//    the tile loop gives wherever the grid covers it (every pixel gets the same seeds in the same order).
#include <sys/stat.h>
#include <dirent.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "Camera.h"
#include "Graphics.h"
#include "Screen.h"

using Vector::Vector2;
using Vector::Vector3;

namespace {

const float PI = 3.141592653f;  // Program.cpp:62

struct Options {
    std::string scene, out, checkpoint, resume, scene_dir = "scenes", env_map;
    int env_w = 0, env_h = 0;
    int variant = -1;
    int width = 800, height = 600;  // Graphics.cpp:6
    int samples = 128;              // Program.cpp:104
    int passes = 16;
    int grid_w = 4, grid_h = 4;     // Program.cpp:106-107
    int frame = 0;
    int device = 0;
    std::vector<int> devices;       // --gpus / --devices: the device group
    bool per_sample = false, interactive = false, quiet = false;
    bool print_tiles = false, print_view = false;  // host-only diagnostics (no GPU needed)
    rmr_params params;
    int denoise = -1;               // --denoise [N]: a-trous iterations, -1 = no denoise
    bool tonemap = false;           // --tonemap / --exposure: the tone-mapping stage runs last, with `tone`
    rmr_tonemap_params tone{};
    bool bloom = false;             // --bloom [THRESHOLD[:INTENSITY]]: the bloom stage runs before the tone mapping
    rmr_bloom_params bloom_p{};
    double variance_guided = -1.0;  // --variance-guided [SIGMA_L]: the guided filter's sigma_l, < 0 = the plain filter
    std::string aov;                // --aov PREFIX: guide planes as PREFIX_*.pfm
    std::string sampled_aov;        // --sampled-aov PREFIX: the sampled AOVs as PREFIX_*.pfm
    std::string mesh;               // --mesh FILE.obj|FILE.ply: the scene's surface-nets mesh
    bool mesh_ply = false;
    bool have_mesh_bounds = false, have_mesh_opts = false;
    double mesh_bounds[6] = {0, 0, 0, 0, 0, 0};   // --mesh-bounds x0,y0,z0,x1,y1,z1
    int mesh_grid = 128;            // --mesh-grid N: cells along the longest side
    float mesh_iso = 0.0f;          // --mesh-iso V
    int mesh_bake = 0;              // --mesh-bake N[:AO_DISTANCE]: seeds of the vertex bake (0: none)
    bool mesh_bake_ao = false;
    float mesh_bake_ao_distance = 0.0f;
    std::string probes;             // --probes FILE: the irradiance probe field (rmr.h rmr_bake_probe_field)
    bool have_probe_bounds = false, have_probe_opts = false;
    double probe_bounds[6] = {0, 0, 0, 0, 0, 0};  // --probe-bounds x0,y0,z0,x1,y1,z1
    int probe_grid = 8;             // --probe-grid N: cells along the longest side
    int probe_samples = 256;        // --probe-samples K: seeds per probe
    int probe_vis = 0;              // --probe-visibility K[:RANGE]: seeds per probe of the visibility maps (0: none)
    float probe_vis_range = 0.0f;   //   RANGE (0: 2.6f * spacing)
    double adaptive = -1.0;         // --adaptive T: the tile-error threshold, < 0 = uniform sampling
    int min_samples = 16, pass_samples = 16;   // --min-samples / --pass-samples (rmr_adaptive_params)
    bool have_camera = false;
    double cam[6] = {0, 4, -6, 0, -3, 6};
    rmr_camera_model model;         // --camera thinlens:A,F | equirect | ortho:W,H (default: the view's own rays)
};

// Program.cpp:113-115, 203-222: the outward spiral over the tile grid
std::vector<std::pair<int, int>> tile_spiral(int gw, int gh) {
    std::vector<std::pair<int, int>> order;
    int x = (int)std::ceil((float)gw / 2.0) - 1, y = (int)std::ceil((float)gh / 2.0) - 1;
    int dx = -1, dy = 0, passed = 0, last = 0, dist = 0;
    while (passed < gw * gh) {
        order.emplace_back(x, y);
        x -= gw / 2;
        y -= gh / 2;
        if (dist * 2 == passed - last) {
            dist++;
            last = passed;
            const int t = dx; dx = dy; dy = -t;
        } else if (dist == passed - last) {
            const int t = dx; dx = dy; dy = -t;
        }
        passed++;
        x += dx + gw / 2;
        y += dy + gh / 2;
    }
    return order;
}

float seed_time(int frame, unsigned s) { return (float)(1000.0 * frame + 0.016 * (double)s); }

std::string read_file(const std::string& path, bool* ok) {
    std::ifstream f(path, std::ios::binary);
    *ok = (bool)f;
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// Split a scene file's "materials" / "objects" arrays into per-element JSON texts for
// Graphics::addMaterial / addObject (CLI.cpp:63-75 addScene). A small bracket matcher: strings
// are skipped, so brackets inside names do not count.
bool split_array(const std::string& js, const std::string& key, std::vector<std::string>& out) {
    const size_t k = js.find("\"" + key + "\"");
    if (k == std::string::npos) return true;  // absent = empty
    size_t i = js.find('[', k);
    if (i == std::string::npos) return false;
    int depth = 0;
    size_t start = std::string::npos;
    bool in_str = false;
    for (; i < js.size(); i++) {
        const char c = js[i];
        if (in_str) {
            if (c == '\\') i++;
            else if (c == '"') in_str = false;
            continue;
        }
        if (c == '"') { in_str = true; continue; }
        if (c == '[' || c == '{') {
            if (depth == 1 && start == std::string::npos) start = i;
            depth++;
        } else if (c == ']' || c == '}') {
            depth--;
            if (depth == 1 && start != std::string::npos) {
                out.push_back(js.substr(start, i - start + 1));
                start = std::string::npos;
            }
            if (depth == 0) return true;
        }
    }
    return false;
}

bool load_scene(const std::string& path) {
    bool ok = false;
    const std::string js = read_file(path, &ok);
    if (!ok) {
        std::cout << "Failed to load file" << std::endl;  // CLI.cpp:58-61
        return false;
    }
    std::vector<std::string> mats, objs;
    if (!split_array(js, "materials", mats) || !split_array(js, "objects", objs)) {
        std::cout << "Failed to parse configuration" << std::endl;
        return false;
    }
    Graphics::clearScene();
    for (auto& m : mats) Graphics::addMaterial(m);
    for (auto& o : objs) Graphics::addObject(o);
    return true;
}

std::string save_name() {
    std::time_t t = std::time(nullptr);
    std::tm now;
    localtime_r(&t, &now);
    char buf[80];
    std::strftime(buf, sizeof buf, "%Y-%m-%d_%H-%M-%S", &now);
    return std::string(buf) + ".bmp";
}

void save(const Options& o) {  // Program.cpp:71-84
    std::string path = o.out;
    if (path.empty()) {
        mkdir("output", 0755);
        path = "output/" + save_name();
    }
    Graphics::SaveImage(path);
    if (Graphics::lastStatus() == RMR_OK) std::cout << "Saved image as: " << path << std::endl;
}

struct RenderResult {
    double seconds = 0;
    unsigned long long samples = 0;
};

rmr_adaptive_params adaptive_params(const Options& o) {
    rmr_adaptive_params p;
    rmr_default_adaptive_params(&p);
    p.threshold = (float)o.adaptive;
    p.min_samples = (uint32_t)o.min_samples;
    p.pass_samples = (uint32_t)o.pass_samples;
    p.max_samples = (uint32_t)o.samples;
    return p;
}

// One render of the current scene: fixed-spp (samples > 0) or progressive (samples == 0).
RenderResult render(const Options& o, unsigned first_pass) {
    Graphics::Reload();
    if (o.variance_guided > 0) {   // the half image from the first sample on (rmr_denoise_variance needs it)
        Graphics::setErrorEstimate(true);
        if (Graphics::lastStatus() != RMR_OK) return RenderResult();
    }
    Camera camera(Vector3(o.cam[0], o.cam[1], o.cam[2]), Vector3(o.cam[3], o.cam[4], o.cam[5]).normalized(),
                  (float)(Graphics::getImageSize().x / Graphics::getImageSize().y), PI / 4);
    if (!o.resume.empty()) {
        unsigned done = 0;
        if (Graphics::loadCheckpoint(o.resume, &done)) first_pass = done;
    }
    const int W = (int)Graphics::getImageSize().x, H = (int)Graphics::getImageSize().y;
    const int cw = W / o.grid_w, ch = H / o.grid_h;  // Program.cpp:108-109 (remainder not rendered)
    const auto order = tile_spiral(o.grid_w, o.grid_h);
    RenderResult r;
    Graphics::Sync();
    const auto t0 = std::chrono::steady_clock::now();
    auto tile_rect = [&](std::pair<int, int> t, Vector2& mn, Vector2& mx) {
        mn = Vector2(t.first * cw, t.second * ch);
        mx = Vector2((t.first + 1) * cw, (t.second + 1) * ch);
    };
    if (!o.devices.empty()) {   // the device group: one frame over the whole image
        const unsigned n = o.samples > 0 ? (unsigned)o.samples : (unsigned)o.passes;
        std::vector<float> times(n);
        for (unsigned s = 0; s < n; s++) times[s] = seed_time(o.frame, s);
        Graphics::RenderFrame(times.data(), n);
        if (Graphics::lastStatus() != RMR_OK) return r;
        Graphics::Sync();
        r.samples = (unsigned long long)n * (unsigned long long)W * H;
        r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return r;
    }
    if (o.adaptive >= 0) {   // --adaptive T: the whole image, --samples as the maximum per pixel
        std::vector<float> times(o.samples);
        for (int s = 0; s < o.samples; s++) times[s] = seed_time(o.frame, s);
        rmr_adaptive_result res{};
        if (!Graphics::RenderAdaptive(times.data(), adaptive_params(o), &res)) return r;
        Graphics::Sync();
        r.samples = res.samples;
        r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("adaptive: passes %u, mean spp %.3f, open tiles %u, max error %.6g\n", res.passes,
                    (double)res.samples / ((double)W * H), res.tiles_open, (double)res.max_error);
        if (!o.checkpoint.empty()) Graphics::saveCheckpoint(o.checkpoint, (unsigned)o.samples);
        return r;
    }
    if (o.samples > 0) {
        std::vector<float> times(o.samples);
        for (int s = 0; s < o.samples; s++) times[s] = seed_time(o.frame, s);
        for (auto t : order) {
            Vector2 mn, mx;
            tile_rect(t, mn, mx);
            if (o.per_sample) {
                for (int s = 0; s < o.samples; s++) Graphics::Render(times[s], mn, mx, (unsigned)s);
            } else {
                Graphics::RenderSamples(times.data(), mn, mx, 0, (unsigned)o.samples);
            }
            if (Graphics::lastStatus() != RMR_OK) return r;
        }
        r.samples = (unsigned long long)o.samples * (unsigned long long)cw * ch * order.size();
    } else {
        for (unsigned s = first_pass; s < first_pass + (unsigned)o.passes; s++) {
            const float tm = seed_time(o.frame, s);
            for (auto t : order) {
                Vector2 mn, mx;
                tile_rect(t, mn, mx);
                Graphics::Render(tm, mn, mx, s);
            }
            if (Graphics::lastStatus() != RMR_OK) return r;
            if (!o.quiet) std::cout << s << std::endl;  // Program.cpp:197
        }
        r.samples = (unsigned long long)o.passes * (unsigned long long)cw * ch * order.size();
        if (!o.checkpoint.empty()) Graphics::saveCheckpoint(o.checkpoint, first_pass + o.passes);
    }
    Graphics::Sync();
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (o.samples > 0 && !o.checkpoint.empty()) Graphics::saveCheckpoint(o.checkpoint, (unsigned)o.samples);
    return r;
}

// --aov PREFIX: the first-hit guide planes as float images (rmr_encode_pfm): PREFIX_normal.pfm,
// PREFIX_position.pfm, PREFIX_ray.pfm (the planes' xyz) and PREFIX_depth_id.pfm (R = t, G = id, B = 0)
bool write_aovs(const Options& o) {
    rmr_ctx* c = Graphics::context();
    const int W = (int)Graphics::getImageSize().x, H = (int)Graphics::getImageSize().y;
    auto fail = [&](const std::string& what) {
        std::cerr << "--aov: " << what << ": " << rmr_last_error(c) << std::endl;
        return false;
    };
    if (rmr_render_guides(c, 0, 0, W, H) != RMR_OK) return fail("rmr_render_guides");
    const size_t n = (size_t)W * H * 4;
    std::vector<float> ray(n), hit(n), nrm(n), di(n, 0.0f);
    if (rmr_read_guide(c, RMR_GUIDE_RAY, ray.data(), n * sizeof(float)) != RMR_OK ||
        rmr_read_guide(c, RMR_GUIDE_HIT, hit.data(), n * sizeof(float)) != RMR_OK ||
        rmr_read_guide(c, RMR_GUIDE_NORMAL, nrm.data(), n * sizeof(float)) != RMR_OK)
        return fail("rmr_read_guide");
    for (size_t i = 0; i < (size_t)W * H; i++) {
        di[4 * i] = hit[4 * i + 3];
        di[4 * i + 1] = nrm[4 * i + 3];
    }
    const struct { const char* name; const std::vector<float>* img; } files[] = {
        {"_normal.pfm", &nrm}, {"_position.pfm", &hit}, {"_ray.pfm", &ray}, {"_depth_id.pfm", &di}};
    for (const auto& f : files) {
        const std::string path = o.aov + f.name;
        if (rmr_encode_pfm(f.img->data(), W, H, path.c_str()) != RMR_OK) {
            std::cerr << "--aov: cannot write " << path << std::endl;
            return false;
        }
        if (!o.quiet) std::cout << "Saved plane as: " << path << std::endl;
    }
    if (o.variance_guided > 0) {   // PREFIX_variance.pfm (R = the filtered variance, -1: not filtered)
        std::vector<float> var((size_t)W * H), vp(n, 0.0f);
        if (rmr_read_variance(c, RMR_VARIANCE_FILTERED, var.data(), var.size() * sizeof(float)) != RMR_OK)
            return fail("rmr_read_variance");
        for (size_t i = 0; i < var.size(); i++) vp[4 * i] = var[i];
        const std::string path = o.aov + "_variance.pfm";
        if (rmr_encode_pfm(vp.data(), W, H, path.c_str()) != RMR_OK) {
            std::cerr << "--aov: cannot write " << path << std::endl;
            return false;
        }
        if (!o.quiet) std::cout << "Saved plane as: " << path << std::endl;
    }
    if (o.adaptive < 0) return true;
    // --adaptive: PREFIX_spp.pfm (R = the pixel's tile's sample count) and PREFIX_error.pfm (R = its tile error)
    const int TX = (W + 7) / 8, TY = (H + 7) / 8;
    std::vector<uint32_t> counts((size_t)TX * TY);
    std::vector<float> err((size_t)TX * TY);
    if (rmr_read_sample_counts(c, counts.data(), counts.size() * sizeof(uint32_t)) != RMR_OK)
        return fail("rmr_read_sample_counts");
    if (rmr_tile_error(c, adaptive_params(o).offset, err.data(), err.size() * sizeof(float)) != RMR_OK)
        return fail("rmr_tile_error");
    std::vector<float> spp(n, 0.0f), ep(n, 0.0f);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t t = (size_t)(y / 8) * TX + x / 8, i = 4 * ((size_t)y * W + x);
            spp[i] = (float)counts[t];
            ep[i] = err[t];
        }
    const struct { const char* name; const std::vector<float>* img; } more[] = {{"_spp.pfm", &spp}, {"_error.pfm", &ep}};
    for (const auto& f : more) {
        const std::string path = o.aov + f.name;
        if (rmr_encode_pfm(f.img->data(), W, H, path.c_str()) != RMR_OK) {
            std::cerr << "--aov: cannot write " << path << std::endl;
            return false;
        }
        if (!o.quiet) std::cout << "Saved plane as: " << path << std::endl;
    }
    return true;
}

// --sampled-aov PREFIX: the render's own sample schedule folded into the sampled AOVs (rmr_render_aov), the
// resolved planes as float images: PREFIX_alpha.pfm (R = alpha, G = samples, B = hits), PREFIX_depth.pfm
// (R = mean t, G = min t), PREFIX_normal.pfm, PREFIX_position.pfm (the planes' xyz) and PREFIX_ids.pfm
// (R, G = id0, coverage0; B = id1)
bool write_sampled_aovs(const Options& o) {
    rmr_ctx* c = Graphics::context();
    const int W = (int)Graphics::getImageSize().x, H = (int)Graphics::getImageSize().y;
    auto fail = [&](const std::string& what) {
        std::cerr << "--sampled-aov: " << what << ": " << rmr_last_error(c) << std::endl;
        return false;
    };
    const unsigned ns = o.samples > 0 ? (unsigned)o.samples : (unsigned)o.passes;
    std::vector<float> times(ns);
    for (unsigned s = 0; s < ns; s++) times[s] = seed_time(o.frame, s);
    if (rmr_render_aov(c, ns ? times.data() : nullptr, ns, 0, 0, W, H, 1) != RMR_OK) return fail("rmr_render_aov");
    const size_t n = (size_t)W * H * 4;
    std::vector<float> depth(n), nrm(n), pos(n), ids(n), alpha(n, 0.0f);
    if (rmr_read_aov_resolved(c, RMR_AOV_R_DEPTH, depth.data(), n * sizeof(float)) != RMR_OK ||
        rmr_read_aov_resolved(c, RMR_AOV_R_NORMAL, nrm.data(), n * sizeof(float)) != RMR_OK ||
        rmr_read_aov_resolved(c, RMR_AOV_R_POSITION, pos.data(), n * sizeof(float)) != RMR_OK ||
        rmr_read_aov_resolved(c, RMR_AOV_R_IDS01, ids.data(), n * sizeof(float)) != RMR_OK)
        return fail("rmr_read_aov_resolved");
    for (size_t i = 0; i < (size_t)W * H; i++) {
        alpha[4 * i] = depth[4 * i + 2];
        alpha[4 * i + 1] = depth[4 * i + 3];
        alpha[4 * i + 2] = pos[4 * i + 3];
        depth[4 * i + 2] = 0.0f;
    }
    const struct { const char* name; const std::vector<float>* img; } files[] = {
        {"_alpha.pfm", &alpha}, {"_depth.pfm", &depth}, {"_normal.pfm", &nrm}, {"_position.pfm", &pos}, {"_ids.pfm", &ids}};
    for (const auto& f : files) {
        const std::string path = o.sampled_aov + f.name;
        if (rmr_encode_pfm(f.img->data(), W, H, path.c_str()) != RMR_OK) {
            std::cerr << "--sampled-aov: cannot write " << path << std::endl;
            return false;
        }
        if (!o.quiet) std::cout << "Saved plane as: " << path << std::endl;
    }
    return true;
}

// The lattice of --mesh-bounds and --mesh-grid: the spacing is the longest side over N, the longest side has
// N cells and the other sides are rounded up to whole cells; the origin is the bounds' lower corner.
rmr_volume_desc box_lattice(const double bounds[6], int grid) {
    rmr_volume_desc d;
    double longest = 0.0;
    int which = 0;
    for (int a = 0; a < 3; a++) {
        const double side = bounds[3 + a] - bounds[a];
        if (side > longest) { longest = side; which = a; }
        d.origin[a] = (float)bounds[a];
    }
    d.spacing = (float)(longest / (double)grid);
    for (int a = 0; a < 3; a++) {
        const double cells = std::ceil((bounds[3 + a] - bounds[a]) / (double)d.spacing);
        d.n[a] = a == which ? grid + 1 : (int)std::fmin(std::fmax(cells, 1.0), 1e6) + 1;
    }
    return d;
}
rmr_volume_desc mesh_lattice(const Options& o) { return box_lattice(o.mesh_bounds, o.mesh_grid); }
// --probe-bounds and --probe-grid state their lattice the same way
rmr_volume_desc probe_lattice(const Options& o) { return box_lattice(o.probe_bounds, o.probe_grid); }

// --probes FILE: rmr_bake_probe_field over that lattice with --probe-samples seeds of the render's schedule,
// written as the line "RMRPROBES 1 nx ny nz ox oy oz spacing" (floats as %.9g) and the points' 28 little-endian
// float32 each (raymarchrenderer_amd.load_probes reads it). With --probe-visibility K[:RANGE]: the field's
// visibility maps as well (rmr_bake_probe_field_visibility with the schedule's first K seeds), the line
// "RMRPROBES 2 nx ny nz ox oy oz spacing 8 range" and, after the sh payload, the points' 128 float32 each.
bool write_probes(const Options& o) {
    rmr_ctx* c = Graphics::context();
    auto fail = [&](const std::string& what) {
        std::cerr << "--probes: " << what << ": " << rmr_last_error(c) << std::endl;
        return false;
    };
    const rmr_volume_desc d = probe_lattice(o);
    std::vector<float> times((size_t)o.probe_samples);
    for (int s = 0; s < o.probe_samples; s++) times[(size_t)s] = seed_time(o.frame, (unsigned)s);
    if (rmr_bake_probe_field(c, &d, times.data(), (uint32_t)o.probe_samples, nullptr) != RMR_OK) return fail("rmr_bake_probe_field");
    std::vector<float> sh((size_t)d.n[0] * (size_t)d.n[1] * (size_t)d.n[2] * 28);
    if (rmr_read_probe_field(c, nullptr, sh.data()) != RMR_OK) return fail("rmr_read_probe_field");
    std::vector<float> vis;
    const float range = o.probe_vis_range > 0.0f ? o.probe_vis_range : 2.6f * d.spacing;
    if (o.probe_vis > 0) {
        std::vector<float> vt((size_t)o.probe_vis);
        for (int s = 0; s < o.probe_vis; s++) vt[(size_t)s] = seed_time(o.frame, (unsigned)s);
        if (rmr_bake_probe_field_visibility(c, vt.data(), (uint32_t)o.probe_vis, range) != RMR_OK)
            return fail("rmr_bake_probe_field_visibility");
        vis.resize(sh.size() / 28 * 128);
        if (rmr_read_probe_field_visibility(c, vis.data(), nullptr) != RMR_OK) return fail("rmr_read_probe_field_visibility");
    }
    const uint16_t one = 1;
    unsigned char first;
    std::memcpy(&first, &one, 1);
    std::FILE* f = first == 1 ? std::fopen(o.probes.c_str(), "wb") : nullptr;   // (the floats are written as they lie in memory)
    bool ok = f != nullptr;
    if (f) {
        std::fprintf(f, "RMRPROBES %d %d %d %d %.9g %.9g %.9g %.9g", o.probe_vis > 0 ? 2 : 1, d.n[0], d.n[1], d.n[2], d.origin[0],
                     d.origin[1], d.origin[2], d.spacing);
        if (o.probe_vis > 0) std::fprintf(f, " 8 %.9g", range);
        std::fprintf(f, "\n");
        ok = std::fwrite(sh.data(), sizeof(float), sh.size(), f) == sh.size();
        ok = (vis.empty() || std::fwrite(vis.data(), sizeof(float), vis.size(), f) == vis.size()) && ok;
        ok = (std::fclose(f) == 0) && ok;
    }
    if (!ok) {
        std::cerr << "--probes: cannot write " << o.probes << std::endl;
        return false;
    }
    if (!o.quiet) std::printf("probes: %d x %d x %d at spacing %.6g, %d samples each -> %s\n", d.n[0], d.n[1], d.n[2], d.spacing,
                              o.probe_samples, o.probes.c_str());
    if (!o.quiet && o.probe_vis > 0) std::printf("probes: visibility maps from %d samples each, range %.6g\n", o.probe_vis, range);
    return true;
}

// --mesh FILE: rmr_extract_mesh over that lattice with normals and material ids, written as OBJ (v, vn, f) or
// binary PLY (x y z nx ny nz material). --mesh-bake N: rmr_bake_mesh with the render's seed schedule, the
// PLY's vertex colours being the display's sRGB bytes of the baked radiance; with :AO_DISTANCE the radiance
// times the occlusion within that distance (the product rounded to float32).
bool write_mesh(const Options& o) {
    rmr_ctx* c = Graphics::context();
    auto fail = [&](const std::string& what) {
        std::cerr << "--mesh: " << what << ": " << rmr_last_error(c) << std::endl;
        return false;
    };
    const rmr_volume_desc d = mesh_lattice(o);
    const rmr_mesh_params mp = {o.mesh_iso, RMR_MESH_NORMALS | RMR_MESH_IDS};
    rmr_mesh_info info = {0, 0};
    if (rmr_extract_mesh(c, &d, &mp, &info) != RMR_OK) return fail("rmr_extract_mesh");
    std::vector<float> v(3 * (size_t)info.n_vertices), n(3 * (size_t)info.n_vertices), ids((size_t)info.n_vertices);
    std::vector<uint32_t> q(4 * (size_t)info.n_quads);
    if (rmr_read_mesh(c, v.data(), n.data(), ids.data(), q.data()) != RMR_OK) return fail("rmr_read_mesh");
    std::vector<uint8_t> rgb8;
    if (o.mesh_bake > 0) {
        const size_t nv = (size_t)info.n_vertices;
        std::vector<float> times((size_t)o.mesh_bake), rgba(4 * nv), ao(nv), rgb(3 * nv);
        for (int s = 0; s < o.mesh_bake; s++) times[(size_t)s] = seed_time(o.frame, (unsigned)s);
        rmr_bake_params bp;
        rmr_default_bake_params(&bp);
        // surface-nets vertices lie off the surface by a fraction of a cell (inside a convex shape): lift the rays'
        // origins past that, or every ray of such a vertex starts inside the shape
        bp.bias = 0.002f + 0.125f * d.spacing;
        if (o.mesh_bake_ao) {
            bp.flags |= RMR_BAKE_AO;
            bp.ao_distance = o.mesh_bake_ao_distance;
        }
        if (rmr_bake_mesh(c, times.data(), (uint32_t)o.mesh_bake, &bp) != RMR_OK) return fail("rmr_bake_mesh");
        if (rmr_read_mesh_bake(c, rgba.data(), o.mesh_bake_ao ? ao.data() : nullptr) != RMR_OK) return fail("rmr_read_mesh_bake");
        for (size_t i = 0; i < nv; i++)
            for (int k = 0; k < 3; k++) rgb[3 * i + (size_t)k] = o.mesh_bake_ao ? rgba[4 * i + (size_t)k] * ao[i] : rgba[4 * i + (size_t)k];
        rgb8.resize(3 * nv);
        if (rmr_srgb8_pixels(rgb.data(), nv, rgb8.data()) != RMR_OK) return fail("rmr_srgb8_pixels");
    }
    const int rc = o.mesh_bake > 0 ? rmr_encode_ply_colors(o.mesh.c_str(), v.data(), n.data(), ids.data(), rgb8.data(),
                                                           (size_t)info.n_vertices, q.data(), (size_t)info.n_quads)
                   : o.mesh_ply ? rmr_encode_ply(o.mesh.c_str(), v.data(), n.data(), ids.data(), (size_t)info.n_vertices, q.data(), (size_t)info.n_quads)
                              : rmr_encode_obj(o.mesh.c_str(), v.data(), n.data(), (size_t)info.n_vertices, q.data(), (size_t)info.n_quads);
    if (rc != RMR_OK) {
        std::cerr << "--mesh: cannot write " << o.mesh << std::endl;
        return false;
    }
    if (!o.quiet)
        std::cout << "Saved mesh as: " << o.mesh << " (" << info.n_vertices << " vertices, " << info.n_quads << " quads, lattice "
                  << d.n[0] << "x" << d.n[1] << "x" << d.n[2] << ", spacing " << d.spacing << ")" << std::endl;
    return true;
}

void report(const Options& o, const RenderResult& r) {
    std::cout << "Render Time: " << r.seconds << std::endl;  // Program.cpp:297
    if (!o.quiet && r.seconds > 0)
        std::printf("{\"samples\": %llu, \"seconds\": %.6f, \"msamples_per_s\": %.3f}\n", r.samples, r.seconds,
                    r.samples / r.seconds / 1e6);
}

std::vector<std::string> list_scenes(const std::string& dir) {  // CLI.cpp:9-36 listNames
    std::vector<std::string> out;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d)) {
            std::string n = e->d_name;
            if (n.size() > 6 && n.find(".scene") != std::string::npos) out.push_back(dir + "/" + n);
        }
        closedir(d);
    }
    std::sort(out.begin(), out.end());
    return out;
}

bool read_int(int* dst) {
    std::string in;
    if (!(std::cin >> in)) return false;
    try {
        *dst = std::stoi(in);
    } catch (const std::exception&) {
        std::cout << "ERROR: Invalid Number" << std::endl;
    }
    return true;
}

// CLI.cpp:176-218: load_scene / samples / grid_width / grid_height / render / save (+ quit)
int interactive(Options o) {
    bool will_save = false;
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "load_scene") {
            const auto paths = list_scenes(o.scene_dir);
            for (size_t i = 0; i < paths.size(); i++)
                std::cout << "[" << i << "] " << paths[i].substr(paths[i].find_last_of('/') + 1) << std::endl;
            int idx = -1;
            if (!read_int(&idx)) break;
            if (idx < 0 || idx >= (int)paths.size()) {
                std::cout << "ERROR: Out of Range" << std::endl;
                continue;
            }
            load_scene(paths[idx]);
        } else if (cmd == "samples") {
            std::cout << "Enter number:" << std::endl;
            if (!read_int(&o.samples)) break;
        } else if (cmd == "grid_width") {
            std::cout << "Enter number:" << std::endl;
            if (!read_int(&o.grid_w)) break;
        } else if (cmd == "grid_height") {
            std::cout << "Enter number:" << std::endl;
            if (!read_int(&o.grid_h)) break;
        } else if (cmd == "render") {
            report(o, render(o, 0));
            if (will_save) {
                save(o);
                will_save = false;
            }
        } else if (cmd == "save") {
            will_save = true;
            if (Graphics::context()) {
                save(o);
                will_save = false;
            }
        } else if (cmd == "quit" || cmd == "exit") {
            break;
        } else {
            std::cout << "Unknown command: " << cmd << std::endl;
        }
    }
    return 0;
}

void usage() {
    std::puts(
        "rmr_cli — headless driver of the rmr SDF ray-march path tracer (Program.cpp / CLI.cpp)\n"
        "  --scene FILE        scene JSON (v1 format for rm1, v2 for rm2); none = RayMarch3 built-in\n"
        "  --variant rm1|rm2|rm3   (default rm1 with --scene, rm3 without)\n"
        "  --size WxH          image size (default 800x600)\n"
        "  --samples N         spp per tile (default 128); 0 = progressive\n"
        "  --passes P          progressive passes (default 16)\n"
        "  --grid GWxGH        tile grid (default 4x4)\n"
        "  --bounces B --max-steps N --max-dist D --step-mult S --separate-channels 0|1\n"
        "  --camera ex,ey,ez,dx,dy,dz   (default 0,4,-6,0,-3,6)\n"
        "  --camera thinlens:APERTURE,FOCUS | equirect | ortho:WIDTH,HEIGHT   the camera model (rmr.h\n"
        "                      rmr_camera_model; both forms of --camera may be given); not with --gpus / --devices\n"
        "  --env-map FILE WxH  raw RGBA8 envTex for skyColor (row 0 = up); enables useEnvTex\n"
        "  --frame F           seed schedule frame: time = 1000 F + 0.016 s\n"
        "  --per-sample        one Graphics::Render launch per sample per tile (reference pattern)\n"
        "  --out FILE.bmp      (default output/<timestamp>.bmp)\n"
        "  --denoise [N]       after the render, filter the image with N a-trous iterations (0..8, default 5)\n"
        "                      and write --out from the denoised image\n"
        "  --variance-guided [SIGMA_L]  with --denoise: the variance-guided filter (luminance weight of\n"
        "                      SIGMA_L standard deviations, default 4; safe at any sample count); keeps the\n"
        "                      error estimate on from the first sample; --aov adds PREFIX_variance.pfm\n"
        "  --bloom [THRESHOLD[:INTENSITY]]  after the render (and --denoise), before --tonemap: spread the part of\n"
        "                      the image above THRESHOLD (scene units, default 1) over a five-level pyramid and\n"
        "                      add INTENSITY (default 0.2) of it back; --tonemap then reads the bloom image, and\n"
        "                      without --tonemap --out is written from it; not with --gpus / --devices\n"
        "  --tonemap linear|reinhard[:WHITE]|aces   after the render (and --denoise): tone-map the image with\n"
        "                      that curve (reinhard's white point, default 4) and write --out from the result\n"
        "  --exposure EV|auto[:KEY]   the stage's exposure: EV stops (scale 2^EV, |EV| <= 32), or metered from\n"
        "                      the luminance histogram so that the image's log-average goes to KEY (default\n"
        "                      0.18); alone it implies --tonemap aces; not with --gpus / --devices\n"
        "  --aov PREFIX        first-hit planes as float PFM: PREFIX_normal.pfm, PREFIX_position.pfm,\n"
        "                      PREFIX_ray.pfm, PREFIX_depth_id.pfm (R = t, G = material id or -1, B = 0)\n"
        "  --sampled-aov PREFIX  the render's own samples' first hits folded per pixel (anti-aliased, every\n"
        "                      --camera model): PREFIX_alpha.pfm (R = alpha, G = samples, B = hits),\n"
        "                      PREFIX_depth.pfm (R = mean t, G = min t), PREFIX_normal.pfm, PREFIX_position.pfm,\n"
        "                      PREFIX_ids.pfm (R, G = id0, coverage0; B = id1); not with --gpus / --devices\n"
        "  --mesh FILE.obj|FILE.ply  after the render: the scene's surface as a quad mesh (surface nets over a\n"
        "                      lattice of distance samples, rmr.h rmr_extract_mesh) with normals and, in PLY,\n"
        "                      material ids; needs --mesh-bounds; not with --gpus / --devices or --interactive\n"
        "  --mesh-bounds x0,y0,z0,x1,y1,z1   the box that is meshed (required: a scene has no finite box of its\n"
        "                      own); a surface that leaves it is cut open there\n"
        "  --mesh-grid N       cells along the box's longest side (1..4095, default 128); the spacing is that\n"
        "                      side over N, the other sides are rounded up to whole cells\n"
        "  --mesh-iso V        the level that is meshed (default 0; V > 0 grows the shape)\n"
        "  --mesh-bake N[:AO_DISTANCE]  bake N samples of light per vertex (rmr.h rmr_bake_mesh; seeds of --frame)\n"
        "                      into the PLY's uchar red green blue (the display's sRGB encode); with AO_DISTANCE\n"
        "                      (> 0 or inf) the colour is the radiance times the occlusion within it; the rays\n"
        "                      start 0.002 + an eighth of the lattice spacing off the vertex; needs --mesh FILE.ply\n"
        "  --probes FILE       after the render: a field of irradiance probes (rmr.h rmr_bake_probe_field: nine\n"
        "                      spherical harmonics per channel at a lattice's points) as 'RMRPROBES 1 nx ny nz ox oy\n"
        "                      oz spacing' and 28 float32 per point; needs --probe-bounds; not with --gpus /\n"
        "                      --devices or --interactive\n"
        "  --probe-bounds x0,y0,z0,x1,y1,z1   the box the lattice spans\n"
        "  --probe-grid N      cells along the box's longest side (1..4095, default 8), as --mesh-grid\n"
        "  --probe-samples K   seeds per probe (1..2^24, default 256; seeds of --frame)\n"
        "  --probe-visibility K[:RANGE]   with --probes: the probes' visibility maps as well (rmr.h\n"
        "                      rmr_bake_probe_field_visibility: 8 x 8 octahedral depth moments per probe from K seeds,\n"
        "                      1..2^24; RANGE finite and > 0, default 2.6 x spacing); the file becomes 'RMRPROBES 2 ...\n"
        "                      spacing 8 range' with 128 more float32 per point after the sh payload\n"
        "  --adaptive T        adaptive sampling: render until every block's tile error is <= T, at most\n"
        "                      --samples per pixel, over the whole image; prints passes, mean spp, open tiles\n"
        "                      and max error; with --aov also PREFIX_spp.pfm (R = samples) and PREFIX_error.pfm\n"
        "  --min-samples N     adaptive: samples everywhere before the first estimate (default 16, >= 2)\n"
        "  --pass-samples N    adaptive: samples per further pass on the open blocks (default 16)\n"
        "  --checkpoint FILE   write the float accumulator at the end; --resume FILE continue from one\n"
        "  --device N  --interactive (CLI.cpp commands on stdin)  --scene-dir DIR  --quiet\n"
        "  --gpus N | --devices a,b,..  the frame tile-partitioned over those GPUs (one process, RCCL reduce)");
}

// --camera's model form: thinlens:APERTURE,FOCUS | equirect | ortho:WIDTH,HEIGHT | view. False when the
// argument is none of them (the numbers' ranges are checked by rmr_check_camera_model afterwards).
bool camera_model_arg(const std::string& v, rmr_camera_model& m) {
    char tail = 0;
    float a = 0, b = 0;
    if (v == "equirect" || v == "view") {
        m.model = v == "view" ? RMR_CAMERA_VIEW : RMR_CAMERA_EQUIRECT;
        return true;
    }
    if (std::sscanf(v.c_str(), "thinlens:%f,%f%c", &a, &b, &tail) == 2) {
        m.model = RMR_CAMERA_THIN_LENS;
        m.aperture = a;
        m.focus = b;
        return true;
    }
    if (std::sscanf(v.c_str(), "ortho:%f,%f%c", &a, &b, &tail) == 2) {
        m.model = RMR_CAMERA_ORTHO;
        m.width = a;
        m.height = b;
        return true;
    }
    return false;
}

// "NAME" or "NAME:NUMBER" (the whole of v): false for anything else. has_num: the number was given.
bool name_and_number(const std::string& v, const char* name, float& num, bool& has_num) {
    const size_t n = std::strlen(name);
    has_num = false;
    if (v.compare(0, n, name) != 0) return false;
    if (v.size() == n) return true;
    if (v[n] != ':') return false;
    char* end = nullptr;
    const char* t = v.c_str() + n + 1;
    num = std::strtof(t, &end);
    has_num = true;
    return end != t && *end == '\0';
}

bool parse(int argc, char** argv, Options& o) {
    rmr_default_params(&o.params);
    rmr_default_tonemap_params(&o.tone);
    rmr_default_bloom_params(&o.bloom_p);
    rmr_default_camera_model(&o.model);
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&](const char* name) -> const char* {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "missing value for %s\n", name);
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "--scene") o.scene = next("--scene");
        else if (a == "--variant") {
            const std::string v = next("--variant");
            o.variant = v == "rm1" ? RMR_VARIANT_RM1 : v == "rm2" ? RMR_VARIANT_RM2 : v == "rm3" ? RMR_VARIANT_RM3 : -2;
            if (o.variant == -2) return false;
        } else if (a == "--size") {
            if (std::sscanf(next("--size"), "%dx%d", &o.width, &o.height) != 2) return false;
        } else if (a == "--samples") o.samples = std::atoi(next("--samples"));
        else if (a == "--passes") o.passes = std::atoi(next("--passes"));
        else if (a == "--grid") {
            if (std::sscanf(next("--grid"), "%dx%d", &o.grid_w, &o.grid_h) != 2) return false;
        } else if (a == "--bounces") o.params.max_bounces = std::atoi(next("--bounces"));
        else if (a == "--max-steps") o.params.max_steps = std::atoi(next("--max-steps"));
        else if (a == "--max-dist") o.params.max_dist = (float)std::atof(next("--max-dist"));
        else if (a == "--step-mult") o.params.step_multiply = (float)std::atof(next("--step-mult"));
        else if (a == "--separate-channels") o.params.separate_channels = std::atoi(next("--separate-channels"));
        else if (a == "--camera") {
            const std::string v = next("--camera");
            if (camera_model_arg(v, o.model)) continue;   // a model; else the eye and the direction
            double* c = o.cam;
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf,%lf,%lf,%lf", c, c + 1, c + 2, c + 3, c + 4, c + 5) != 6)
                return false;
            o.have_camera = true;
        } else if (a == "--frame") o.frame = std::atoi(next("--frame"));
        else if (a == "--per-sample") o.per_sample = true;
        else if (a == "--out") o.out = next("--out");
        else if (a == "--denoise") {   // the count is optional: taken when the next argument is a number
            o.denoise = 5;
            if (i + 1 < argc && argv[i + 1][0] != '\0' && std::strspn(argv[i + 1], "0123456789") == std::strlen(argv[i + 1])) {
                o.denoise = std::atoi(argv[++i]);
                if (o.denoise > 8 || std::strlen(argv[i]) > 2) return false;
            }
        } else if (a == "--variance-guided") {   // SIGMA_L is optional: taken when the next argument is no option
            o.variance_guided = 4.0;
            if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) {
                char* end = nullptr;
                const char* v = argv[++i];
                o.variance_guided = std::strtod(v, &end);
                if (end == v || *end != '\0' || !std::isfinite(o.variance_guided) || !(o.variance_guided > 0) ||
                    !std::isfinite((float)o.variance_guided) || !((float)o.variance_guided > 0.0f))
                    return false;
            }
        } else if (a == "--bloom") {   // the value is optional: taken when the next argument is no option
            o.bloom = true;
            if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) {
                const char* v = argv[++i];
                char* end = nullptr;
                o.bloom_p.threshold = std::strtof(v, &end);
                if (end == v) return false;
                if (*end == ':') {
                    const char* w = end + 1;
                    o.bloom_p.intensity = std::strtof(w, &end);
                    if (end == w) return false;
                }
                if (*end != '\0') return false;
            }
        } else if (a == "--tonemap") {
            const std::string v = next("--tonemap");
            float white = 0.0f;
            bool has = false;
            if (v == "linear") o.tone.curve = RMR_TONE_LINEAR;
            else if (v == "aces") o.tone.curve = RMR_TONE_ACES;
            else if (name_and_number(v, "reinhard", white, has)) {
                o.tone.curve = RMR_TONE_REINHARD;
                if (has) o.tone.white = white;
            } else return false;
            o.tonemap = true;
        } else if (a == "--exposure") {
            const std::string v = next("--exposure");
            float key = 0.0f;
            bool has = false;
            if (name_and_number(v, "auto", key, has)) {
                o.tone.auto_exposure = 1;
                if (has) o.tone.key = key;
            } else {
                char* end = nullptr;
                o.tone.auto_exposure = 0;
                o.tone.exposure_ev = std::strtof(v.c_str(), &end);
                if (end == v.c_str() || *end != '\0') return false;
            }
            o.tonemap = true;
        } else if (a == "--aov") {
            o.aov = next("--aov");
            if (o.aov.empty()) return false;
        }
        else if (a == "--sampled-aov") {
            o.sampled_aov = next("--sampled-aov");
            if (o.sampled_aov.empty()) return false;
        }
        else if (a == "--mesh") {
            o.mesh = next("--mesh");
            const size_t dot = o.mesh.rfind('.');
            const std::string ext = dot == std::string::npos ? "" : o.mesh.substr(dot);
            if (ext != ".obj" && ext != ".ply") return false;
            o.mesh_ply = ext == ".ply";
        } else if (a == "--mesh-bounds") {
            char tail = 0;
            double* b = o.mesh_bounds;
            if (std::sscanf(next("--mesh-bounds"), "%lf,%lf,%lf,%lf,%lf,%lf%c", b, b + 1, b + 2, b + 3, b + 4, b + 5, &tail) != 6)
                return false;
            for (int k = 0; k < 3; k++)
                if (!std::isfinite((float)b[k]) || !std::isfinite((float)b[3 + k]) || !(b[3 + k] > b[k])) return false;
            o.have_mesh_bounds = true;
        } else if (a == "--mesh-grid") {
            char* end = nullptr;
            const char* v = next("--mesh-grid");
            const long n = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 1 || n > 4095) return false;
            o.mesh_grid = (int)n;
            o.have_mesh_opts = true;
        } else if (a == "--mesh-iso") {
            char* end = nullptr;
            const char* v = next("--mesh-iso");
            o.mesh_iso = std::strtof(v, &end);
            if (end == v || *end != '\0' || !std::isfinite(o.mesh_iso)) return false;
            o.have_mesh_opts = true;
        } else if (a == "--probes") {
            o.probes = next("--probes");
            if (o.probes.empty()) return false;
        } else if (a == "--probe-bounds") {
            char tail = 0;
            double* b = o.probe_bounds;
            if (std::sscanf(next("--probe-bounds"), "%lf,%lf,%lf,%lf,%lf,%lf%c", b, b + 1, b + 2, b + 3, b + 4, b + 5, &tail) != 6)
                return false;
            for (int k = 0; k < 3; k++)
                if (!std::isfinite((float)b[k]) || !std::isfinite((float)b[3 + k]) || !(b[3 + k] > b[k])) return false;
            o.have_probe_bounds = true;
        } else if (a == "--probe-grid") {
            char* end = nullptr;
            const char* v = next("--probe-grid");
            const long n = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 1 || n > 4095) return false;
            o.probe_grid = (int)n;
            o.have_probe_opts = true;
        } else if (a == "--probe-samples") {
            char* end = nullptr;
            const char* v = next("--probe-samples");
            const long n = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 1 || n > (1L << 24)) return false;
            o.probe_samples = (int)n;
            o.have_probe_opts = true;
        } else if (a == "--probe-visibility") {
            char* end = nullptr;
            const char* v = next("--probe-visibility");
            const long n = std::strtol(v, &end, 10);
            if (end == v || n < 1 || n > (1L << 24)) return false;
            o.probe_vis = (int)n;
            if (*end == ':') {
                const char* rv = end + 1;
                o.probe_vis_range = std::strtof(rv, &end);
                if (end == rv || *end != '\0' || !std::isfinite(o.probe_vis_range) || !(o.probe_vis_range > 0.0f)) return false;
            } else if (*end != '\0') {
                return false;
            }
            o.have_probe_opts = true;
        } else if (a == "--mesh-bake") {
            char* end = nullptr;
            const char* v = next("--mesh-bake");
            const long n = std::strtol(v, &end, 10);
            if (end == v || n < 1 || n > (1L << 24)) return false;
            o.mesh_bake = (int)n;
            if (*end == ':') {
                const char* w = end + 1;
                o.mesh_bake_ao_distance = std::strtof(w, &end);
                if (end == w || *end != '\0' || !(o.mesh_bake_ao_distance > 0.0f)) return false;
                o.mesh_bake_ao = true;
            } else if (*end != '\0') {
                return false;
            }
        }
        else if (a == "--adaptive") {
            char* end = nullptr;
            const char* v = next("--adaptive");
            o.adaptive = std::strtod(v, &end);
            if (end == v || *end != '\0' || !std::isfinite(o.adaptive) || o.adaptive < 0) return false;
        } else if (a == "--min-samples") o.min_samples = std::atoi(next("--min-samples"));
        else if (a == "--pass-samples") o.pass_samples = std::atoi(next("--pass-samples"));
        else if (a == "--checkpoint") o.checkpoint = next("--checkpoint");
        else if (a == "--resume") o.resume = next("--resume");
        else if (a == "--device") o.device = std::atoi(next("--device"));
        else if (a == "--gpus") {
            const int n = std::atoi(next("--gpus"));
            if (n <= 0) return false;
            o.devices.clear();
            for (int d = 0; d < n; d++) o.devices.push_back(d);
        } else if (a == "--devices") {
            std::stringstream ss(next("--devices"));
            std::string item;
            o.devices.clear();
            while (std::getline(ss, item, ',')) o.devices.push_back(std::atoi(item.c_str()));
            if (o.devices.empty()) return false;
        }
        else if (a == "--interactive") o.interactive = true;
        else if (a == "--scene-dir") o.scene_dir = next("--scene-dir");
        else if (a == "--quiet") o.quiet = true;
        else if (a == "--env-map") {  // raw RGBA8 file + its size: skyColor's envTex, enables useEnvTex
            o.env_map = next("--env-map");
            if (std::sscanf(next("--env-map size"), "%dx%d", &o.env_w, &o.env_h) != 2) return false;
            o.params.use_env_tex = 1;
        }
        else if (a == "--print-tiles") o.print_tiles = true;
        else if (a == "--print-view") o.print_view = true;
        else if (a == "--help" || a == "-h") {
            usage();
            std::exit(0);
        } else {
            std::fprintf(stderr, "unknown option %s\n", a.c_str());
            return false;
        }
    }
    if (o.variant < 0) o.variant = (o.scene.empty() && !o.interactive) ? RMR_VARIANT_RM3 : RMR_VARIANT_RM1;
    if (o.width <= 0 || o.height <= 0 || o.grid_w <= 0 || o.grid_h <= 0 || o.samples < 0 || o.passes < 0)
        return false;
    if (rmr_check_camera_model(&o.model) != RMR_OK) {
        std::fprintf(stderr, "--camera: thinlens needs APERTURE >= 0 and FOCUS > 0, ortho WIDTH > 0 and HEIGHT > 0\n");
        return false;
    }
    if (rmr_check_tonemap_params(&o.tone) != RMR_OK) {
        std::fprintf(stderr, "--tonemap / --exposure: reinhard needs WHITE > 0, auto KEY > 0, and |EV| <= 32\n");
        return false;
    }
    if (rmr_check_bloom_params(&o.bloom_p) != RMR_OK) {
        std::fprintf(stderr, "--bloom: THRESHOLD and INTENSITY are finite and >= 0\n");
        return false;
    }
    if (o.mesh.empty() ? (o.have_mesh_bounds || o.have_mesh_opts) : !o.have_mesh_bounds) {
        std::fprintf(stderr, "--mesh FILE.obj|FILE.ply needs --mesh-bounds x0,y0,z0,x1,y1,z1 (and they need --mesh)\n");
        return false;
    }
    if (o.mesh_bake > 0 && (o.mesh.empty() || !o.mesh_ply)) {
        std::fprintf(stderr, "--mesh-bake needs --mesh FILE.ply (an OBJ has no vertex colours)\n");
        return false;
    }
    if (!o.mesh.empty()) {
        const rmr_volume_desc d = mesh_lattice(o);
        const char* bad = nullptr;
        if (rmr_check_volume(&d, &bad) != RMR_OK) {
            std::fprintf(stderr, "--mesh-bounds / --mesh-grid: the lattice's %s is out of range\n", bad);
            return false;
        }
    }
    if (o.probes.empty() ? (o.have_probe_bounds || o.have_probe_opts) : !o.have_probe_bounds) {
        std::fprintf(stderr, "--probes FILE needs --probe-bounds x0,y0,z0,x1,y1,z1 (and they need --probes)\n");
        return false;
    }
    if (!o.probes.empty()) {
        const rmr_volume_desc d = probe_lattice(o);
        const char* bad = nullptr;
        if (rmr_check_volume(&d, &bad) != RMR_OK) {
            std::fprintf(stderr, "--probe-bounds / --probe-grid: the lattice's %s is out of range\n", bad);
            return false;
        }
    }
    if (o.adaptive >= 0 && (o.min_samples < 2 || o.pass_samples < 1 || o.samples < o.min_samples)) {
        std::fprintf(stderr, "--adaptive: --min-samples >= 2, --pass-samples >= 1 and --samples >= --min-samples\n");
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    if (!parse(argc, argv, o)) {
        usage();
        return 2;
    }
    if (o.print_tiles) {  // the spiral tile order, one "x y" per line
        for (auto t : tile_spiral(o.grid_w, o.grid_h)) std::printf("%d %d\n", t.first, t.second);
        return 0;
    }
    if (o.print_view) {  // Camera corner rays (camera names: ray00 ray10 ray01 ray11), %.9g
        Camera cam(Vector3(o.cam[0], o.cam[1], o.cam[2]), Vector3(o.cam[3], o.cam[4], o.cam[5]).normalized(),
                   (float)((double)o.width / (double)o.height), PI / 4);
        Vector3 r[4];
        cam.getRays(r[0], r[1], r[2], r[3]);
        for (auto& v : r) std::printf("%.9g %.9g %.9g\n", v.x, v.y, v.z);
        return 0;
    }
    if (o.adaptive >= 0 && (!o.devices.empty() || !o.resume.empty() || o.per_sample || o.interactive)) {
        std::fprintf(stderr, "--adaptive: not with --gpus / --devices, --resume, --per-sample or --interactive\n");
        return 2;
    }
    if (o.variance_guided > 0 && (o.denoise < 0 || !o.devices.empty() || !o.resume.empty() || o.per_sample)) {
        std::fprintf(stderr, "--variance-guided: needs --denoise; not with --gpus / --devices, --resume or --per-sample\n");
        return 2;
    }
    if (o.tonemap && (!o.devices.empty() || o.interactive)) {
        std::fprintf(stderr, "--tonemap / --exposure: not with --gpus / --devices or --interactive\n");
        return 2;
    }
    if (o.bloom && (!o.devices.empty() || o.interactive)) {
        std::fprintf(stderr, "--bloom: not with --gpus / --devices or --interactive\n");
        return 2;
    }
    if (o.model.model != RMR_CAMERA_VIEW && !o.devices.empty()) {
        std::fprintf(stderr, "--camera MODEL: not with --gpus / --devices (the device group keeps the view's own rays)\n");
        return 2;
    }
    if ((o.model.model == RMR_CAMERA_EQUIRECT || o.model.model == RMR_CAMERA_ORTHO) && (o.denoise >= 0 || !o.aov.empty())) {
        std::fprintf(stderr, "--camera equirect / ortho: no --denoise and no --aov (no first-hit guides for these models)\n");
        return 2;
    }
    if (!o.sampled_aov.empty() && (!o.devices.empty() || o.interactive)) {
        std::fprintf(stderr, "--sampled-aov: not with --gpus / --devices or --interactive\n");
        return 2;
    }
    if (!o.mesh.empty() && (!o.devices.empty() || o.interactive)) {
        std::fprintf(stderr, "--mesh: not with --gpus / --devices or --interactive\n");
        return 2;
    }
    if (!o.probes.empty() && (!o.devices.empty() || o.interactive)) {
        std::fprintf(stderr, "--probes: not with --gpus / --devices or --interactive\n");
        return 2;
    }
    Screen::setScreenSize(Vector2(1280, 720));  // Program.cpp:89
    Graphics::setDevice(o.device);
    if (!o.devices.empty()) {
        if (!o.checkpoint.empty() || !o.resume.empty() || o.interactive || o.denoise >= 0 || !o.aov.empty()) {
            std::fprintf(stderr, "--gpus / --devices: no checkpoint, resume, interactive mode, --denoise or --aov\n");
            return 2;
        }
        Graphics::setDevices(o.devices);
    }
    Graphics::setVariant(o.variant);
    Graphics::setImageSize(Vector2(o.width, o.height));
    if (!o.scene.empty() && !load_scene(o.scene)) return 1;
    Graphics::Init();
    if (!Graphics::context()) return 3;  // no device: fail loudly, there is no CPU path
    if (!o.interactive && Graphics::lastStatus() != RMR_OK) return 1;  // interactive: scene comes later
    Graphics::setParams(o.params);
    if (o.model.model != RMR_CAMERA_VIEW) {
        Graphics::setCameraModel(o.model);
        if (Graphics::lastStatus() != RMR_OK) return 1;
    }
    if (!o.env_map.empty()) {
        bool ok = false;
        const std::string tex = read_file(o.env_map, &ok);
        if (!ok || tex.size() != (size_t)o.env_w * o.env_h * 4) {
            std::cerr << "env map: cannot read " << o.env_w << "x" << o.env_h << " RGBA8 from " << o.env_map << std::endl;
            return 1;
        }
        Graphics::setEnvMap((const unsigned char*)tex.data(), o.env_w, o.env_h);
    }
    if (o.interactive) return interactive(o);
    const RenderResult r = render(o, 0);
    if (Graphics::lastStatus() != RMR_OK) return 1;
    report(o, r);
    if (o.denoise >= 0) {
        if (o.variance_guided > 0) Graphics::DenoiseVariance(o.denoise, (float)o.variance_guided);
        else Graphics::Denoise(o.denoise);
        if (Graphics::lastStatus() != RMR_OK) return 1;
        Graphics::setOutputSource(RMR_OUTPUT_DENOISED);
    }
    int shown = o.denoise >= 0 ? RMR_OUTPUT_DENOISED : RMR_OUTPUT_ACCUM;   // the image --out is written from
    if (o.bloom) {
        Graphics::Bloom(shown, o.bloom_p);
        if (Graphics::lastStatus() != RMR_OK) return 1;
        shown = RMR_OUTPUT_BLOOM;
        Graphics::setOutputSource(shown);
        if (Graphics::lastStatus() != RMR_OK) return 1;
    }
    if (o.tonemap) {   // last: the image --out would have been written from, through the exposure and the curve
        Graphics::Tonemap(shown, o.tone);
        if (Graphics::lastStatus() != RMR_OK) return 1;
        Graphics::setOutputSource(RMR_OUTPUT_TONEMAPPED);
        if (Graphics::lastStatus() != RMR_OK) return 1;
        if (o.tone.auto_exposure && !o.quiet) {
            double l = 0.0;
            float scale = 0.0f;
            if (Graphics::readExposure(&l, &scale)) std::printf("exposure: %+.3f stops (scale %.6g)\n", l, scale);
        }
    }
    save(o);
    int rc = Graphics::lastStatus() == RMR_OK ? 0 : 1;
    if (rc == 0 && !o.aov.empty() && !write_aovs(o)) rc = 1;
    if (rc == 0 && !o.sampled_aov.empty() && !write_sampled_aovs(o)) rc = 1;
    if (rc == 0 && !o.mesh.empty() && !write_mesh(o)) rc = 1;
    if (rc == 0 && !o.probes.empty() && !write_probes(o)) rc = 1;
    Graphics::Shutdown();
    return rc;
}
