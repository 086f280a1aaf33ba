// trail_rule_test.cpp — host check of the trailing steps' acceptance rule (rmr_trail_rule.h, the header
// trace_main compiles). Build: make trail_rule_test / trail_rule_test_san (-ffp-contract=off, as the kernels).
//
// Per scene, rays are marched as the kernel marches them (march(), stepMultiply 0.25 / 0.5 / 1.7): at every
// march point (the anchor) the approximate fold of the generated map is run — box keys first, then the
// spheres, each square root the correctly rounded one moved by -1 / 0 / +1 ulp at random, which is the
// premise the map's error bound err() is stated on — and gives w and s2. From the anchor up to fifteen
// trailing steps follow, each through trail_rule with primitive w alone, and further random steps of
// the same ray up to 1.5 |s2| ahead. Origins are random points of the scene's box, the eye, and bounce
// origins on faces, edges and corners of the boxes and on the spheres (exactly on them and 0.003 off).
//
// Checked wherever the rule accepts: the whole float opU fold at that point is (F_w, id_w) bit for bit,
// and the box form of F_w used there is sd_box / sd_sphere bit for bit. Wherever it certifies: at each of
// getNormal's six probes of the point every other primitive is strictly farther than w.
// Last line "ok"; a line "FAIL ..." per violation otherwise.
//
// trail_rule_test --scene FILE runs the same checks on one scene read from a text file instead (generated
// scenes at other scales and offsets, tests/scene_family.py write_rule_scene): the first line max_dist, then
// one line per primitive, `b|s id cx cy cz rx ry rz`, every number a C hex float; 200,000 triples. The
// origins and the march's outer limit, which the compiled-in scenes have about the origin at Cornell-5's
// size, move and scale with the file's scene (Frame).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rmr_trail_rule.h"

namespace {

struct Prim {
    bool box;
    float c[3], r[3];
    float id;
};
// where the rays start and how far a march is followed: the compiled-in scenes' constants (an eye at
// (0, 3, -6), origins within 4.5 of the origin, marches up to 30 from it) are this frame at c = 0, k = 1
struct Frame {
    float c[3] = {0.0f, 0.0f, 0.0f};
    float k = 1.0f;
};
struct Scene {
    const char* name;
    std::vector<Prim> prims;
    float max_dist;
    Frame fr;
};

Prim box(float id, float cx, float cy, float cz, float rx, float ry, float rz) { return Prim{true, {cx, cy, cz}, {rx, ry, rz}, id}; }
Prim sphere(float id, float cx, float cy, float cz, float r) { return Prim{false, {cx, cy, cz}, {r, r, r}, id}; }

// scenes/cornell5.scene
Scene cornell5(float max_dist) {
    return Scene{"cornell5",
                 {box(0, 0, -1.025f, 0, 4, 0.05f, 4), box(1, -3, 1, 0, 0.05f, 3, 4), box(2, 3, 1, 0, 0.05f, 3, 4),
                  sphere(0, 0, 0, 0, 1), box(3, 0, 4, 0, 1.5f, 0.05f, 1.5f)},
                 max_dist};
}
// tests/test_gpu_batch_probes.py overlay_scene: a slab 0.0005 above the floor (near ties over the overlay)
Scene overlay(const char* name, float r) {
    return Scene{name,
                 {box(0, 0, -1.025f, 0, 4, 0.05f, 4), box(1, 0, -1.0245f, 0, r, 0.05f, r), box(2, -3, 1, 0, 0.05f, 3, 4),
                  sphere(3, 0.8f, -0.475f, 0.5f, 0.5f), box(4, -0.8f, -0.475f, 0.5f, 0.5f, 0.5f, 0.5f)},
                 1000.0f};
}
// the large-R case: a sphere of radius 100 as the ground (err()'s R term, eps's extent)
Scene big_sphere() {
    return Scene{"big_sphere",
                 {sphere(0, 0, -101, 0, 100), box(1, -3, 1, 0, 0.05f, 3, 4), sphere(2, 0.5f, -0.5f, 0.25f, 0.5f),
                  box(3, -1, -0.6f, -0.5f, 0.4f, 0.4f, 0.4f), sphere(4, 0, 3, 0, 0.75f)},
                 1000.0f};
}

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    float uni() { return (float)(next() & 0xffffff) * 0x1p-24f; }          // [0, 1)
    float sym() { return 2.0f * uni() - 1.0f; }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

uint32_t bits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}
float dot3(const float* a, const float* b) { return fmaf(a[0], b[0], fmaf(a[1], b[1], a[2] * b[2])); }   // rmr_math.h dot

// rmr_trace.h sd_box / sd_sphere (sqrt_cr is the correctly rounded square root)
float sd(const Prim& q, const float* p) {
    if (q.box) {
        float v[3], o[3];
        for (int k = 0; k < 3; k++) {
            v[k] = fabsf(p[k] - q.c[k]) - q.r[k];
            o[k] = fmaxf(v[k], 0.0f);
        }
        return fminf(fmaxf(v[0], fmaxf(v[1], v[2])), 0.0f) + sqrtf(dot3(o, o));
    }
    const float v[3] = {p[0] - q.c[0], p[1] - q.c[1], p[2] - q.c[2]};
    return sqrtf(dot3(v, v)) - q.r[0];
}
// the trailing step's evaluation: the box form of either primitive through the rule header's two parts
float sd_trail(const Prim& q, const float* p, float& len2) {
    const float h[3] = {q.box ? q.r[0] : 0.0f, q.box ? q.r[1] : 0.0f, q.box ? q.r[2] : 0.0f};
    const float rad = q.box ? 0.0f : q.r[0];
    const float qx = fabsf(p[0] - q.c[0]) - h[0], qy = fabsf(p[1] - q.c[1]) - h[1], qz = fabsf(p[2] - q.c[2]) - h[2];
    len2 = rmr::trail_len2(qx, qy, qz);
    return (rmr::trail_k(qx, qy, qz) + sqrtf(len2)) - rad;
}
// opU fold from (maxDist, -1) in scene order (rmr_trace.h opu)
void fold(const Scene& s, const float* p, float& dx, float& dy) {
    dx = s.max_dist;
    dy = -1.0f;
    for (const Prim& q : s.prims) {
        const float dj = sd(q, p);
        const bool take_id = !(dx < dj), take_d = dx >= dj;
        dy = take_id ? q.id : dy;
        dx = take_d ? dj : dx;
    }
}

// v_sqrt_f32's premise: within 1 ulp of the correctly rounded root for x >= 2^-96, within 2^-47 below
float asqrt(float x, Rng& g) {
    const float r = sqrtf(x);
    if (!(x >= 0x1p-96f)) return x == 0.0f ? 0.0f : fmaxf(r + g.sym() * 0x1p-48f, 0.0f);
    const int k = g.below(3);
    return k == 0 ? r : (k == 1 ? std::nextafterf(r, INFINITY) : std::nextafterf(r, 0.0f));
}
float med3(float a, float b, float c) { return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c)); }

// the generated approximate fold (rmr_jit.cpp: bm_box* over the boxes when there are two or more, am_boxes,
// then the spheres with am_sphere; otherwise am_box / am_sphere in scene order): minimiser w, runner-up s2
void approx_fold(const Scene& s, const float* p, Rng& g, int& w, float& s2) {
    size_t nbox = 0;
    for (const Prim& q : s.prims) nbox += q.box;
    const bool bkey = nbox >= 2;
    float a = 0.0f;
    bool first = true;
    w = -1;
    s2 = INFINITY;
    if (bkey) {
        float k1 = 0.0f, k2 = INFINITY;
        bool bf = true;
        for (size_t j = 0; j < s.prims.size(); j++) {
            const Prim& q = s.prims[j];
            if (!q.box) continue;
            float v[3], o[3];
            for (int k = 0; k < 3; k++) {
                v[k] = fabsf(p[k] - q.c[k]) - q.r[k];
                o[k] = fmaxf(v[k], 0.0f);
            }
            const float key = dot3(o, o) + fminf(fmaxf(v[0], fmaxf(v[1], v[2])), 0.0f);   // bm_key
            if (bf) {
                k1 = key;
                w = (int)j;
                bf = false;
            } else {
                k2 = med3(k1, key, k2);
                if (key < k1) {
                    k1 = key;
                    w = (int)j;
                }
            }
        }
        a = k1 > 0.0f ? asqrt(k1, g) : k1;    // bm_dist
        s2 = k2 > 0.0f ? asqrt(k2, g) : k2;
        first = false;
    }
    for (size_t j = 0; j < s.prims.size(); j++) {
        const Prim& q = s.prims[j];
        if (bkey && q.box) continue;
        float aj;
        if (q.box) {
            float v[3], o[3];
            for (int k = 0; k < 3; k++) {
                v[k] = fabsf(p[k] - q.c[k]) - q.r[k];
                o[k] = fmaxf(v[k], 0.0f);
            }
            aj = fminf(fmaxf(v[0], fmaxf(v[1], v[2])), 0.0f) + asqrt(dot3(o, o), g);
        } else {
            const float v[3] = {p[0] - q.c[0], p[1] - q.c[1], p[2] - q.c[2]};
            aj = asqrt(dot3(v, v), g) - q.r[0];
        }
        if (first) {
            a = aj;
            w = (int)j;
            first = false;
        } else {   // am_take
            s2 = med3(a, aj, s2);
            if (aj < a) {
                a = aj;
                w = (int)j;
            }
        }
    }
}

struct Consts {
    float r2, eps0, am_dmax;
};
Consts scene_consts(const Scene& s) {
    float R = 0.0f, E = 0.0f;   // scene.cpp max_sphere_radius, accel.cpp scene_extent<float>
    for (const Prim& q : s.prims) {
        if (!q.box) R = fmaxf(R, fabsf(q.r[0]));
        const float rr = q.box ? fmaxf(fabsf(q.r[0]), fmaxf(fabsf(q.r[1]), fabsf(q.r[2]))) : fabsf(q.r[0]);
        E = fmaxf(E, fmaxf(fabsf(q.c[0]), fmaxf(fabsf(q.c[1]), fabsf(q.c[2]))) + rr);
    }
    Consts c;
    c.r2 = 2.0f * R;
    c.eps0 = E * 0x1p-17f + 0x1p-60f;
    const double b = (double)s.max_dist - (((double)s.max_dist + (double)c.r2) * 0x1p-20 + 0x1p-39);   // am_direct_bound
    const float f = std::nextafterf((float)b, -INFINITY);
    c.am_dmax = f > 0.0f ? f : -INFINITY;
    return c;
}

struct Tally {
    uint64_t triples = 0, accepted = 0, certified = 0, hits = 0, cert_hits = 0, fails = 0;
};

void point_at(const float* o, const float* d, float t, float* p) {
    for (int k = 0; k < 3; k++) p[k] = fmaf(d[k], t, o[k]);
}

// one trailing attempt from the anchor (t0, anchor bound, w) at parameter t; true when accepted
bool attempt(const Scene& s, const Consts& c, const float* o, const float* d, float anchor, float t0, float t, int w, Tally& T,
             float& F_out) {
    float p[3];
    point_at(o, d, t, p);
    float len2;
    const Prim& q = s.prims[(size_t)w];
    const float F = sd_trail(q, p, len2);
    const rmr::TrailStep r = rmr::trail_rule(anchor, t0, t, rmr::trail_linf(p[0], p[1], p[2]), rmr::trail_finite(p[0], p[1], p[2]),
                                             F, len2, c.eps0, c.am_dmax);
    T.triples++;
    F_out = F;
    if (!r.accept) {
        if (r.cert) {
            T.fails++;
            std::printf("FAIL %s: certified without accepting\n", s.name);
        }
        return false;
    }
    T.accepted++;
    float dx, dy;
    fold(s, p, dx, dy);
    if (bits(sd(q, p)) != bits(F) || bits(dx) != bits(F) || bits(dy) != bits(q.id)) {
        T.fails++;
        if (T.fails < 20)
            std::printf("FAIL %s: accepted w %d at p (%a %a %a) t0 %a t %a: F %a sd %a fold (%a, %a)\n", s.name, w, p[0], p[1], p[2],
                        t0, t, F, sd(q, p), dx, dy);
    }
    const bool hit = F < 0.001f;
    T.hits += hit;
    if (r.cert) {
        T.certified++;
        T.cert_hits += hit;
        for (int e = 0; e < 6; e++) {   // getNormal's probes (rmr_trace.h spread_probes: signed zeros included)
            const float sg = (e & 1) ? -1.0f : 1.0f;
            const int ax = e >> 1;
            const float pr[3] = {p[0] + sg * (ax == 0 ? 0.001f : 0.0f), p[1] + sg * (ax == 1 ? 0.001f : 0.0f),
                                 p[2] + sg * (ax == 2 ? 0.001f : 0.0f)};
            const float fw = sd(q, pr);
            for (size_t j = 0; j < s.prims.size(); j++) {
                if ((int)j == w) continue;
                if (!(sd(s.prims[j], pr) > fw)) {
                    T.fails++;
                    if (T.fails < 20)
                        std::printf("FAIL %s: certified w %d at p (%a %a %a) probe %d: primitive %zu is not farther\n", s.name, w,
                                    p[0], p[1], p[2], e, j);
                }
            }
        }
    }
    return true;
}

void unit(Rng& g, float* d) {
    for (;;) {
        const float v[3] = {g.sym(), g.sym(), g.sym()};
        const float l2 = dot3(v, v);
        if (l2 < 0.01f || l2 > 1.0f) continue;
        const float inv = 1.0f / sqrtf(l2);
        for (int k = 0; k < 3; k++) d[k] = v[k] * inv;
        return;
    }
}

// a ray origin: the scene's box, the eye, or a bounce origin on a primitive (face / edge / corner)
void origin(const Scene& s, Rng& g, float* o, float* d) {
    unit(g, d);
    const int kind = g.below(8);
    if (kind == 0) {
        const float eye[3] = {0.0f, 3.0f, -6.0f};   // an eye above and in front of the scene, looking in
        for (int k = 0; k < 3; k++) o[k] = s.fr.c[k] + s.fr.k * eye[k];
        if (d[2] < 0.0f) d[2] = -d[2];
        return;
    }
    if (kind <= 2) {
        for (int k = 0; k < 3; k++) o[k] = s.fr.c[k] + s.fr.k * (4.5f * g.sym());
        return;
    }
    const Prim& q = s.prims[(size_t)g.below((int)s.prims.size())];
    const float off = g.below(2) ? 0.003f : 0.0f;   // a bounce origin, or exactly on the surface
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (!q.box) {
        unit(g, n);
        for (int k = 0; k < 3; k++) o[k] = fmaf(n[k], q.r[0] + off, q.c[k]);
    } else {
        // each axis: on the -face, on the +face, or inside the extent; at least one axis on a face
        int on[3];
        do {
            for (int k = 0; k < 3; k++) on[k] = g.below(4) == 0 ? (g.below(2) ? 1 : -1) : 0;
        } while (!on[0] && !on[1] && !on[2]);
        for (int k = 0; k < 3; k++) {
            o[k] = on[k] ? q.c[k] + (float)on[k] * (q.r[k] + off) : q.c[k] + q.r[k] * g.sym();
            n[k] = (float)on[k];
        }
    }
    if (dot3(d, n) < 0.0f)
        for (int k = 0; k < 3; k++) d[k] = -d[k];
}

Tally run_scene(const Scene& s, uint64_t want, uint64_t seed) {
    const Consts c = scene_consts(s);
    const float mults[3] = {0.25f, 0.5f, 1.7f};
    Tally T;
    Rng g{seed};
    for (uint64_t ray = 0; T.triples < want && ray < 64 * want; ray++) {
        const float mult = mults[ray % 3];
        float o[3], d[3];
        origin(s, g, o, d);
        float t = 0.0f;
        for (int step = 0; step < 512; step++) {   // march(), rmr_trace.h march_update
            float p0[3];
            point_at(o, d, t, p0);
            if (!rmr::trail_finite(p0[0], p0[1], p0[2]) ||
                rmr::trail_linf(p0[0] - s.fr.c[0], p0[1] - s.fr.c[1], p0[2] - s.fr.c[2]) > s.fr.k * 30.0f)
                break;
            float dx, dy;
            fold(s, p0, dx, dy);
            int w;
            float s2;
            approx_fold(s, p0, g, w, s2);
            const float anchor = rmr::trail_anchor(s2, c.r2, rmr::trail_eps(rmr::trail_linf(p0[0], p0[1], p0[2]), c.eps0));
            if (dx < 0.001f || t >= s.max_dist) break;
            const float tn = fmaf(dx, mult, t);
            // up to kTrailMaxSteps trailing steps after the iteration's own
            float tt = tn;
            for (int k = 0; k < rmr::kTrailMaxSteps; k++) {
                float F;
                if (!attempt(s, c, o, d, anchor, t, tt, w, T, F)) break;
                if (F < 0.001f || tt >= s.max_dist) break;
                tt = fmaf(F, mult, tt);
            }
            // steps of any length ahead of the anchor
            for (int k = 0; k < 2; k++) {
                float F;
                attempt(s, c, o, d, anchor, t, t + g.uni() * 1.5f * fabsf(s2 == s2 && s2 < s.fr.k * 100.0f ? s2 : s.fr.k), w, T, F);
            }
            t = tn;
        }
    }
    return T;
}

// the frame of a scene read from a file: the box of its primitives, without those more than 100 times
// the smallest one (a ground sphere of radius 10^4 says nothing about where the scene's surfaces meet);
// k takes the compiled-in scenes' half-size of 4 to the box's
Frame frame_of(const std::vector<Prim>& prims) {
    auto size = [](const Prim& q) { return fmaxf(fabsf(q.r[0]), q.box ? fmaxf(fabsf(q.r[1]), fabsf(q.r[2])) : 0.0f); };
    float least = INFINITY;
    for (const Prim& q : prims) least = fminf(least, size(q));
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const Prim& q : prims) {
        if (size(q) > 100.0f * least) continue;
        for (int k = 0; k < 3; k++) {
            const float h = fabsf(q.box ? q.r[k] : q.r[0]);
            lo[k] = fminf(lo[k], q.c[k] - h);
            hi[k] = fmaxf(hi[k], q.c[k] + h);
        }
    }
    Frame fr;
    float half = 0.0f;
    for (int k = 0; k < 3; k++) {
        fr.c[k] = 0.5f * (lo[k] + hi[k]);
        half = fmaxf(half, 0.5f * (hi[k] - lo[k]));
    }
    fr.k = half / 4.0f;
    return fr;
}

bool read_scene(const char* path, Scene& s) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) return false;
    bool ok = std::fscanf(f, "%f", &s.max_dist) == 1;
    while (ok) {
        char kind;
        Prim q{};
        const int n = std::fscanf(f, " %c %f %f %f %f %f %f %f", &kind, &q.id, &q.c[0], &q.c[1], &q.c[2], &q.r[0], &q.r[1], &q.r[2]);
        if (n == EOF) break;
        ok = n == 8 && (kind == 'b' || kind == 's') && s.prims.size() < 64;
        q.box = kind == 'b';
        if (ok) s.prims.push_back(q);
    }
    std::fclose(f);
    ok = ok && !s.prims.empty() && s.max_dist > 0.0f;
    if (ok) s.fr = frame_of(s.prims);
    return ok && s.fr.k > 0.0f && std::isfinite(s.fr.k);
}

void report(const Scene& s, const Tally& T) {
    std::printf("%s maxDist %g: triples %llu accepted %llu (%.1f %%) hits %llu certified %llu certified hits %llu\n", s.name,
                (double)s.max_dist, (unsigned long long)T.triples, (unsigned long long)T.accepted,
                100.0 * (double)T.accepted / (double)T.triples, (unsigned long long)T.hits, (unsigned long long)T.certified,
                (unsigned long long)T.cert_hits);
}

int run_file(const char* path) {
    std::string name(path);
    name = name.substr(name.find_last_of('/') + 1);
    name = name.substr(0, name.find('.'));
    Scene s{name.c_str(), {}, 0.0f, Frame{}};
    if (!read_scene(path, s)) {
        std::printf("FAIL %s: not a scene file (max_dist, then `b|s id cx cy cz rx ry rz` per primitive)\n", path);
        return 2;
    }
    const uint64_t want = 200000ull;
    const Tally T = run_scene(s, want, 0x5eed);
    report(s, T);
    uint64_t fails = T.fails;
    if (T.triples < want) {
        fails++;
        std::printf("FAIL %s: fewer than %llu triples\n", s.name, (unsigned long long)want);
    }
    if (fails) {
        std::printf("FAIL %llu violations\n", (unsigned long long)fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && std::strcmp(argv[1], "--scene") == 0) return run_file(argv[2]);
    if (argc != 1) {
        std::printf("usage: trail_rule_test [--scene FILE]\n");
        return 2;
    }
    const Scene scenes[] = {cornell5(1000.0f), cornell5(6.0f), overlay("overlay2", 2.0f), overlay("overlay4", 4.0f), big_sphere()};
    uint64_t fails = 0;
    uint64_t seed = 0x5eed;
    for (const Scene& s : scenes) {
        const Tally T = run_scene(s, 1000000ull, seed++);
        report(s, T);
        fails += T.fails;
        if (T.triples < 1000000ull) {
            fails++;
            std::printf("FAIL %s: fewer than 10^6 triples\n", s.name);
        }
        if (std::strcmp(s.name, "cornell5") == 0 && (T.accepted == 0 || T.cert_hits == 0)) {
            fails++;
            std::printf("FAIL %s: the rule never accepted (or never certified a hit): the check is vacuous\n", s.name);
        }
    }
    if (fails) {
        std::printf("FAIL %llu violations\n", (unsigned long long)fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
