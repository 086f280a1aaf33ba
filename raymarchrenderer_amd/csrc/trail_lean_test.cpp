// trail_lean_test.cpp — host check of the statements the trailing steps run (rmr_trail_rule.h trail_row,
// trail_anchor_hi, trail_rule_hi with the launch-constant eps of accel.cpp trail_eps_bound). Build: make
// trail_lean_test / trail_lean_test_san (-ffp-contract=off, as the kernels).
//
// The scenes, the origins, the approximate fold and the marches are trail_rule_test.cpp's, compiled into this
// program as they stand. What differs is what the kernel does differently: every ray has its escape bound
// (each primitive's box inflated by accel.cpp escape_inflation, the slab test of rmr_trace.h ray_exit in
// double, widened as there), a march ends where its t passes the bound, and no point past it is evaluated.
//
// Checked at every evaluated point: eps(p) of the first rule (|p|_inf + 0.002) is at most the launch's
// eps_hi, and the table row's box form has sd_box's / sd_sphere's bits. Wherever the rule accepts: the whole
// float opU fold at that point is (F_w, id_w) bit for bit. Wherever it certifies: at each of getNormal's six
// probes every other primitive is strictly farther than w. Rays and parameters that are not finite (a NaN or
// infinite coordinate of the origin or the direction, a t that overflows the point, an infinite or NaN t)
// follow per scene: the rule, which has no finiteness test of its own, must refuse every point with a
// coordinate that is not finite.
// Per scene one line with the counts, the share of the first rule's accepts that this rule refuses among
// them (recorded, not gated). Last line "ok"; a line "FAIL ..." per violation otherwise.
//
// trail_lean_test --scene FILE: the same on one scene file (trail_rule_test.cpp's format), 200,000 triples.
#define main trail_rule_test_main
#include "trail_rule_test.cpp"
#undef main

#include "accel.hpp"

namespace {

struct Lean {
    Consts c;
    float eps_hi, ak, ck;
    std::vector<double> boxes;   // inflated escape boxes: lo.xyz, hi.xyz per primitive
};

Lean lean_consts(const Scene& s) {
    Lean L;
    L.c = scene_consts(s);
    float E = 0.0f;   // accel.cpp scene_extent<float>
    double esc_extent = 0.0;
    for (const Prim& q : s.prims) {
        const float rr = q.box ? fmaxf(fabsf(q.r[0]), fmaxf(fabsf(q.r[1]), fabsf(q.r[2]))) : fabsf(q.r[0]);
        E = fmaxf(E, fmaxf(fabsf(q.c[0]), fmaxf(fabsf(q.c[1]), fabsf(q.c[2]))) + rr);
        for (int k = 0; k < 3; k++)
            esc_extent = std::fmax(esc_extent, std::fabs((double)q.c[k]) + std::fabs((double)(q.box ? q.r[k] : q.r[0])));
    }
    // the origins' extent in the eye's place: the frame's eye and its box of random origins (origin())
    float org[3] = {0.0f, 0.0f, 0.0f};
    org[0] = fmaxf(fabsf(s.fr.c[0]), fmaxf(fabsf(s.fr.c[1]), fabsf(s.fr.c[2]))) + 6.0f * s.fr.k;
    const double infl = rmr::escape_inflation(org, esc_extent, s.max_dist);
    L.eps_hi = rmr::trail_eps_bound(org, esc_extent, infl, E);
    L.ak = rmr::trail_anchor_const(L.eps_hi);
    L.ck = rmr::trail_cert_const(L.eps_hi);
    for (const Prim& q : s.prims) {
        for (int k = 0; k < 3; k++) L.boxes.push_back((double)q.c[k] - std::fabs((double)(q.box ? q.r[k] : q.r[0])) - infl);
        for (int k = 0; k < 3; k++) L.boxes.push_back((double)q.c[k] + std::fabs((double)(q.box ? q.r[k] : q.r[0])) + infl);
    }
    return L;
}

// rmr_trace.h ray_exit: the last parameter at which the ray is inside a box, widened; -inf when it meets none
double ray_exit(const Lean& L, const float* o, const float* d) {
    double last = -INFINITY;
    for (size_t b = 0; b + 6 <= L.boxes.size(); b += 6) {
        double tn = -INFINITY, tf = INFINITY;
        bool out = false;
        for (int k = 0; k < 3; k++) {
            const double lo = L.boxes[b + (size_t)k], hi = L.boxes[b + 3 + (size_t)k];
            if (d[k] == 0.0f) {
                out = out || (double)o[k] < lo || (double)o[k] > hi;
                continue;
            }
            const double a = (lo - (double)o[k]) / (double)d[k], c = (hi - (double)o[k]) / (double)d[k];
            tn = std::fmax(tn, std::fmin(a, c));
            tf = std::fmin(tf, std::fmax(a, c));
        }
        if (!out && !(tn > tf)) last = std::fmax(last, tf);
    }
    return last > 0.0 ? last * (1.0 + 0x1p-19) + 0x1p-60 : last;
}

struct LeanTally {
    Tally T;
    uint64_t old_accepts = 0, old_refused = 0;   // the first rule's accepts; those among them this rule refuses
    uint64_t nonfinite = 0;                      // points with a coordinate that is not finite, all refused
};

bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// one trailing attempt from the anchor (t0, both rules' anchors, w) at parameter t; true when accepted
bool attempt_lean(const Scene& s, const Lean& L, const float* o, const float* d, float anchor, float anchor_old, float t0, float t,
                  int w, LeanTally& LT, float& F_out) {
    Tally& T = LT.T;
    float p[3];
    point_at(o, d, t, p);
    const Prim& q = s.prims[(size_t)w];
    float row[8];
    rmr::trail_row(q.box, q.c[0], q.c[1], q.c[2], q.r[0], q.r[1], q.r[2], q.id, row);
    const float len2 = rmr::trail_len2(fabsf(p[0] - row[0]) - row[3], fabsf(p[1] - row[1]) - row[4], fabsf(p[2] - row[2]) - row[5]);
    const float F = rmr::trail_row_dist(row, p[0], p[1], p[2], sqrtf(len2));
    const rmr::TrailStep r = rmr::trail_rule_hi(anchor, t0, t, F, len2, L.ck, L.c.am_dmax);
    T.triples++;
    F_out = F;
    if (!finite3(p)) {
        LT.nonfinite++;
        if (r.accept || r.cert) {
            T.fails++;
            if (T.fails < 20)
                std::printf("FAIL %s: accepted at a point that is not finite: p (%a %a %a) t0 %a t %a anchor %a F %a\n", s.name, p[0],
                            p[1], p[2], t0, t, anchor, F);
        }
        return false;
    }
    // the launch's eps bounds the first rule's eps at the point (and at its probes: the 0.002)
    const float linf = rmr::trail_linf(p[0], p[1], p[2]);
    if (!(rmr::trail_eps(linf + 0.002f, L.c.eps0) <= L.eps_hi)) {
        T.fails++;
        if (T.fails < 20) std::printf("FAIL %s: eps at p (%a %a %a) exceeds eps_hi %a\n", s.name, p[0], p[1], p[2], L.eps_hi);
    }
    // the row's box form is the primitive's own distance, bit for bit
    float len2_old;
    if (bits(sd(q, p)) != bits(F) || bits(sd_trail(q, p, len2_old)) != bits(F) || bits(row[7]) != bits(q.id)) {
        T.fails++;
        if (T.fails < 20) std::printf("FAIL %s: row of w %d at p (%a %a %a): F %a sd %a\n", s.name, w, p[0], p[1], p[2], F, sd(q, p));
    }
    const rmr::TrailStep ro = rmr::trail_rule(anchor_old, t0, t, linf, rmr::trail_finite(p[0], p[1], p[2]), F, len2, L.c.eps0, L.c.am_dmax);
    LT.old_accepts += ro.accept;
    LT.old_refused += ro.accept && !r.accept;
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
    if (bits(dx) != bits(F) || bits(dy) != bits(q.id)) {
        T.fails++;
        if (T.fails < 20)
            std::printf("FAIL %s: accepted w %d at p (%a %a %a) t0 %a t %a: F %a fold (%a, %a)\n", s.name, w, p[0], p[1], p[2], t0, t, F,
                        dx, dy);
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
                        std::printf("FAIL %s: certified w %d at p (%a %a %a) probe %d: primitive %zu is not farther\n", s.name, w, p[0],
                                    p[1], p[2], e, j);
                }
            }
        }
    }
    return true;
}

// both rules' anchors at p0 = fma(d, t0, o), and the map's minimiser
void anchors(const Scene& s, const Lean& L, Rng& g, const float* p0, float& anchor, float& anchor_old, int& w, float& s2) {
    approx_fold(s, p0, g, w, s2);
    anchor = rmr::trail_anchor_hi(s2, L.c.r2, L.ak, p0[0], p0[1], p0[2]);
    anchor_old = rmr::trail_anchor(s2, L.c.r2, rmr::trail_eps(rmr::trail_linf(p0[0], p0[1], p0[2]), L.c.eps0));
}

void run_marches(const Scene& s, const Lean& L, uint64_t want, uint64_t seed, LeanTally& LT) {
    const float mults[3] = {0.25f, 0.5f, 1.7f};
    Tally& T = LT.T;
    Rng g{seed};
    for (uint64_t ray = 0; T.triples < want && ray < 64 * want; ray++) {
        const float mult = mults[ray % 3];
        float o[3], d[3];
        origin(s, g, o, d);
        const double texit = ray_exit(L, o, d);
        if (!(texit >= 0.0)) continue;   // start_march: the march ends as its miss at once
        float t = 0.0f;
        for (int step = 0; step < 512; step++) {   // march(), rmr_trace.h march_update
            float p0[3];
            point_at(o, d, t, p0);
            if (!finite3(p0)) break;
            float dx, dy;
            fold(s, p0, dx, dy);
            int w;
            float s2, anchor, anchor_old;
            anchors(s, L, g, p0, anchor, anchor_old, w, s2);
            if (!(rmr::trail_eps(rmr::trail_linf(p0[0], p0[1], p0[2]) + 0.002f, L.c.eps0) <= L.eps_hi)) {
                T.fails++;
                if (T.fails < 20) std::printf("FAIL %s: eps at the anchor (%a %a %a) exceeds eps_hi %a\n", s.name, p0[0], p0[1], p0[2], L.eps_hi);
            }
            if (dx < 0.001f || t >= s.max_dist) break;
            const float tn = fmaf(dx, mult, t);
            if ((double)tn > texit) break;   // escaped
            // up to kTrailMaxSteps trailing steps after the iteration's own
            float tt = tn;
            for (int k = 0; k < rmr::kTrailMaxSteps; k++) {
                float F;
                if (!attempt_lean(s, L, o, d, anchor, anchor_old, t, tt, w, LT, F)) break;
                if (F < 0.001f || tt >= s.max_dist) break;
                const float t2 = fmaf(F, mult, tt);
                if ((double)t2 > texit) break;
                tt = t2;
            }
            // steps of any length ahead of the anchor, within the escape bound
            for (int k = 0; k < 2; k++) {
                float F;
                const float ta = t + g.uni() * 1.5f * fabsf(s2 == s2 && s2 < s.fr.k * 100.0f ? s2 : s.fr.k);
                if ((double)ta <= texit) attempt_lean(s, L, o, d, anchor, anchor_old, t, ta, w, LT, F);
            }
            t = tn;
        }
    }
}

// rays and parameters that are not finite: whatever the anchor's map gives there, no such point is accepted
void run_nonfinite(const Scene& s, const Lean& L, uint64_t seed, LeanTally& LT) {
    Rng g{seed ^ 0x9e3779b97f4a7c15ull};
    const float bad[3] = {NAN, INFINITY, -INFINITY};
    for (int n = 0; n < 60000; n++) {
        float o[3], d[3];
        origin(s, g, o, d);
        float t0 = g.uni() * 4.0f * s.fr.k, t = t0 + g.uni() * 2.0f * s.fr.k;
        const int kind = n % 6, k = g.below(3);
        if (kind == 0) o[k] = bad[g.below(3)];
        else if (kind == 1) d[k] = bad[g.below(3)];
        else if (kind == 2) {   // a finite ray whose point overflows (a unit direction needs a huge origin for that)
            for (int j = 0; j < 3; j++) d[j] = j == k ? 1.0f : 0.0f;
            o[k] = t = 0x1.8p127f;
        }
        else if (kind == 3) t = g.below(2) ? INFINITY : NAN;
        else if (kind == 4) t0 = 0.0f, d[k] = bad[1 + g.below(2)];   // 0 x inf at the anchor
        else o[k] = bad[g.below(3)], d[(k + 1) % 3] = bad[g.below(3)];
        float p0[3];
        point_at(o, d, t0, p0);
        int w;
        float s2, anchor, anchor_old;
        anchors(s, L, g, p0, anchor, anchor_old, w, s2);
        const uint64_t before = LT.nonfinite;
        float F;
        attempt_lean(s, L, o, d, anchor, anchor_old, t0, t, w, LT, F);
        if (LT.nonfinite == before) {
            LT.T.fails++;
            if (LT.T.fails < 20) std::printf("FAIL %s: case %d of the points that are not finite gave a finite point\n", s.name, kind);
        }
    }
}

LeanTally run_lean(const Scene& s, uint64_t want, uint64_t seed) {
    const Lean L = lean_consts(s);
    LeanTally LT;
    if (!std::isfinite(L.eps_hi)) {
        LT.T.fails++;
        std::printf("FAIL %s: eps_hi is not finite\n", s.name);
        return LT;
    }
    run_marches(s, L, want, seed, LT);
    run_nonfinite(s, L, seed, LT);
    return LT;
}

void report_lean(const Scene& s, const LeanTally& LT) {
    const Tally& T = LT.T;
    std::printf("%s maxDist %g: triples %llu accepted %llu (%.1f %%) hits %llu certified %llu certified hits %llu "
                "first-rule accepts %llu refused of them %llu (%.3f %%) nonfinite %llu\n",
                s.name, (double)s.max_dist, (unsigned long long)T.triples, (unsigned long long)T.accepted,
                100.0 * (double)T.accepted / (double)(T.triples ? T.triples : 1), (unsigned long long)T.hits,
                (unsigned long long)T.certified, (unsigned long long)T.cert_hits, (unsigned long long)LT.old_accepts,
                (unsigned long long)LT.old_refused, 100.0 * (double)LT.old_refused / (double)(LT.old_accepts ? LT.old_accepts : 1),
                (unsigned long long)LT.nonfinite);
}

int finish(uint64_t fails) {
    if (fails) {
        std::printf("FAIL %llu violations\n", (unsigned long long)fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

int run_lean_file(const char* path) {
    std::string name(path);
    name = name.substr(name.find_last_of('/') + 1);
    name = name.substr(0, name.find('.'));
    Scene s{name.c_str(), {}, 0.0f, Frame{}};
    if (!read_scene(path, s)) {
        std::printf("FAIL %s: not a scene file (max_dist, then `b|s id cx cy cz rx ry rz` per primitive)\n", path);
        return 2;
    }
    const uint64_t want = 200000ull;
    const LeanTally LT = run_lean(s, want, 0x5eed);
    report_lean(s, LT);
    uint64_t fails = LT.T.fails;
    if (LT.T.triples < want) {
        fails++;
        std::printf("FAIL %s: fewer than %llu triples\n", s.name, (unsigned long long)want);
    }
    return finish(fails);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && std::strcmp(argv[1], "--scene") == 0) return run_lean_file(argv[2]);
    if (argc != 1) {
        std::printf("usage: trail_lean_test [--scene FILE]\n");
        return 2;
    }
    const Scene scenes[] = {cornell5(1000.0f), cornell5(6.0f), overlay("overlay2", 2.0f), overlay("overlay4", 4.0f), big_sphere()};
    uint64_t fails = 0;
    uint64_t seed = 0x5eed;
    for (const Scene& s : scenes) {
        const LeanTally LT = run_lean(s, 1000000ull, seed++);
        report_lean(s, LT);
        fails += LT.T.fails;
        if (LT.T.triples < 1000000ull) {
            fails++;
            std::printf("FAIL %s: fewer than 10^6 triples\n", s.name);
        }
        if (std::strcmp(s.name, "cornell5") == 0 && (LT.T.accepted == 0 || LT.T.cert_hits == 0)) {
            fails++;
            std::printf("FAIL %s: the rule never accepted (or never certified a hit): the check is vacuous\n", s.name);
        }
    }
    return finish(fails);
}
