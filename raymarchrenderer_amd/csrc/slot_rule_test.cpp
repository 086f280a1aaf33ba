// slot_rule_test.cpp — host checks of the lane-slot park step's overflow rule (rmr_slot_rule.h, the header
// trace_main compiles) and of the wave schedule around it (tests/test_slot_rule_cpu.py builds and runs this
// program, plain and under the address and undefined-behaviour sanitizers).
//
// 1. The rule on masks: every partition of a 6-lane wave's slots into empty / event / ready with every
//    candidate set, and random 64-lane masks. The assignment is injective and uses only empty slots, the
//    event count afterwards is the number of event slots, no candidate is left while a slot is empty.
// 2. A whole wave of trace_main's lane-slot schedule, with random march lengths and event kinds, through
//    the exhaustion of the work queue, with the overflow deposit on and off: the loop ends, every unit's
//    sample is stored exactly once, and no pass of the outer loop runs with neither an active lane nor
//    progress.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rmr_slot_rule.h"

using namespace rmr;

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
    double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

// the rule's properties for one state; returns the step
static SlotStep check_step(uint64_t cand, uint64_t empty, uint64_t events, uint64_t ready, uint64_t all) {
    const SlotStep s = slot_overflow_step(cand, empty, events);
    const int nc = slot_popc(cand), ne = slot_popc(empty);
    CHECK(s.n == (nc < ne ? nc : ne), "n %d", s.n);
    CHECK(slot_popc(s.give) == s.n && slot_popc(s.take) == s.n, "counts");
    CHECK((s.give & ~cand) == 0 && (s.take & ~empty) == 0, "give within candidates, take within empty slots");
    CHECK((s.take & (events | ready)) == 0, "a deposit touches no event or ready slot");
    CHECK(s.events == (events | s.take) && slot_popc(s.events) == slot_popc(events) + s.n, "nev is the number of event slots");
    CHECK((s.events | s.empty | ready) == all && (s.events & s.empty) == 0 && (s.empty & ready) == 0, "the slots stay partitioned");
    CHECK(s.waiting == (cand & ~s.give) && (s.waiting == 0 || s.empty == 0), "no candidate left while a slot is empty");
    // the lanes' own view (the kernel: rank by mbcnt, slot_in_step, the target through the rank table)
    uint64_t used = 0;
    int tab[64];
    for (int l = 0; l < 64; l++)
        if (slot_in_step((empty >> l) & 1, slot_rank(empty, l), s.n)) tab[slot_rank(empty, l)] = l;
    for (int l = 0; l < 64; l++) {
        const bool give = slot_in_step((cand >> l) & 1, slot_rank(cand, l), s.n);
        CHECK(give == (bool)((s.give >> l) & 1), "lane %d give", l);
        CHECK(slot_in_step((empty >> l) & 1, slot_rank(empty, l), s.n) == (bool)((s.take >> l) & 1), "lane %d take", l);
        if (!give) continue;
        const int t = tab[slot_rank(cand, l)];
        CHECK(t == slot_target(cand, empty, l), "lane %d target", l);
        CHECK((empty >> t) & 1, "lane %d deposits into a slot that is not empty", l);
        CHECK(!((used >> t) & 1), "slot %d used twice", t);
        used |= 1ull << t;
    }
    CHECK(used == s.take, "the targets are the taken slots");
    return s;
}

static void rule_cases() {
    // exhaustive: 6 lanes, each slot empty / event / ready, every candidate set within the event slots
    const int W = 6;
    int pw = 1;
    for (int i = 0; i < W; i++) pw *= 3;
    long cases = 0;
    for (int code = 0; code < pw; code++) {
        uint64_t m[3] = {0, 0, 0};
        for (int i = 0, c = code; i < W; i++, c /= 3) m[c % 3] |= 1ull << i;
        for (uint64_t cand = m[1];; cand = (cand - 1) & m[1]) {   // every subset of the event slots
            check_step(cand, m[0], m[1], m[2], (1ull << W) - 1);
            cases++;
            if (!cand) break;
        }
    }
    // the same wave placed at the top of 64 lanes (bit 63, shifts by 63)
    for (int code = 0; code < pw; code++) {
        uint64_t m[3] = {0, 0, 0};
        for (int i = 0, c = code; i < W; i++, c /= 3) m[c % 3] |= 1ull << (58 + i);
        check_step(m[1], m[0], m[1], m[2], ((1ull << W) - 1) << 58);
        cases++;
    }
    Rng g{0x9e3779b97f4a7c15ull};
    for (int k = 0; k < 200000; k++) {
        // slot states of varied density, candidates a random part of the event slots
        const uint64_t a = g.next(), b = g.next(), d0 = (k & 1) ? g.next() : ~0ull, d1 = (k & 2) ? g.next() : ~0ull;
        const uint64_t events = a & d0, ready = ~events & b & d1, empty = ~(events | ready);
        uint64_t cand = events & g.next();
        if ((k & 12) == 0) cand = events;
        check_step(cand, empty, events, ready, ~0ull);
        cases++;
    }
    check_step(~0ull, 0, ~0ull, 0, ~0ull);
    check_step(0, ~0ull, 0, 0, ~0ull);
    std::printf("rule: %ld cases\n", cases + 2);
}

// ---- the wave's schedule (trace_main, lane slots) ----
enum { IDLE = 0, MARCH = 1, HIT = 2 };   // HIT: the march ended (is_shade)
struct Path {
    int unit = -1, bounces = 0;
};
struct SimStats {
    long passes = 0, iters = 0, batches = 0, events = 0, deposits = 0, lost_wait = 0, lost_fin = 0, lane_iters = 0;
};

static bool simulate(int PK, int T2, int TR, int n_units, bool overflow, uint64_t seed, double mean, int max_bounces, SimStats& st) {
    Rng g{seed * 0x2545f4914f6cdd1dull + 1};
    int phase[64], steps[64], sst[64];
    bool cheap[64];
    Path reg[64], slot[64];
    for (int l = 0; l < 64; l++) phase[l] = IDLE, steps[l] = 0, sst[l] = 0, cheap[l] = false;
    std::vector<int> stored((size_t)n_units, 0);
    int next_unit = 0, nev = 0;
    bool exhausted = false;
    auto march_len = [&]() { int n = 1; while (g.unit() > 1.0 / mean && n < 400) n++; return n; };
    auto start = [&](int l, Path p) { reg[l] = p; phase[l] = MARCH; steps[l] = march_len(); };
    auto mask = [&](auto f) { uint64_t m = 0; for (int l = 0; l < 64; l++) if (f(l)) m |= 1ull << l; return m; };
    // (every pass with an active lane advances a march of at most 400 steps; a unit has at most
    // max_bounces + 1 marches; the passes without an active lane make progress, checked below)
    const long pass_limit = 4L * 400 * n_units * (max_bounces + 1) + 1000;
    for (;;) {
        if (++st.passes > pass_limit) { std::printf("FAIL: the loop does not end\n"); return false; }
        bool progress = false;
        for (int l = 0; l < 64; l++)   // an idle lane marches its slot's ready ray before any fresh unit
            if (phase[l] == IDLE && sst[l] == 2) { start(l, slot[l]); sst[l] = 0; progress = true; }
        if (!exhausted) {
            const uint64_t idle = mask([&](int l) { return phase[l] == IDLE; }), act0 = mask([&](int l) { return phase[l] == MARCH; });
            if (idle && (slot_popc(idle) >= TR || act0 == 0)) {
                if (next_unit >= n_units) {
                    exhausted = true;
                    progress = true;   // (the claim that finds the queue used up happens once)
                }
                for (int l = 0; l < 64 && next_unit < n_units; l++)
                    if (phase[l] == IDLE) { start(l, Path{next_unit++, 0}); progress = true; }
            }
        }
        const bool had_active = mask([&](int l) { return phase[l] == MARCH; }) != 0;
        if (had_active) {
            const uint64_t wait0 = mask([&](int l) { return phase[l] == HIT; });
            const int TL = slot_popc(wait0) + PK;
            for (;;) {
                const uint64_t sm0 = mask([&](int l) { return phase[l] == HIT; });
                st.lost_wait += slot_popc(wait0);
                st.lost_fin += slot_popc(sm0 & ~wait0);
                for (int l = 0; l < 64; l++)
                    if (phase[l] == MARCH) {
                        st.lane_iters++;
                        if (--steps[l] == 0) {
                            phase[l] = HIT;
                            // a miss, an emitter, the last bounce: the event ends its path
                            cheap[l] = g.unit() < 0.42 || reg[l].bounces >= max_bounces;
                        }
                    }
                st.iters++;
                const uint64_t sm = mask([&](int l) { return phase[l] == HIT; }), am = mask([&](int l) { return phase[l] == MARCH; });
                if (!am || slot_popc(sm) >= TL) break;
            }
        }
        for (;;) {
            // park step
            for (int l = 0; l < 64; l++) {
                if (phase[l] != HIT) continue;
                if (cheap[l]) {
                    stored[(size_t)reg[l].unit]++;
                    phase[l] = IDLE;
                    progress = true;
                } else if (sst[l] != 1) {
                    const bool swap = sst[l] == 2;
                    const Path ray = slot[l];
                    slot[l] = reg[l];
                    phase[l] = IDLE;
                    if (swap) start(l, ray);
                    sst[l] = 1;
                    nev++;
                    progress = true;
                }
            }
            if (overflow) {
                const uint64_t cand = mask([&](int l) { return phase[l] == HIT; });
                const uint64_t empty = mask([&](int l) { return sst[l] == 0; }), events = mask([&](int l) { return sst[l] == 1; });
                const uint64_t ready = mask([&](int l) { return sst[l] == 2; });
                if (cand && empty) {
                    const SlotStep s = check_step(cand, empty, events, ready, ~0ull);
                    for (int l = 0; l < 64; l++)
                        if ((s.give >> l) & 1) {
                            const int t = slot_target(cand, empty, l);
                            slot[t] = reg[l];
                            sst[t] = 1;
                            phase[l] = IDLE;
                        }
                    nev += s.n;
                    st.deposits += s.n;
                    progress = true;
                }
            }
            CHECK(nev == slot_popc(mask([&](int l) { return sst[l] == 1; })), "nev %d", nev);
            const bool active = mask([&](int l) { return phase[l] == MARCH; }) != 0;
            if (!(nev && (nev >= T2 || !active))) break;
            st.batches++;
            st.events += nev;
            nev = 0;
            progress = true;
            for (int l = 0; l < 64; l++) {
                if (sst[l] != 1) continue;
                sst[l] = 0;
                if (g.unit() < 0.8) {   // the next ray marches; else it met no escape box: shaded as its miss
                    slot[l].bounces++;
                    sst[l] = 2;
                } else {
                    stored[(size_t)slot[l].unit]++;
                }
            }
            if (mask([&](int l) { return phase[l] == HIT; }) == 0) break;
        }
        CHECK(had_active || progress, "a pass with neither an active lane nor progress (pass %ld)", st.passes);
        if (!had_active && !progress) return false;
        const bool live = mask([&](int l) { return phase[l] != IDLE; }) != 0, used = mask([&](int l) { return sst[l] != 0; }) != 0;
        if (!live && exhausted && !used) break;
    }
    for (int u = 0; u < n_units; u++)
        if (stored[(size_t)u] != 1) {
            std::printf("FAIL: unit %d stored %d times\n", u, stored[(size_t)u]);
            return false;
        }
    return true;
}

int main(int argc, char** argv) {
    rule_cases();
    const int Ps[] = {1, 8, 20, 255}, T2s[] = {1, 24, 32, 48, 56, 64, 255}, TRs[] = {1, 4, 32};
    const int units[] = {1, 40, 64, 700, 3000};
    int runs = 0;
    for (int P : Ps)
        for (int T2 : T2s)
            for (int TR : TRs)
                for (int n : units)
                    for (int ov = 0; ov < 2; ov++)
                        for (uint64_t seed = 1; seed <= 2; seed++) {
                            SimStats st;
                            const double mean = seed == 1 ? 38.0 : 3.0;
                            if (!simulate(P, T2, TR, n, ov != 0, seed + 7 * (uint64_t)runs, mean, 4, st)) {
                                std::printf("FAIL: P %d T2 %d TR %d units %d overflow %d seed %d\n", P, T2, TR, n, ov, (int)seed);
                                g_fail++;
                            }
                            if (!ov) CHECK(st.deposits == 0, "deposits without the switch");
                            runs++;
                        }
    std::printf("wave: %d runs\n", runs);
    // the schedule's figures for one setting (argv: P T2 TR overflow), for a look by hand
    if (argc >= 5) {
        SimStats st;
        simulate(std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), 20000, std::atoi(argv[4]) != 0, 5, 38.0, 4, st);
        std::printf("iters %ld lanes/iter %.2f waiting/iter %.2f finished/iter %.2f batches %ld events/batch %.2f deposits %ld\n", st.iters,
                    (double)st.lane_iters / (double)st.iters, (double)st.lost_wait / (double)st.iters,
                    (double)st.lost_fin / (double)st.iters, st.batches, (double)st.events / (double)(st.batches ? st.batches : 1),
                    st.deposits);
    }
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
