// trail_word_test.cpp — the trailing passes' launch word (rmr_trail_rule.h trail_word) on the CPU: packing and
// unpacking round-trip over the whole range, the word stays clear of the park and batch thresholds below it in
// KParams::shade_threshold, a fixed schedule's word is its pass count, and the range check refuses everything
// outside the range. Prints "ok" last; any line with FAIL fails tests/test_trail_adaptive_cpu.py.
#include <cstdio>

#include "rmr_trail_rule.h"

int main() {
    int bad = 0, n = 0;
    for (int k = 0; k <= rmr::kTrailMaxSteps; k++)
        for (int r = 0; r <= rmr::kTrailMaxRatio; r++)
            for (int x = 0; x <= 1; x++) {
                const int w = rmr::trail_word(k, r, x != 0);
                n++;
                if (!rmr::trail_word_valid(k, r, x)) bad++, printf("FAIL valid(%d, %d, %d)\n", k, r, x);
                if (rmr::trail_word_k(w) != k || rmr::trail_word_ratio(w) != r || rmr::trail_word_park_exit(w) != (x != 0))
                    bad++, printf("FAIL round trip (%d, %d, %d) -> %#x -> (%d, %d, %d)\n", k, r, x, w, rmr::trail_word_k(w),
                                  rmr::trail_word_ratio(w), (int)rmr::trail_word_park_exit(w));
                if (w < 0 || w >= (1 << 9)) bad++, printf("FAIL word %#x of (%d, %d, %d) outside nine bits\n", w, k, r, x);
                // in the launch word: above the two thresholds' bytes, below the sign bit, and read back whatever they hold
                const int t = 0xffff | (w << rmr::kTrailWordShift);
                if (t < 0 || (t & 0xffff) != 0xffff || (t >> rmr::kTrailWordShift) != w)
                    bad++, printf("FAIL launch word %#x of (%d, %d, %d)\n", t, k, r, x);
                if (r == 0 && x == 0 && w != k) bad++, printf("FAIL fixed schedule %d has word %#x\n", k, w);
            }
    // distinct tunings have distinct words
    for (int a = 0; a < (1 << 9); a++) {
        int hits = 0;
        for (int k = 0; k <= rmr::kTrailMaxSteps; k++)
            for (int r = 0; r <= rmr::kTrailMaxRatio; r++)
                for (int x = 0; x <= 1; x++) hits += rmr::trail_word(k, r, x != 0) == a;
        if (hits > 1) bad++, printf("FAIL word %#x has %d tunings\n", a, hits);
    }
    const int outside[][3] = {{-1, 0, 0}, {rmr::kTrailMaxSteps + 1, 0, 0}, {0, -1, 0}, {0, rmr::kTrailMaxRatio + 1, 0},
                              {0, 0, -1}, {0, 0, 2}, {1 << 20, 3, 1}, {3, 1 << 20, 1}};
    for (const auto& o : outside)
        if (rmr::trail_word_valid(o[0], o[1], o[2])) bad++, printf("FAIL valid(%d, %d, %d)\n", o[0], o[1], o[2]);
    printf("tunings %d k_max 0..%d ratio 0..%d\n", n, rmr::kTrailMaxSteps, rmr::kTrailMaxRatio);
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
