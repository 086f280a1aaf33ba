// rmr_slot_rule.h — the bookkeeping of the lane-slot park step's overflow deposit (rmr_trace.h
// RMR_SLOT_OVERFLOW, trace_main), as arithmetic on the wave's 64-bit lane masks. The kernel and the
// host program csrc/slot_rule_test.cpp compile this one statement.
//
// After the own-slot parks of a park step, a lane that still holds a continuing hit in registers has an
// event in its own slot (a candidate). The slots that are empty then are the targets. The k-th candidate
// in lane order deposits its event into the k-th target in lane order, for k < n = min(candidates,
// targets): the candidate goes idle, the target slot holds an event. Candidates beyond n keep waiting
// in registers. A deposit never touches a slot that holds an event or a ready ray.
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define RMR_SLOT_HD __host__ __device__ inline
#else
#define RMR_SLOT_HD inline
#endif

namespace rmr {

RMR_SLOT_HD int slot_popc(uint64_t m) { return __builtin_popcountll(m); }
// lanes of m below `lane`: the lane's rank among m's lanes (the kernel: v_mbcnt of the ballot)
RMR_SLOT_HD int slot_rank(uint64_t m, int lane) { return slot_popc(m & ((1ull << lane) - 1ull)); }
// deposits of a step: every candidate finds a target, or every target a candidate
RMR_SLOT_HD int slot_deposits(uint64_t cand, uint64_t empty) {
    const int nc = slot_popc(cand), ne = slot_popc(empty);
    return nc < ne ? nc : ne;
}
// a lane of `mask` with this rank takes part in a step of n deposits (candidates give, targets take)
RMR_SLOT_HD bool slot_in_step(bool in_mask, int rank, int n) { return in_mask && rank < n; }

// the first n lanes of m
RMR_SLOT_HD uint64_t slot_first(uint64_t m, int n) {
    uint64_t r = 0;
    for (; n > 0 && m; n--) {
        const uint64_t low = m & (0ull - m);
        r |= low;
        m ^= low;
    }
    return r;
}
// the lane of m with rank k (k < popc(m))
RMR_SLOT_HD int slot_nth(uint64_t m, int k) {
    for (; k > 0; k--) m &= m - 1ull;
    return __builtin_ctzll(m);
}

// One overflow step on the masks: candidates, empty slots, event slots, ready-ray slots (the three slot
// masks partition the wave; `cand` lies within `events`).
struct SlotStep {
    int n;             // deposits
    uint64_t give;     // candidates that deposit and go idle
    uint64_t take;     // slots that receive an event
    uint64_t events;   // event slots afterwards (nev = their count)
    uint64_t empty;    // empty slots afterwards
    uint64_t waiting;  // candidates left in registers (none while a slot is empty)
};
RMR_SLOT_HD SlotStep slot_overflow_step(uint64_t cand, uint64_t empty, uint64_t events) {
    SlotStep s;
    s.n = slot_deposits(cand, empty);
    s.give = slot_first(cand, s.n);
    s.take = slot_first(empty, s.n);
    s.events = events | s.take;
    s.empty = empty & ~s.take;
    s.waiting = cand & ~s.give;
    return s;
}
// the slot a depositing candidate writes: the target with the candidate's rank
RMR_SLOT_HD int slot_target(uint64_t cand, uint64_t empty, int lane) { return slot_nth(empty, slot_rank(cand, lane)); }

}  // namespace rmr
