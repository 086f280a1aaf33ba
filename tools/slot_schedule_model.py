"""Monte Carlo cost model of one wave under trace_main's lane-slot schedule (no GPU): what a change to the
park step or the thresholds does to the wave's issue slots, before it is built.

    python tools/slot_schedule_model.py [--units N] [--seed S] [--map-cost C] [--pass-cost C] [--batch-cost C]
                                        [P,T2[,overflow[,any_ready]] ...]

The wave runs the schedule of DESIGN.md §4.1 (ready rays first, refill, map loop until P more finished
marches, park step with the own-slot cases, the overflow deposit of csrc/rmr_slot_rule.h, batch at T2 events
or with no active lane) on random paths and charges every wave-level step a fixed number of issue slots: a
map-loop iteration, an outer pass, a shading batch. A batch costs the same at 34 lanes as at 60, which is
the whole argument for fuller batches. `any_ready` is the schedule's possible second step: idle lanes take
any slot's ready ray, and a lane that finds no empty slot swaps with any ready slot.

Inputs (Cornell-5, 1080p, 16 spp, RMR_PROFILE build): march lengths exponential with mean 38 steps (2.97e9
march steps over 78.2e6 events); 42 % of the events end their path or are misses and store at once (78.2e6
events, 45e6 certified continuing hits); 4 bounces. Costs: 130 issue slots per map iteration, 60-180 per
outer pass, 1,550-1,700 per batch.

Calibration (model against the kernel, same inputs):

    setting            model                                   measured
    (8, 32)            shares 0.65 / 0.15 / 0.20 (map, pass,   0.616 / 0.124 / 0.237; 34 events per batch
                       batch); 33 events per batch
    (8, 40) vs (8, 32) 0 %                                     +0.6 %
    (8, 48) vs (8, 32) +3.4 to +4.1 %                          +4.6 % (+4.3 % re-measured with the
                                                               deposit's counters in place)
    large P            no penalty                              (12, 48) +9 %: not reproduced, read the model
                                                               as optimistic
    overflow (8, 32)   -3 %                                    -1.9 %
    overflow (8, 40)   -6.6 %                                  -2.9 %
    overflow (8, 48)   -8 to -10 %; 50 events per batch        -3.3 %; 50.6 events per batch
    overflow (8, 56)   -                                       +7.7 %: ready rays hold the slots the deposits
                                                               need, 8.9 lanes wait per map iteration

The model's lanes per map iteration (56.6 at (8, 32)) is the kernel's map evaluations over its iterations
with the batches' probe evaluations counted in (57.4); without them the kernel has 52.5, and 6.8 of the
64 lanes are idle per iteration where the model has about 3 — the share of the gain the model promises
and the kernel does not deliver.
"""
import argparse
import random


def run(P, T2, overflow, any_ready, units, seed, map_cost, pass_cost, batch_cost, mean=38.0, cheap_p=0.42,
        next_p=0.8, max_bounces=4, TR=4):
    rng = random.Random(seed)
    IDLE, MARCH, HIT = 0, 1, 2
    phase = [IDLE] * 64
    steps = [0] * 64
    cheap = [False] * 64
    bounces = [0] * 64
    sst = [0] * 64          # 0 empty, 1 event, 2 ready ray
    sb = [0] * 64           # the slot's path: bounces
    nxt, nev, stored = 0, 0, 0
    exhausted = False
    cost = {"map": 0.0, "pass": 0.0, "batch": 0.0}
    iters = lane_iters = wait_iters = batches = events = deposits = 0

    def start(l, b):
        phase[l], bounces[l] = MARCH, b
        steps[l] = max(1, int(rng.expovariate(1.0 / mean)) + 1)

    while True:
        cost["pass"] += pass_cost
        for l in range(64):
            if phase[l] == IDLE and sst[l] == 2:
                start(l, sb[l])
                sst[l] = 0
        if any_ready:   # idle lanes take any slot's ready ray, by rank
            givers = [l for l in range(64) if sst[l] == 2]
            takers = [l for l in range(64) if phase[l] == IDLE]
            for t, g in zip(takers, givers):
                start(t, sb[g])
                sst[g] = 0
        if not exhausted:
            idle = [l for l in range(64) if phase[l] == IDLE]
            if idle and (len(idle) >= TR or MARCH not in phase):
                if nxt >= units:
                    exhausted = True
                for l in idle:
                    if nxt < units:
                        start(l, 0)
                        nxt += 1
        if MARCH in phase:
            waiting = phase.count(HIT)
            TL = waiting + P
            while True:
                iters += 1
                cost["map"] += map_cost
                wait_iters += waiting
                for l in range(64):
                    if phase[l] == MARCH:
                        lane_iters += 1
                        steps[l] -= 1
                        if steps[l] == 0:
                            phase[l] = HIT
                            cheap[l] = rng.random() < cheap_p or bounces[l] >= max_bounces
                if MARCH not in phase or phase.count(HIT) >= TL:
                    break
        while True:
            for l in range(64):
                if phase[l] != HIT:
                    continue
                if cheap[l]:
                    stored += 1
                    phase[l] = IDLE
                elif sst[l] != 1:
                    ray = sst[l] == 2
                    rb = sb[l]
                    sb[l] = bounces[l]
                    sst[l] = 1
                    nev += 1
                    phase[l] = IDLE
                    if ray:
                        start(l, rb)
            if overflow:
                cand = [l for l in range(64) if phase[l] == HIT]
                empty = [l for l in range(64) if sst[l] == 0]
                for c, e in zip(cand, empty):
                    sb[e], sst[e] = bounces[c], 1
                    phase[c] = IDLE
                    nev += 1
                    deposits += 1
                if any_ready:   # candidates left over swap with any ready slot
                    cand = [l for l in range(64) if phase[l] == HIT]
                    ready = [l for l in range(64) if sst[l] == 2]
                    for c, r in zip(cand, ready):
                        rb = sb[r]
                        sb[r], sst[r] = bounces[c], 1
                        nev += 1
                        deposits += 1
                        start(c, rb)
            if not (nev and (nev >= T2 or MARCH not in phase)):
                break
            batches += 1
            events += nev
            cost["batch"] += batch_cost
            nev = 0
            for l in range(64):
                if sst[l] == 1:
                    if rng.random() < next_p:
                        sb[l] += 1
                        sst[l] = 2
                    else:
                        sst[l] = 0
                        stored += 1
            if HIT not in phase:
                break
        if exhausted and all(p == IDLE for p in phase) and not any(sst):
            break
    assert stored == units
    total = sum(cost.values())
    return {"total": total, "shares": {k: round(v / total, 3) for k, v in cost.items()},
            "lanes_per_iter": round(lane_iters / iters, 2), "waiting_per_iter": round(wait_iters / iters, 2),
            "events_per_batch": round(events / max(1, batches), 2), "deposits": deposits}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("settings", nargs="*", default=["8,32", "8,40", "8,48", "8,32,1", "8,40,1", "8,48,1", "8,56,1", "8,56,1,1"])
    ap.add_argument("--units", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--map-cost", type=float, default=130.0)
    ap.add_argument("--pass-cost", type=float, default=120.0)
    ap.add_argument("--batch-cost", type=float, default=1600.0)
    a = ap.parse_args()
    base = None
    for s in a.settings:
        f = [int(x) for x in s.split(",")] + [0, 0]
        r = run(f[0], f[1], bool(f[2]), bool(f[3]), a.units, a.seed, a.map_cost, a.pass_cost, a.batch_cost)
        base = base or r["total"]
        print("(%d, %d) overflow %d any_ready %d: %+.1f %% vs the first, shares %s, %.2f lanes / %.2f waiting per "
              "iteration, %.2f events per batch, %d deposits" % (f[0], f[1], f[2], f[3], 100.0 * (r["total"] / base - 1.0),
                                                                  r["shares"], r["lanes_per_iter"], r["waiting_per_iter"],
                                                                  r["events_per_batch"], r["deposits"]))


if __name__ == "__main__":
    main()
