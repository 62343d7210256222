#!/usr/bin/env python3
"""Reduce a clock dump of the instrumented 16-lane row kernel (vecchia_rows16.hip built with
-DGPBOOST_AMD_ROWS16_PHASE=1, run with GPBOOST_AMD_ROWS16_PHASE_DUMP=<file>) to

  - the waves per SIMD and whether HW_ID's wave slot tells the two waves of a SIMD apart (by value, by parity);
  - the distribution over SIMDs of the two co-resident waves' offset within the trip, at the chosen trips
    (0-based; the distance of their trip tops folded into half a trip, in cycles and as a share of the trip);
  - per wave slot, the trip length by trip and the time from entry to the end of the last elimination;
  - the trip's three segments (top -> covariances stored -> elimination done -> next top), per wave, as
    median and spread: a wait shows as the excess of a segment over its shortest instances.

    python scripts/rows16_phase_offsets.py dump.bin [--trips 1,6,11]
"""
import argparse
import sys
from collections import Counter, defaultdict

import numpy as np


def load(path):
    raw = np.fromfile(path, dtype=np.uint64)
    blocks, stride, tm, prio = (int(x) for x in raw[:4])
    trips, marks = tm & 0xFFFF, tm >> 16
    rec = raw[4:4 + blocks * stride].reshape(blocks, stride)
    return rec, trips, marks, prio


def pct(x, qs=(10, 25, 50, 75, 90)):
    return " / ".join(f"{np.percentile(x, q):.0f}" for q in qs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dump")
    ap.add_argument("--trips", default="1,6,11")
    args = ap.parse_args()
    rec, ntrips, marks, prio = load(args.dump)
    head = 4
    hw, xcc, entry, ran = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64), rec[:, 3].astype(np.int64)
    t = rec[:, head:head + ntrips * marks].astype(np.int64).reshape(len(rec), ntrips, marks)
    slot, simd, cu, sh, se = hw & 15, hw >> 4 & 3, hw >> 8 & 15, hw >> 12 & 1, hw >> 13 & 3
    print(f"waves {len(rec)}, priority turns {prio}, trips per wave: {dict(sorted(Counter(ran.tolist()).items()))}")
    print(f"XCC ids {sorted(set(xcc.tolist()))}, SE {sorted(set(se.tolist()))}, SH {sorted(set(sh.tolist()))}, "
          f"CU {sorted(set(cu.tolist()))}, SIMD {sorted(set(simd.tolist()))}, wave slots {dict(sorted(Counter(slot.tolist()).items()))}")
    groups = defaultdict(list)
    for w in range(len(rec)):
        groups[(xcc[w], se[w], sh[w], cu[w], simd[w])].append(w)
    sizes = Counter(len(v) for v in groups.values())
    print(f"SIMDs {len(groups)}, waves per SIMD: {dict(sorted(sizes.items()))}")
    pairs = [v for v in groups.values() if len(v) == 2]
    same_slot = sum(slot[a] == slot[b] for a, b in pairs)
    same_parity = sum((slot[a] ^ slot[b]) & 1 == 0 for a, b in pairs)
    print(f"pairs {len(pairs)}: same slot {same_slot} (must be 0), same slot parity {same_parity}")
    if not pairs:
        sys.exit("no SIMD holds two waves: nothing to compare")
    pa = np.array(pairs)
    # order each pair (even slot, odd slot) where parity separates them, else by slot
    sw = (slot[pa[:, 0]] & 1) > (slot[pa[:, 1]] & 1)
    pa[sw] = pa[sw][:, ::-1]
    a, b = pa[:, 0], pa[:, 1]
    d0 = entry[b] - entry[a]
    print(f"entry clock, odd-slot wave minus even-slot wave, cycles (p10/25/50/75/90): {pct(d0)}; |.| median {np.median(np.abs(d0)):.0f}")
    full = ran.min()
    tops = t[:, :, 0]
    trip_len = np.diff(tops[:, :min(full, ntrips)], axis=1)
    L = float(np.median(trip_len))
    print(f"trip length, cycles (p10/25/50/75/90 over waves and trips): {pct(trip_len.ravel())}")
    for k in (int(x) for x in args.trips.split(",")):
        both = (ran[a] > k) & (ran[b] > k)
        if k >= ntrips or not both.any():
            continue
        d = np.abs(tops[b[both], k] - tops[a[both], k]) % L
        d = np.minimum(d, L - d)
        print(f"trip {k}: offset of the pair's trip tops folded to half a trip, cycles: {pct(d)}; "
              f"share of the trip: {' / '.join(f'{np.percentile(d, q) / L:.3f}' for q in (10, 25, 50, 75, 90))}; "
              f"pairs under 2 % of a trip: {np.mean(d < 0.02 * L):.2f}, under 10 %: {np.mean(d < 0.1 * L):.2f}")
    last = t[np.arange(len(rec)), np.minimum(ran, ntrips) - 1, marks - 1] - entry
    for sl in sorted(set(slot.tolist())):
        m = slot == sl
        print(f"wave slot {sl}: {m.sum()} waves, {int((ran[m] > full).sum())} with an extra trip; median trip length by "
              f"trip {np.median(np.diff(tops[m, :min(full, ntrips)], axis=1), axis=0).astype(int).tolist()}; entry -> last "
              f"elimination done, cycles (p0/10/50/90/100): {pct(last[m], (0, 10, 50, 90, 100))}")
    kk = min(full, ntrips) - 1
    if marks >= 3 and kk > 0:
        seg = [t[:, :kk, 1] - t[:, :kk, 0], t[:, :kk, 2] - t[:, :kk, 1], t[:, 1:kk + 1, 0] - t[:, :kk, 2]]
        names = ["top -> covariances stored (gather, the records' wait, 30 pairs)",
                 "-> elimination done (border row, row load, 30 pivots)",
                 "-> next top (next set's loads, stash, traces, sums, partials)"]
        for nm, s in zip(names, seg):
            s = s[:, 1:] if s.shape[1] > 1 else s   # trip 0 starts cold
            print(f"segment {nm}: min {s.min()}, p10/25/50/75/90 {pct(s.ravel())}, max {s.max()}; "
                  f"median excess over the shortest {np.median(s) - s.min():.0f}")


if __name__ == "__main__":
    main()
