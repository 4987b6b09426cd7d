#!/usr/bin/env python3
"""The dependent launch chain of a pair in a rocprofv3 --kernel-trace CSV (diagnostics).

    python trace_chain.py <kernel_trace.csv> [--skip 1]

Pairs are the launches of one host thread (a lane) from one k_find_header to the next; the first
--skip pairs of every lane are left out.  Prints, as medians over the pairs (us):
  (a) end of k_strip_summary -> start of k_strip_write, per strip (ref = the sweep's stream)
  (b) end of the reference k_strip_write -> start of k_sweep_early
  (c) end of k_sweep_early -> start of the first k_walk
  (d) end of round 1's k_walk -> start of round 2's k_walk
  (e) end of the last k_walk (carry included) -> end of k_long_copy
and the pair's in-lane time (start of k_find_header -> end of its last kernel of that thread),
the launches per pair, and the kernel time inside every interval.
"""
from __future__ import annotations

import argparse
import collections
import csv
import re
import statistics
import sys



def is_k(k, name: str) -> bool:
    """k's kernel is `name` (a template or not), whatever namespace it is in"""
    return re.search(r"(^|[ :])" + name + r"[<(]", k[3]) is not None


def pair_intervals(ks):
    """ks: (start, end, stream, kernel name) of one pair, by start.  -> dict or None"""
    def first(pred, after=0):
        for k in ks:
            if k[0] >= after and pred(k):
                return k
        return None
    sweep = first(lambda k: is_k(k, "k_sweep_early"))
    anyw = [k for k in ks if is_k(k, "k_walk")]
    walks = [k for k in anyw if re.search(r"k_walk<\w+, false>", k[3])]   # the rounds' own (not the carry's)
    lc = [k for k in ks if is_k(k, "k_long_copy")]
    if not sweep or len(walks) < 2 or not lc:
        return None
    out = {}
    for tag, want_ref in (("a_ref", True), ("a_tgt", False)):
        su = first(lambda k: is_k(k, "k_strip_summary") and (k[2] == sweep[2]) == want_ref)
        wr = first(lambda k: is_k(k, "k_strip_write") and k[2] == su[2], su[1]) if su else None
        if not wr:
            return None
        out[tag] = (su[1], wr[0])
        if want_ref:
            out["b"] = (wr[1], sweep[0])
    out["c"] = (sweep[1], walks[0][0])
    out["d"] = (walks[0][1], walks[1][0])
    out["e"] = (max(k[1] for k in anyw), max(k[1] for k in lc))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--skip", type=int, default=1)
    a = ap.parse_args()
    lanes = collections.defaultdict(list)
    every = []
    with open(a.csv) as f:
        for r in csv.DictReader(f):
            k = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Stream_Id"], r["Kernel_Name"])
            lanes[r["Thread_Id"]].append(k)
            every.append(k)
    every.sort()
    acc = collections.defaultdict(list)
    busy = collections.defaultdict(list)
    npairs = 0
    for tid, ks in lanes.items():
        ks.sort()
        heads = [i for i, k in enumerate(ks) if is_k(k, "k_find_header")]
        for n, i0 in enumerate(heads):
            if n < a.skip:
                continue
            i1 = heads[n + 1] if n + 1 < len(heads) else len(ks)
            iv = pair_intervals(ks[i0:i1])
            if not iv:
                continue
            npairs += 1
            t0, t1 = ks[i0][0], max(k[1] for k in ks[i0:i1])
            acc["pair"].append((t1 - t0) / 1e3)
            for tag, (s, e) in iv.items():
                acc[tag].append((e - s) / 1e3)
                # this lane's kernel time inside the interval (union), the rest is waiting
                u, ce = 0, s
                for k in ks[i0:i1]:
                    lo, hi = max(k[0], ce), min(k[1], e)
                    if hi > lo:
                        u += hi - lo
                        ce = hi
                busy[tag].append(u / 1e3)
    if not npairs:
        sys.exit("no complete pair found")
    nh = sum(1 for k in every if is_k(k, "k_find_header"))
    print(f"pairs {npairs} (of {nh}), launches per pair {len(every) / nh:.1f}")
    med = {t: statistics.median(v) for t, v in acc.items()}
    print(f"{'interval':8s} {'median us':>10s} {'p25':>8s} {'p75':>8s} {'own kernels us':>15s}")
    for t in ("a_ref", "a_tgt", "b", "c", "d", "e"):
        v = sorted(acc[t])
        print(f"{t:8s} {med[t]:10.1f} {v[len(v) // 4]:8.1f} {v[3 * len(v) // 4]:8.1f} {statistics.median(busy[t]):15.1f}")
    chain = sum(med[t] for t in ("a_ref", "a_tgt", "b", "c", "d", "e"))
    print(f"sum (a)-(e) {chain:.1f} us; pair in-lane time {med['pair']:.1f} us; share {100 * chain / med['pair']:.1f} %")


if __name__ == "__main__":
    main()
