#!/usr/bin/env python3
"""Region-fetch times on the chr1-sized synthetic pair, beside the full reconstruction.

    python bench_fetch.py [--profile hg --ref-len 247249719 --tgt-len 249250621 --seed 1] [--calls 20] [--warmup 3]
Compresses the pair once, opens a reader on the device-resident record (open ms: host clock around
sccg_reader_open_device, which ends in a synchronise) and times sccg_reader_fetch_device for
1 x 1 kb, 1 x 1 Mb, 1000 x 1 kb and 100,000 x 100 b (seeded random starts): HIP events on the
stream around each call (the region list's copy, the kernel and the call's own host work between
them), the host clock around the same call, and -- in calls of their own -- the kernel alone from
the profiler's "fetch" family.  sccg_reconstruct_device on the same pair in the same process is the
yardstick.  Then sccg_reader_fetch_encoded_device at 1000 x 1 kb and 100,000 x 100 b -- index, one-hot
f16 and f32, ASCII with alternating strands -- each beside the two-step path it replaces: the ASCII
fetch of the same regions followed by a PyTorch lookup-table encode to the same dtype on the same
stream.  Then the cohort: S = 8 readers opened through one shared reference -- the SAME record eight
times, because the generator makes reference and target from one seed and cannot hold the reference
fixed under another target; the kernel's per-span choice of the source is the same -- and a batch
of 1000 x 1 kb and of 100,000 x 100 b spread evenly over the samples in random order, index and
one-hot f16, interleaved call by call: (a) one sccg_cohort_fetch_device, (b) S
sccg_reader_fetch_encoded_device calls of the same regions grouped by sample, (c) the same total
shape from one reader in one call, and (a1) the cohort call over ONE reader listed S times, which
keeps (a)'s per-span descriptor reads and (c)'s memory footprint; with the readers' device bytes and
open times, private against shared.  Then the origin fetch (SCCG_ENC_ORIGIN, 4 bytes per base, R' never
read) beside index (1 byte) and one-hot u8 (the same 4 bytes, R' read) at the same two shapes, one
reader and the S-sample cohort, all through a reference opened with SCCG_REF_COORDS and interleaved
call by call; and sccg_reference_open_device with and without SCCG_REF_COORDS.  --only-origin runs
that last section alone.  --only-locate runs the locate leg alone: sccg_reader_enable_locate (host ms, index
bytes), sccg_reader_locate_device and sccg_cohort_locate_device for 1 / 1,000 / 100,000 random reference
positions (every located base checked against the reference), the 1000 x 1 kb index and origin fetches
of the same run, and Cohort.fetch_tensor_at beside the fetch_tensor it wraps.  --only-segments runs the
segments leg alone: sccg_reader_segments_device / sccg_cohort_segments_device at 1 x 1 Mb, 1000 x 1 kb,
1 x 10 Mb and the whole sequence beside what they replace -- the origin fetch of the same regions plus a run-length coding of its
output on the device in PyTorch -- interleaved call by call, with the segment counts and the bytes either
writes; the segments are checked by expanding them back to the origin fetch's output.  --only-lift runs the
lift leg alone: sccg_reader_lift_device / sccg_cohort_lift_device at 1 x 1 kb, 1 x 1 Mb, 1000 x 1 kb of the
reference and the whole reference beside what they replace -- the locate call of every position of the intervals
plus a run-length coding of its output on the device in PyTorch (not at the whole reference: its query list
alone is 8 bytes per base) -- and, as yardsticks, the locate call alone and the segments call over sequence
regions of the same sizes, interleaved call by call, with the block counts and the bytes either writes; the
blocks are checked row for row against that coding (the whole reference: expanded at 100,000 random
positions against locate).  --only-find runs the find leg alone: sccg_reader_find_device at 1 x 1 Mb, 1000 x 1 kb,
1 x 10 Mb and the whole sequence and sccg_cohort_find_device at 1000 x 1 kb, both strands, for GAATTC, a 20-mer cut
from the sample and N x 21 + GG, beside what the call replaces -- the index fetch of the same regions, then a
PyTorch mask-table compare over m shifted slices and nonzero on the same stream -- interleaved call by call; every
timed result is first checked equal to that baseline's rows.  --only-find-approx runs the find-with-mismatches leg alone:
sccg_*_find_approx_device at the same shapes for a 20-mer cut from the sample plus NGG at K = 0, 2 and 4, both strands,
beside the exact find of the same pattern and what the call replaces -- the index fetch, an integer sum of mask misses
over m shifted slices, `<= K` and nonzero on the same stream -- interleaved call by call and checked the same way.
Every shape's bytes are checked against the target FASTA (an origin r >= 0
must name the reference base the target's base is, -2 an N).  Prints one JSON line
(median, min, max of `calls` calls after `warmup`)."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def cohort_section(a, ctx, lib, torch, sccg, dev, stream, rd, d_ref, ref_len, d_rec, rec_len, truth, code, S=8):
    """Memory and open time, private against shared; then (a) / (b) / (c) interleaved."""
    s = stream.cuda_stream
    L = rd.length
    out = {"samples": S, "same_record": True}

    def opened(fn, close=True):
        ts, h = [], None
        for _ in range(3):
            if h is not None and close:
                h.close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return h, spread(ts)

    ref, out["reference_open_ms"] = opened(lambda: ctx.open_reference_device(d_ref.data_ptr(), ref_len, stream=s))
    prv, out["open_private_ms"] = opened(lambda: ctx.open_reader_device(d_ref.data_ptr(), ref_len, d_rec.data_ptr(), rec_len, s))
    sh0, out["open_shared_ms"] = opened(lambda: ref.open_reader_device(d_rec.data_ptr(), rec_len, s))
    readers = [sh0] + [ref.open_reader_device(d_rec.data_ptr(), rec_len, s) for _ in range(S - 1)]
    out["reader_device_bytes"] = {"private": prv.device_bytes, "shared": sh0.device_bytes, "reference": ref.device_bytes,
                                  f"{S}_private": S * prv.device_bytes, f"{S}_shared_plus_reference": S * sh0.device_bytes + ref.device_bytes}
    prv.close()
    co = sccg.Cohort(readers)
    co1 = sccg.Cohort([readers[0]] * S)   # S table entries, one reader's memory: the descriptor reads without the S-fold footprint
    rng = random.Random(2)
    codes = np.array(code, dtype=np.uint8)
    out["fetch"] = {}
    for name, (n, ln) in {"1000x1kb": (1000, 1000), "100000x100b": (100_000, 100)}.items():
        begins = [rng.randrange(L - ln) for _ in range(n)]
        samp = [k % S for k in range(n)]
        rng.shuffle(samp)
        F = n * ln
        items = (sccg.CohortRegion * n)(*[(b, b + ln, sm, 0) for b, sm in zip(begins, samp)])
        flat = (sccg.Region * n)(*[(b, b + ln) for b in begins])
        groups = [[b for b, sm in zip(begins, samp) if sm == k] for k in range(S)]
        garr = [(sccg.Region * len(g))(*[(b, b + ln) for b in g]) for g in groups]
        fwd = b"".join(truth[b:b + ln] for b in begins)
        grouped = b"".join(truth[b:b + ln] for g in groups for b in g)
        for row, (enc, dt, bpb) in {"index": ("index", "u8", 1), "onehot_f16": ("onehot", "f16", 8)}.items():
            fmt = sccg.FetchFormat(sccg.ENCODINGS[enc], sccg.DTYPES[dt], 0, 0)
            d_o = [torch.empty(F * bpb + 64, dtype=torch.uint8, device=dev) for _ in range(4)]
            got = ctypes.c_size_t()

            def call_a():
                rc = lib.sccg_cohort_fetch_device(co.ptr, items, n, ctypes.byref(fmt), d_o[0].data_ptr(), F * bpb, ctypes.byref(got), s)
                assert rc == 0 and got.value == F * bpb, (rc, got.value)

            def call_b():
                at = 0
                for k in range(S):
                    nb = len(groups[k]) * ln * bpb
                    rc = lib.sccg_reader_fetch_encoded_device(readers[k].ptr, garr[k], len(groups[k]), None, ctypes.byref(fmt),
                                                              d_o[1].data_ptr() + at, nb, ctypes.byref(got), s)
                    assert rc == 0 and got.value == nb, (rc, got.value)
                    at += nb

            def call_c():
                rc = lib.sccg_reader_fetch_encoded_device(readers[0].ptr, flat, n, None, ctypes.byref(fmt), d_o[2].data_ptr(), F * bpb,
                                                          ctypes.byref(got), s)
                assert rc == 0 and got.value == F * bpb, (rc, got.value)

            def call_a1():
                rc = lib.sccg_cohort_fetch_device(co1.ptr, items, n, ctypes.byref(fmt), d_o[3].data_ptr(), F * bpb, ctypes.byref(got), s)
                assert rc == 0 and got.value == F * bpb, (rc, got.value)

            calls = {"a_cohort": call_a, "b_per_sample": call_b, "c_one_reader": call_c, "a1_cohort_of_one_reader": call_a1}
            ev = {k: [] for k in calls}
            for i in range(a.warmup + a.calls):   # interleaved: a, b, c, a, b, c, ...
                for k, call in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    e0.record(stream)
                    call()
                    e1.record(stream)
                    stream.synchronize()
                    if i >= a.warmup:
                        ev[k].append(e0.elapsed_time(e1))
            ctx.profile(True, families=["fetch"])
            for _ in range(a.calls):
                call_a()
            kern = ctx.profile_get().get("fetch", (0.0, 0))
            ctx.profile(False)

            def encoded(seq):
                c = codes[np.frombuffer(seq, dtype=np.uint8)]
                return c.tobytes() if enc == "index" else np.vstack([np.eye(4), np.zeros((1, 4))]).astype(np.float16)[c].tobytes()

            w_flat, w_grouped = encoded(fwd), encoded(grouped)
            exact = [d_o[0][:F * bpb].cpu().numpy().tobytes() == w_flat, d_o[1][:F * bpb].cpu().numpy().tobytes() == w_grouped,
                     d_o[2][:F * bpb].cpu().numpy().tobytes() == w_flat, d_o[3][:F * bpb].cpu().numpy().tobytes() == w_flat]
            med = {k: statistics.median(v) for k, v in ev.items()}
            out["fetch"][f"{name}/{row}"] = {
                "bytes": F * bpb, "event_ms": {k: spread(v) for k, v in ev.items()},
                "kernel_ms_mean": round(kern[0] / max(kern[1], 1), 4), "launches_per_call": kern[1] / a.calls,
                "b_over_a": round(med["b_per_sample"] / med["a_cohort"], 2), "a_over_c": round(med["a_cohort"] / med["c_one_reader"], 3),
                "exact": all(exact)}
            del d_o
    co.close()
    co1.close()
    for r in readers:
        r.close()
    ref.close()
    return out


def origin_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, ref_len, d_rec, rec_len, truth, rfa, code, S=8):
    """Reference open with and without the R' -> R map; index / one-hot u8 / origin, reader and cohort."""
    s = stream.cuda_stream
    out = {"samples": S, "same_record": True}

    def opened(coords):
        ts, h = [], None
        for _ in range(3):
            if h is not None:
                h.close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = ctx.open_reference_device(d_ref.data_ptr(), ref_len, stream=s, coords=coords)
            ts.append((time.perf_counter() - t0) * 1e3)
        return h, spread(ts)

    plain, out["reference_open_ms"] = opened(False)
    ref, out["reference_open_coords_ms"] = opened(True)
    out["reference_device_bytes"] = {"plain": plain.device_bytes, "coords": ref.device_bytes}
    plain.close()
    readers = [ref.open_reader_device(d_rec.data_ptr(), rec_len, s) for _ in range(S)]
    rd, co = readers[0], sccg.Cohort(readers)
    L = rd.length
    Ru = np.frombuffer(rfa.partition(b"\n")[2].replace(b"\n", b"").upper(), dtype=np.uint8)
    Tu = np.frombuffer(truth.upper(), dtype=np.uint8)
    codes = np.array(code, dtype=np.uint8)
    rng = random.Random(3)
    out["fetch"] = {}
    rows = {"index": ("index", "u8", 1), "onehot_u8": ("onehot", "u8", 4), "origin": ("origin", "i32", 4)}
    for name, (n, ln) in {"1000x1kb": (1000, 1000), "100000x100b": (100_000, 100)}.items():
        begins = [rng.randrange(L - ln) for _ in range(n)]
        samp = [k % S for k in range(n)]
        rng.shuffle(samp)
        F = n * ln
        items = (sccg.CohortRegion * n)(*[(b, b + ln, sm, 0) for b, sm in zip(begins, samp)])
        flat = (sccg.Region * n)(*[(b, b + ln) for b in begins])
        pos = (np.array(begins, dtype=np.int64)[:, None] + np.arange(ln, dtype=np.int64)[None, :]).reshape(-1)
        got = ctypes.c_size_t()
        calls, bufs = {}, {}
        for row, (enc, dt, bpb) in rows.items():
            fmt = sccg.FetchFormat(sccg.ENCODINGS[enc], sccg.DTYPES[dt], 0, 0)
            for who in ("reader", "cohort"):
                d_o = torch.empty(F * bpb + 64, dtype=torch.uint8, device=dev)
                bufs[f"{row}/{who}"] = (d_o, bpb)

                def call(fmt=fmt, d_o=d_o, bpb=bpb, who=who):
                    if who == "reader":
                        rc = lib.sccg_reader_fetch_encoded_device(rd.ptr, flat, n, None, ctypes.byref(fmt), d_o.data_ptr(), F * bpb,
                                                                  ctypes.byref(got), s)
                    else:
                        rc = lib.sccg_cohort_fetch_device(co.ptr, items, n, ctypes.byref(fmt), d_o.data_ptr(), F * bpb,
                                                          ctypes.byref(got), s)
                    assert rc == 0 and got.value == F * bpb, (rc, got.value)

                calls[f"{row}/{who}"] = call
        ev = {k: [] for k in calls}
        for i in range(a.warmup + a.calls):   # interleaved: every leg once per round
            for k, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                e0.record(stream)
                call()
                e1.record(stream)
                stream.synchronize()
                if i >= a.warmup:
                    ev[k].append(e0.elapsed_time(e1))
        kern = {}
        for k, call in calls.items():
            ctx.profile(True, families=["fetch"])
            for _ in range(a.calls):
                call()
            t = ctx.profile_get().get("fetch", (0.0, 0))
            ctx.profile(False)
            kern[k] = (round(t[0] / max(t[1], 1), 4), t[1] / a.calls)
        c = codes[Tu[pos]]
        for k, (d_o, bpb) in bufs.items():
            raw = d_o[:F * bpb].cpu().numpy()
            if k.startswith("index"):
                exact = bool(np.array_equal(raw, c))
            elif k.startswith("onehot"):
                exact = bool(np.array_equal(raw.reshape(-1, 4), np.vstack([np.eye(4, dtype=np.uint8), np.zeros((1, 4), dtype=np.uint8)])[c]))
            else:
                o = raw.view("<i4")
                cop = o >= 0
                exact = bool(o.min() >= -2 and o.max() < len(Ru) and np.array_equal(Ru[o[cop]], Tu[pos][cop])
                             and np.all(Tu[pos][o == -2] == ord("N")))
                out["fetch"].setdefault(f"{name}/shares", {"copied": round(float(cop.mean()), 4), "literal": round(float((o == -1).mean()), 4),
                                                           "n_run": round(float((o == -2).mean()), 4)})
            med = statistics.median(ev[k])
            out["fetch"][f"{name}/{k}"] = {"bytes": F * bpb, "event_ms": spread(ev[k]), "kernel_ms_mean": kern[k][0],
                                           "launches_per_call": kern[k][1], "out_GBps": round(F * bpb / med / 1e6, 1), "exact": exact}
        for who in ("reader", "cohort"):
            m = {row: statistics.median(ev[f"{row}/{who}"]) for row in rows}
            out["fetch"][f"{name}/{who}/origin_over_onehot_u8"] = round(m["origin"] / m["onehot_u8"], 3)
        bufs.clear()
        calls.clear()
    co.close()
    for r in readers:
        r.close()
    ref.close()
    return out


def locate_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, ref_len, d_rec, rec_len, truth, rfa, S=8):
    """enable_locate (time, index bytes, tokens); locate of 1 / 1,000 / 100,000 random reference positions, one
    reader and the S-sample cohort, beside the 1000 x 1 kb index and origin fetches of the same run;
    fetch_tensor_at for 1000 x 1 kb against the fetch_tensor it wraps.  HIP events around the device calls."""
    s = stream.cuda_stream
    out = {"samples": S, "same_record": True}
    ref = ctx.open_reference_device(d_ref.data_ptr(), ref_len, stream=s, coords=True)
    readers = [ref.open_reader_device(d_rec.data_ptr(), rec_len, s) for _ in range(S)]
    ts, before = [], readers[0].device_bytes
    for r in readers:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.enable_locate()
        ts.append((time.perf_counter() - t0) * 1e3)
    rd, co = readers[0], sccg.Cohort(readers)
    out["enable_locate_ms"] = spread(ts)
    out["index_bytes"] = rd.device_bytes - before
    out["reader_bytes_before"] = before
    nR = len(rfa.partition(b"\n")[2].replace(b"\n", b""))
    Ru = np.frombuffer(rfa.partition(b"\n")[2].replace(b"\n", b"").upper(), dtype=np.uint8)
    Tu = np.frombuffer(truth.upper(), dtype=np.uint8)
    rng = random.Random(5)

    def events(call):
        ev = []
        for i in range(a.warmup + a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            e0.record(stream)
            call()
            e1.record(stream)
            stream.synchronize()
            if i >= a.warmup:
                ev.append(e0.elapsed_time(e1))
        return ev

    def kernel(call):
        ctx.profile(True, families=["fetch"])
        for _ in range(a.calls):
            call()
        t = ctx.profile_get().get("fetch", (0.0, 0))
        ctx.profile(False)
        return round(t[0] / max(t[1], 1), 4), t[1] / a.calls

    out["locate"] = {}
    for n in (1, 1000, 100_000):
        q = [rng.randrange(nR) for _ in range(n)]
        qa = (ctypes.c_int64 * n)(*q)
        loci = (sccg.CohortLocus * n)(*[(r, k % S, 0) for k, r in enumerate(q)])
        d_pos = torch.empty(n, dtype=torch.int64, device=dev)
        d_cp = torch.empty(n, dtype=torch.int32, device=dev)

        def reader_call():
            assert lib.sccg_reader_locate_device(rd.ptr, qa, n, d_pos.data_ptr(), d_cp.data_ptr(), s) == 0

        def cohort_call():
            assert lib.sccg_cohort_locate_device(co.ptr, loci, n, d_pos.data_ptr(), d_cp.data_ptr(), s) == 0

        for who, call in (("reader", reader_call), ("cohort", cohort_call)):
            ev = events(call)
            km, lpc = kernel(call)
            pos, cp = d_pos.cpu().numpy(), d_cp.cpu().numpy()
            hit = pos >= 0
            qn = np.array(q, dtype=np.int64)
            exact = bool(np.array_equal(Tu[pos[hit]], Ru[qn[hit]]) and np.all(cp[hit] >= 1) and np.all(cp[~hit] == 0))
            out["locate"][f"{n}/{who}"] = {"event_ms": spread(ev), "kernel_ms_mean": km, "launches_per_call": lpc,
                                          "found": round(float(hit.mean()), 4), "max_copies": int(cp.max()), "exact": exact}
    # the yardsticks of the same run: 1000 x 1 kb index and origin fetches, and fetch_tensor_at beside fetch_tensor
    L, n, ln = rd.length, 1000, 1000
    begins = [rng.randrange(L - ln) for _ in range(n)]
    flat = (sccg.Region * n)(*[(b, b + ln) for b in begins])
    got = ctypes.c_size_t()
    out["fetch"] = {}
    for row, (enc, dt, bpb) in {"index": ("index", "u8", 1), "origin": ("origin", "i32", 4)}.items():
        fmt = sccg.FetchFormat(sccg.ENCODINGS[enc], sccg.DTYPES[dt], 0, 0)
        d_o = torch.empty(n * ln * bpb + 64, dtype=torch.uint8, device=dev)

        def call():
            assert lib.sccg_reader_fetch_encoded_device(rd.ptr, flat, n, None, ctypes.byref(fmt), d_o.data_ptr(), n * ln * bpb,
                                                        ctypes.byref(got), s) == 0

        ev = events(call)
        out["fetch"][f"1000x1kb/{row}/reader"] = {"event_ms": spread(ev), "kernel_ms_mean": kernel(call)[0]}
    items = [(k % S, rng.randrange(nR)) for k in range(n)]
    pos, _ = co.locate(items)
    windows = [(sm, int(p), int(p) + ln) for (sm, _), p in zip(items, pos.tolist()) if p >= 0 and p + ln <= L]
    ev_at = events(lambda: co.fetch_tensor_at(items, ln, "index"))
    ev_ft = events(lambda: co.fetch_tensor(windows, "index"))
    out["fetch_tensor_at"] = {"items": n, "found": len(windows), "at_event_ms": spread(ev_at), "fetch_tensor_event_ms": spread(ev_ft)}
    co.close()
    for r in readers:
        r.close()
    ref.close()
    return out


def segments_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, ref_len, d_rec, rec_len, S=8):
    """The segments call beside the origin fetch + a run-length coding in PyTorch, reader and S-sample cohort."""
    s = stream.cuda_stream
    out = {"samples": S, "same_record": True, "shapes": {}}
    ref = ctx.open_reference_device(d_ref.data_ptr(), ref_len, stream=s, coords=True)
    readers = [ref.open_reader_device(d_rec.data_ptr(), rec_len, s) for _ in range(S)]
    rd, co = readers[0], sccg.Cohort(readers)
    L = rd.length
    rng = random.Random(7)
    fmt = sccg.FetchFormat(sccg.ENCODINGS["origin"], sccg.DTYPES["i32"], 0, 0)
    # (the whole sequence is beyond the three shapes asked for: where the one-launch origin fetch's bytes outweigh
    # the segments call's six launches)
    for name, (n, ln) in {"1x1Mb": (1, 1_000_000), "1000x1kb": (1000, 1000), "1x10Mb": (1, 10_000_000), "1xwhole": (1, L)}.items():
        begins = [rng.randrange(L - ln + 1) for _ in range(n)]
        samp = [k % S for k in range(n)]
        rng.shuffle(samp)
        F = n * ln
        flat = (sccg.Region * n)(*[(b, b + ln) for b in begins])
        items = (sccg.CohortRegion * n)(*[(b, b + ln, sm, 0) for b, sm in zip(begins, samp)])
        d_org = torch.empty(F, dtype=torch.int32, device=dev)
        d_beg = torch.tensor(begins, dtype=torch.int64, device=dev)
        got = ctypes.c_size_t()
        for who in ("reader", "cohort"):
            seg_call = lib.sccg_reader_segments_device if who == "reader" else lib.sccg_cohort_segments_device
            h, regs = (rd.ptr, flat) if who == "reader" else (co.ptr, items)
            assert seg_call(h, regs, n, None, None, 0, ctypes.byref(got), s) == 0   # the size query, outside the timing
            m = got.value
            d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            d_seg = torch.empty((m, 3), dtype=torch.int64, device=dev)
            rle = [None]

            def segments():
                assert seg_call(h, regs, n, d_off.data_ptr(), d_seg.data_ptr(), m, ctypes.byref(got), s) == 0 and got.value == m

            def size_query():
                assert seg_call(h, regs, n, None, None, 0, ctypes.byref(got), s) == 0 and got.value == m

            def origin():
                if who == "reader":
                    rc = lib.sccg_reader_fetch_encoded_device(h, regs, n, None, ctypes.byref(fmt), d_org.data_ptr(), 4 * F, ctypes.byref(got), s)
                else:
                    rc = lib.sccg_cohort_fetch_device(h, regs, n, ctypes.byref(fmt), d_org.data_ptr(), 4 * F, ctypes.byref(got), s)
                assert rc == 0 and got.value == 4 * F, (rc, got.value)

            def origin_rle():
                origin()
                o = d_org.view(n, ln)
                start = torch.ones((n, ln), dtype=torch.bool, device=dev)
                start[:, 1:] = ~torch.where(o[:, :-1] >= 0, o[:, 1:] == o[:, :-1] + 1, o[:, 1:] == o[:, :-1])
                at = torch.nonzero(start.view(-1)).view(-1)   # (a host wait for the count, as the segments call's one read)
                end = torch.cat([at[1:], torch.tensor([F], dtype=torch.int64, device=dev)])
                row = torch.div(at, ln, rounding_mode="floor")
                rle[0] = torch.stack([d_beg[row] + (at - row * ln), end - at, d_org[at].long()], dim=1)

            calls = {"segments": segments, "size_query": size_query, "origin_fetch": origin, "origin_fetch_plus_rle": origin_rle}
            ev = {k: [] for k in calls}
            for i in range(a.warmup + a.calls):   # interleaved: every leg once per round
                for k, call in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    e0.record(stream)
                    call()
                    e1.record(stream)
                    stream.synchronize()
                    if i >= a.warmup:
                        ev[k].append(e0.elapsed_time(e1))
            ctx.profile(True, families=["fetch"])
            for _ in range(a.calls):
                segments()
            kern = ctx.profile_get().get("fetch", (0.0, 0))
            ctx.profile(False)
            ln_ = d_seg[:, 1]
            k_in = torch.arange(F, device=dev) - torch.repeat_interleave(torch.cumsum(ln_, 0) - ln_, ln_)
            r_in = torch.repeat_interleave(d_seg[:, 2], ln_)
            exact = bool(int(ln_.sum()) == F and torch.equal(torch.where(r_in >= 0, r_in + k_in, r_in), d_org.long())
                         and torch.equal(rle[0], d_seg) and int(d_off[-1]) == m)
            med = {k: statistics.median(v) for k, v in ev.items()}
            out["shapes"][f"{name}/{who}"] = {
                "bases": F, "segments": m, "segment_bytes": 24 * m + 8 * (n + 1), "origin_bytes": 4 * F,
                "event_ms": {k: spread(v) for k, v in ev.items()}, "kernels_ms_per_call": round(kern[0] / a.calls, 4),
                "launches_per_call": kern[1] / a.calls, "origin_over_segments": round(med["origin_fetch"] / med["segments"], 2),
                "origin_rle_over_segments": round(med["origin_fetch_plus_rle"] / med["segments"], 2), "exact": exact}
            del d_off, d_seg, k_in, r_in
            rle[0] = None
        del d_org
    co.close()
    for r in readers:
        r.close()
    ref.close()
    return out


def lift_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, ref_len, d_rec, rec_len, rfa, S=8):
    """The lift call beside locate of every position + a run-length coding in PyTorch, reader and S-sample cohort."""
    s = stream.cuda_stream
    out = {"samples": S, "same_record": True, "shapes": {}}
    ref = ctx.open_reference_device(d_ref.data_ptr(), ref_len, stream=s, coords=True)
    readers = [ref.open_reader_device(d_rec.data_ptr(), rec_len, s) for _ in range(S)]
    for r in readers:
        r.enable_locate()
    rd, co = readers[0], sccg.Cohort(readers)
    L = rd.length
    nR = len(rfa.partition(b"\n")[2].replace(b"\n", b""))
    rng = random.Random(9)
    PER_BASE = 16_000_000   # the most bases the per-base legs are run at
    for name, (n, ln) in {"1x1kb": (1, 1000), "1x1Mb": (1, 1_000_000), "1000x1kb": (1000, 1000), "1xwhole": (1, nR)}.items():
        begins = [rng.randrange(nR - ln + 1) for _ in range(n)]
        samp = [k % S for k in range(n)]
        rng.shuffle(samp)
        F = n * ln
        per_base = F <= PER_BASE
        flat = (sccg.Region * n)(*[(b, b + ln) for b in begins])
        items = (sccg.CohortRegion * n)(*[(b, b + ln, sm, 0) for b, sm in zip(begins, samp)])
        sl = min(ln, L)   # the segments yardstick: sequence regions of the same sizes
        sflat = (sccg.Region * n)(*[(min(b, L - sl), min(b, L - sl) + sl) for b in begins])
        sitems = (sccg.CohortRegion * n)(*[(min(b, L - sl), min(b, L - sl) + sl, sm, 0) for b, sm in zip(begins, samp)])
        q = np.concatenate([np.arange(b, b + ln, dtype=np.int64) for b in begins]) if per_base else None
        qp = q.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if per_base else None
        d_pos = torch.empty(F if per_base else 1, dtype=torch.int64, device=dev)
        d_beg = torch.tensor(begins, dtype=torch.int64, device=dev)
        got = ctypes.c_size_t()
        for who in ("reader", "cohort"):
            lift_call = lib.sccg_reader_lift_device if who == "reader" else lib.sccg_cohort_lift_device
            seg_call = lib.sccg_reader_segments_device if who == "reader" else lib.sccg_cohort_segments_device
            h, regs, sregs = (rd.ptr, flat, sflat) if who == "reader" else (co.ptr, items, sitems)
            assert lift_call(h, regs, n, None, None, 0, ctypes.byref(got), s) == 0   # the size queries, outside the timing
            m = got.value
            assert seg_call(h, sregs, n, None, None, 0, ctypes.byref(got), s) == 0
            ms = got.value
            d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            d_blk = torch.empty((m, 3), dtype=torch.int64, device=dev)
            d_seg = torch.empty((ms, 3), dtype=torch.int64, device=dev)
            loci = None
            if per_base and who == "cohort":
                loci = (sccg.CohortLocus * F)()
                view = np.frombuffer(loci, dtype=np.dtype([("r", "<i8"), ("s", "<i4"), ("f", "<u4")]))
                view["r"], view["s"] = q, np.repeat(np.array(samp, dtype=np.int32), ln)
            rle = [None]

            def lift():
                assert lift_call(h, regs, n, d_off.data_ptr(), d_blk.data_ptr(), m, ctypes.byref(got), s) == 0 and got.value == m

            def size_query():
                assert lift_call(h, regs, n, None, None, 0, ctypes.byref(got), s) == 0 and got.value == m

            def segments():
                assert seg_call(h, sregs, n, None, d_seg.data_ptr(), ms, ctypes.byref(got), s) == 0 and got.value == ms

            def locate():
                if who == "reader":
                    rc = lib.sccg_reader_locate_device(h, qp, F, d_pos.data_ptr(), None, s)
                else:
                    rc = lib.sccg_cohort_locate_device(h, loci, F, d_pos.data_ptr(), None, s)
                assert rc == 0, rc

            def locate_rle():
                locate()
                o = d_pos.view(n, ln)
                start = torch.ones((n, ln), dtype=torch.bool, device=dev)
                start[:, 1:] = ~torch.where(o[:, :-1] >= 0, o[:, 1:] == o[:, :-1] + 1, o[:, 1:] == o[:, :-1])
                at = torch.nonzero(start.view(-1)).view(-1)   # (a host wait for the count, as the lift call's one read)
                end = torch.cat([at[1:], torch.tensor([F], dtype=torch.int64, device=dev)])
                row = torch.div(at, ln, rounding_mode="floor")
                rle[0] = torch.stack([d_beg[row] + (at - row * ln), end - at, d_pos[at]], dim=1)

            calls = {"lift": lift, "size_query": size_query, "segments_same_sizes": segments}
            if per_base:
                calls.update({"locate": locate, "locate_plus_rle": locate_rle})
            ev = {k: [] for k in calls}
            for i in range(a.warmup + a.calls):   # interleaved: every leg once per round
                for k, call in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    e0.record(stream)
                    call()
                    e1.record(stream)
                    stream.synchronize()
                    if i >= a.warmup:
                        ev[k].append(e0.elapsed_time(e1))
            ctx.profile(True, families=["fetch"])
            for _ in range(a.calls):
                lift()
            kern = ctx.profile_get().get("fetch", (0.0, 0))
            ctx.profile(False)
            ln_ = d_blk[:, 1]
            exact = bool(int(ln_.sum()) == F and int(d_off[-1]) == m and bool((ln_ > 0).all()))
            if per_base:
                exact = exact and torch.equal(rle[0], d_blk)
            else:   # expanded at random positions against locate (one interval: the block of r is the last with ref <= r)
                qs = np.sort(np.array([rng.randrange(nR) for _ in range(100_000)], dtype=np.int64))
                want = (rd.locate(qs)[0] if who == "reader" else co.locate([(samp[0], int(r)) for r in qs])[0])
                blk = d_blk.cpu().numpy()
                k = np.searchsorted(blk[:, 0], qs, side="right") - 1
                exact = exact and bool(np.array_equal(np.where(blk[k, 2] >= 0, blk[k, 2] + (qs - blk[k, 0]), blk[k, 2]), want))
            med = {k: statistics.median(v) for k, v in ev.items()}
            row = {"bases": F, "blocks": m, "block_bytes": 24 * m + 8 * (n + 1), "locate_bytes": 8 * F, "segments_same_sizes": ms,
                   "event_ms": {k: spread(v) for k, v in ev.items()}, "kernels_ms_per_call": round(kern[0] / a.calls, 4),
                   "launches_per_call": kern[1] / a.calls, "exact": exact}
            if per_base:
                row["locate_over_lift"] = round(med["locate"] / med["lift"], 2)
                row["locate_rle_over_lift"] = round(med["locate_plus_rle"] / med["lift"], 2)
            out["shapes"][f"{name}/{who}"] = row
            del d_off, d_blk, d_seg, loci
            rle[0] = None
        del d_pos, q
    co.close()
    for r in readers:
        r.close()
    ref.close()
    return out


def find_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, ref_len, d_rec, rec_len, truth, S=8):
    """The find call beside what it replaces -- an index fetch, then a PyTorch mask-table compare over m shifted
    slices and nonzero, on the same stream -- for one reader at four shapes and the S-sample cohort at 1000 x 1 kb."""
    s = stream.cuda_stream
    out = {"samples": S, "same_record": True, "shapes": {}}
    ref = ctx.open_reference_device(d_ref.data_ptr(), ref_len, stream=s)
    readers = [ref.open_reader_device(d_rec.data_ptr(), rec_len, s) for _ in range(S)]
    rd, co = readers[0], sccg.Cohort(readers)
    L = rd.length
    rng = random.Random(7)
    at = next(k for k in (rng.randrange(L - 20) for _ in range(10_000)) if all(c in b"ACGT" for c in truth[k:k + 20].upper()))
    patterns = {"GAATTC": "GAATTC", "20mer": truth[at:at + 20].decode().upper(), "N21GG": "N" * 21 + "GG"}
    out["patterns"] = patterns
    shapes = [("1x1Mb", "reader", 1, 1_000_000), ("1000x1kb", "reader", 1000, 1000), ("1000x1kb", "cohort", 1000, 1000),
              ("1x10Mb", "reader", 1, 10_000_000), ("1xwhole", "reader", 1, L)]
    for name, who, n, ln in shapes:
        begins = [rng.randrange(L - ln + 1) for _ in range(n)]
        samp = [k % S for k in range(n)]
        rng.shuffle(samp)
        regions = [(b, b + ln) for b in begins]
        flat = (sccg.Region * n)(*regions)
        items = (sccg.CohortRegion * n)(*[(b, b + ln, sm, 0) for b, sm in zip(begins, samp)])
        citems = [(sm, b, b + ln) for b, sm in zip(begins, samp)]
        d_beg = torch.tensor(begins, dtype=torch.int64, device=dev)
        call = lib.sccg_reader_find_device if who == "reader" else lib.sccg_cohort_find_device
        h, regs = (rd.ptr, flat) if who == "reader" else (co.ptr, items)
        got = ctypes.c_size_t()
        for pname, pat in patterns.items():
            pb, m = pat.encode(), len(pat)
            fwd, rev = sccg.find_pattern_masks(pat)
            mk = [torch.tensor(list(x), dtype=torch.uint8, device=dev) for x in (fwd, rev)]
            assert call(h, pb, m, regs, n, 3, None, None, 0, ctypes.byref(got), s) == 0   # the size query, outside the timing
            hits = got.value
            d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            d_hit = torch.empty((max(hits, 1), 2), dtype=torch.int64, device=dev)
            base = [None, None]

            def find():
                assert call(h, pb, m, regs, n, 3, d_off.data_ptr(), d_hit.data_ptr(), hits, ctypes.byref(got), s) == 0 and got.value == hits

            def size_query():
                assert call(h, pb, m, regs, n, 3, None, None, 0, ctypes.byref(got), s) == 0 and got.value == hits

            def fetch_compare():
                c = rd.fetch_tensor(regions, "index", stream=stream) if who == "reader" else co.fetch_tensor(citems, "index", stream=stream)
                c = c.view(n, ln)
                K = ln - m + 1
                acc = torch.ones((n, K, 2), dtype=torch.bool, device=dev)
                for t in range(m):   # a code's bit of the letter's mask; code 4 shifts every mask to 0
                    w = c[:, t:t + K]
                    acc[:, :, 0] &= (torch.bitwise_right_shift(mk[0][t], w) & 1).bool()
                    acc[:, :, 1] &= (torch.bitwise_right_shift(mk[1][t], w) & 1).bool()
                at = torch.nonzero(acc)   # (a host wait for the count, as the find call's one read): rows (region, start, strand)
                base[0] = torch.stack([d_beg[at[:, 0]] + at[:, 1], at[:, 2]], dim=1)
                base[1] = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(acc.sum(dim=(1, 2)), 0)])

            fetch_compare()   # every timed result is first checked equal to the baseline's rows
            find()
            stream.synchronize()
            exact = bool(torch.equal(base[0], d_hit[:hits]) and torch.equal(base[1], d_off))
            calls = {"find": find, "size_query": size_query, "fetch_plus_compare": fetch_compare}
            ev = {k: [] for k in calls}
            for i in range(a.warmup + a.calls):   # interleaved: every leg once per round
                for k, leg in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    e0.record(stream)
                    leg()
                    e1.record(stream)
                    stream.synchronize()
                    if i >= a.warmup:
                        ev[k].append(e0.elapsed_time(e1))
            exact = exact and bool(torch.equal(base[0], d_hit[:hits]) and torch.equal(base[1], d_off))
            ctx.profile(True, families=["fetch"])
            for _ in range(a.calls):
                find()
            kern = ctx.profile_get().get("fetch", (0.0, 0))
            ctx.profile(False)
            med = {k: statistics.median(v) for k, v in ev.items()}
            out["shapes"][f"{name}/{who}/{pname}"] = {
                "bases": n * ln, "hits": hits, "hit_bytes": 16 * hits + 8 * (n + 1), "index_bytes": n * ln,
                "event_ms": {k: spread(v) for k, v in ev.items()}, "kernels_ms_per_call": round(kern[0] / a.calls, 4),
                "launches_per_call": kern[1] / a.calls, "compare_over_find": round(med["fetch_plus_compare"] / med["find"], 2),
                "exact": exact}
            base[0] = base[1] = None
            del d_off, d_hit
            print(f"# find {name}/{who}/{pname}: {out['shapes'][f'{name}/{who}/{pname}']}", file=sys.stderr, flush=True)
    co.close()
    for r in readers:
        r.close()
    ref.close()
    return out


def find_approx_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, ref_len, d_rec, rec_len, truth, S=8):
    """The find-approx call for a guide + PAM (a 20-mer cut from the sample, then NGG) at K = 0, 2 and 4, both strands,
    beside (a) the exact find of the same pattern and (b) what the call replaces -- an index fetch, then an integer
    sum of mask misses over m shifted slices, `<= K` and nonzero, on the same stream -- interleaved call by call, for
    one reader at four shapes and the S-sample cohort at 1000 x 1 kb."""
    s = stream.cuda_stream
    out = {"samples": S, "same_record": True, "shapes": {}}
    ref = ctx.open_reference_device(d_ref.data_ptr(), ref_len, stream=s)
    readers = [ref.open_reader_device(d_rec.data_ptr(), rec_len, s) for _ in range(S)]
    rd, co = readers[0], sccg.Cohort(readers)
    L = rd.length
    rng = random.Random(7)
    at = next(k for k in (rng.randrange(L - 20) for _ in range(10_000)) if all(c in b"ACGT" for c in truth[k:k + 20].upper()))
    pat = truth[at:at + 20].decode().upper() + "NGG"
    out["pattern"] = pat
    pb, m = pat.encode(), len(pat)
    fwd, rev = sccg.find_pattern_masks(pat)
    mk = [torch.tensor(list(x), dtype=torch.uint8, device=dev) for x in (fwd, rev)]
    shapes = [("1x1Mb", "reader", 1, 1_000_000), ("1000x1kb", "reader", 1000, 1000), ("1000x1kb", "cohort", 1000, 1000),
              ("1x10Mb", "reader", 1, 10_000_000), ("1xwhole", "reader", 1, L)]
    for name, who, n, ln in shapes:
        begins = [rng.randrange(L - ln + 1) for _ in range(n)]
        samp = [k % S for k in range(n)]
        rng.shuffle(samp)
        regions = [(b, b + ln) for b in begins]
        flat = (sccg.Region * n)(*regions)
        items = (sccg.CohortRegion * n)(*[(b, b + ln, sm, 0) for b, sm in zip(begins, samp)])
        citems = [(sm, b, b + ln) for b, sm in zip(begins, samp)]
        d_beg = torch.tensor(begins, dtype=torch.int64, device=dev)
        approx = lib.sccg_reader_find_approx_device if who == "reader" else lib.sccg_cohort_find_approx_device
        exact_find = lib.sccg_reader_find_device if who == "reader" else lib.sccg_cohort_find_device
        h, regs = (rd.ptr, flat) if who == "reader" else (co.ptr, items)
        got = ctypes.c_size_t()
        assert exact_find(h, pb, m, regs, n, 3, None, None, 0, ctypes.byref(got), s) == 0
        ehits = got.value
        e_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        e_hit = torch.empty((max(ehits, 1), 2), dtype=torch.int64, device=dev)
        for K in (0, 2, 4):
            assert approx(h, pb, m, regs, n, 3, K, None, None, 0, ctypes.byref(got), s) == 0   # the size query, outside the timing
            hits = got.value
            d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            d_hit = torch.empty((max(hits, 1), 3), dtype=torch.int64, device=dev)
            base = [None, None]

            def find_approx():
                assert approx(h, pb, m, regs, n, 3, K, d_off.data_ptr(), d_hit.data_ptr(), hits, ctypes.byref(got), s) == 0 and got.value == hits

            def find():
                assert exact_find(h, pb, m, regs, n, 3, e_off.data_ptr(), e_hit.data_ptr(), ehits, ctypes.byref(got), s) == 0

            def fetch_sum():
                c = rd.fetch_tensor(regions, "index", stream=stream) if who == "reader" else co.fetch_tensor(citems, "index", stream=stream)
                c = c.view(n, ln)
                C = ln - m + 1
                d = torch.zeros((n, C, 2), dtype=torch.uint8, device=dev)
                for t in range(m):   # 1 where the letter's mask lacks the code's bit; code 4 shifts every mask to 0
                    w = c[:, t:t + C]
                    d[:, :, 0] += (torch.bitwise_right_shift(mk[0][t], w) & 1) ^ 1
                    d[:, :, 1] += (torch.bitwise_right_shift(mk[1][t], w) & 1) ^ 1
                ok = d <= K
                at = torch.nonzero(ok)   # (a host wait for the count, as the call's one read): rows (region, start, strand)
                base[0] = torch.stack([d_beg[at[:, 0]] + at[:, 1], at[:, 2], d[at[:, 0], at[:, 1], at[:, 2]].to(torch.int64)], dim=1)
                base[1] = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(ok.sum(dim=(1, 2)), 0)])

            fetch_sum()   # every timed result is first checked equal to the baseline's rows
            find_approx()
            stream.synchronize()
            exact = bool(torch.equal(base[0], d_hit[:hits]) and torch.equal(base[1], d_off))
            calls = {"find_approx": find_approx, "find": find, "fetch_plus_sum": fetch_sum}
            ev = {k: [] for k in calls}
            for i in range(a.warmup + a.calls):   # interleaved: every leg once per round
                for k, leg in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    e0.record(stream)
                    leg()
                    e1.record(stream)
                    stream.synchronize()
                    if i >= a.warmup:
                        ev[k].append(e0.elapsed_time(e1))
            exact = exact and bool(torch.equal(base[0], d_hit[:hits]) and torch.equal(base[1], d_off))
            if K == 0:
                exact = exact and hits == ehits and bool(torch.equal(d_hit[:hits, :2], e_hit[:ehits]) and torch.equal(d_off, e_off))
            ctx.profile(True, families=["fetch"])
            for _ in range(a.calls):
                find_approx()
            kern = ctx.profile_get().get("fetch", (0.0, 0))
            ctx.profile(False)
            med = {k: statistics.median(v) for k, v in ev.items()}
            key = f"{name}/{who}/K{K}"
            out["shapes"][key] = {
                "bases": n * ln, "hits": hits, "hit_bytes": 24 * hits + 8 * (n + 1), "index_bytes": n * ln,
                "event_ms": {k: spread(v) for k, v in ev.items()}, "kernels_ms_per_call": round(kern[0] / a.calls, 4),
                "launches_per_call": kern[1] / a.calls, "sum_over_find_approx": round(med["fetch_plus_sum"] / med["find_approx"], 2),
                "find_approx_over_find": round(med["find_approx"] / med["find"], 2), "exact": exact}
            base[0] = base[1] = None
            del d_off, d_hit
            print(f"# find-approx {key}: {out['shapes'][key]}", file=sys.stderr, flush=True)
        del e_off, e_hit
    co.close()
    for r in readers:
        r.close()
    ref.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", default="hg")
    ap.add_argument("--ref-len", type=int, default=247_249_719)
    ap.add_argument("--tgt-len", type=int, default=249_250_621)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-origin", action="store_true", help="the origin section alone")
    ap.add_argument("--only-locate", action="store_true", help="the locate section alone")
    ap.add_argument("--only-segments", action="store_true", help="the segments section alone")
    ap.add_argument("--only-lift", action="store_true", help="the lift section alone")
    ap.add_argument("--only-find", action="store_true", help="the find section alone")
    ap.add_argument("--only-find-approx", action="store_true", help="the find-with-mismatches section alone")
    a = ap.parse_args()
    import torch
    import sccg
    import synth
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    rfa, tfa = synth.synth_pair(a.profile, a.ref_len, a.tgt_len, a.seed)
    truth = tfa.partition(b"\n")[2].replace(b"\n", b"")
    ctx = sccg.Context(0)
    lib = ctx.lib
    rec_h = ctx.compress(rfa, tfa)
    d_ref = torch.frombuffer(bytearray(rfa), dtype=torch.uint8).to(dev)
    d_rec = torch.frombuffer(bytearray(rec_h), dtype=torch.uint8).to(dev)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream

    def timed(call):
        """(event ms, host ms) of `calls` calls after `warmup`"""
        ev, host = [], []
        for i in range(a.warmup + a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            t0 = time.perf_counter()
            e0.record(stream)
            call()
            e1.record(stream)
            stream.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                ev.append(e0.elapsed_time(e1))
                host.append((t1 - t0) * 1e3)
        return ev, host

    code = [4] * 256
    for k, ch in enumerate(b"ACGT"):
        code[ch] = code[ch + 32] = k
    if a.only_find_approx:
        out = {"pair": f"{a.profile}-{a.ref_len}-{a.tgt_len}-{a.seed}", "record_bytes": len(rec_h), "calls": a.calls,
               "find_approx": find_approx_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, len(rfa), d_rec, len(rec_h), truth)}
        ctx.close()
        print(json.dumps(out))
        if not all(v["exact"] for v in out["find_approx"]["shapes"].values()):
            raise SystemExit("bench_fetch: find-approx section: the hits are not the rows of the fetch-and-sum baseline")
        return
    if a.only_find:
        out = {"pair": f"{a.profile}-{a.ref_len}-{a.tgt_len}-{a.seed}", "record_bytes": len(rec_h), "calls": a.calls,
               "find": find_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, len(rfa), d_rec, len(rec_h), truth)}
        ctx.close()
        print(json.dumps(out))
        if not all(v["exact"] for v in out["find"]["shapes"].values()):
            raise SystemExit("bench_fetch: find section: the hits are not the rows of the fetch-and-compare baseline")
        return
    if a.only_lift:
        out = {"pair": f"{a.profile}-{a.ref_len}-{a.tgt_len}-{a.seed}", "record_bytes": len(rec_h), "calls": a.calls,
               "lift": lift_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, len(rfa), d_rec, len(rec_h), rfa)}
        ctx.close()
        print(json.dumps(out))
        if not all(v["exact"] for v in out["lift"]["shapes"].values()):
            raise SystemExit("bench_fetch: lift section: the blocks are not the run-length coding of locate's answers")
        return
    if a.only_segments:
        out = {"pair": f"{a.profile}-{a.ref_len}-{a.tgt_len}-{a.seed}", "record_bytes": len(rec_h), "calls": a.calls,
               "segments": segments_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, len(rfa), d_rec, len(rec_h))}
        ctx.close()
        print(json.dumps(out))
        if not all(v["exact"] for v in out["segments"]["shapes"].values()):
            raise SystemExit("bench_fetch: segments section: the segments do not expand to the origin fetch")
        return
    if a.only_locate:
        loc = locate_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, len(rfa), d_rec, len(rec_h), truth, rfa)
        loc["record_line_tokens"] = rec_h.rstrip(b"\n").rpartition(b"\n")[2].count(b"(")   # (zero-length ones included)
        out = {"pair": f"{a.profile}-{a.ref_len}-{a.tgt_len}-{a.seed}", "record_bytes": len(rec_h), "calls": a.calls, "locate": loc}
        ctx.close()
        print(json.dumps(out))
        if not all(v["exact"] for v in loc["locate"].values()):
            raise SystemExit("bench_fetch: locate section: a located base is not the reference's")
        return
    if a.only_origin:
        out = {"pair": f"{a.profile}-{a.ref_len}-{a.tgt_len}-{a.seed}", "record_bytes": len(rec_h), "calls": a.calls,
               "origin": origin_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, len(rfa), d_rec, len(rec_h), truth, rfa, code)}
        ctx.close()
        print(json.dumps(out))
        if not all(v["exact"] for v in out["origin"]["fetch"].values() if isinstance(v, dict) and "exact" in v):
            raise SystemExit("bench_fetch: origin section: bytes differ from the target FASTA")
        return

    # ---- yardstick: the full reconstruction
    need = ctx.reconstruct_device(d_ref.data_ptr(), len(rfa), d_rec.data_ptr(), len(rec_h), 0, 0, s)
    d_fa = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    ev, host = timed(lambda: ctx.reconstruct_device(d_ref.data_ptr(), len(rfa), d_rec.data_ptr(), len(rec_h),
                                                    d_fa.data_ptr(), need + 64, s))
    out = {"pair": f"{a.profile}-{a.ref_len}-{a.tgt_len}-{a.seed}", "record_bytes": len(rec_h), "calls": a.calls,
           "reconstruct_device": {"event_ms": spread(ev), "host_ms": spread(host), "out_bytes": need}}
    del d_fa

    # ---- open
    opens = []
    rd = None
    for _ in range(3):
        if rd is not None:
            rd.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rd = ctx.open_reader_device(d_ref.data_ptr(), len(rfa), d_rec.data_ptr(), len(rec_h), s)
        opens.append((time.perf_counter() - t0) * 1e3)
    out["open_ms"] = spread(opens)
    L = rd.length
    assert L == len(truth)

    # ---- fetch shapes
    rng = random.Random(1)
    shapes = {"1x1kb": (1, 1000), "1x1Mb": (1, 1_000_000), "1000x1kb": (1000, 1000), "100000x100b": (100_000, 100)}
    out["fetch"] = {}
    for name, (n, ln) in shapes.items():
        begins = [rng.randrange(L - ln) for _ in range(n)]
        arr = (sccg.Region * n)(*[(b, b + ln) for b in begins])
        F = n * ln
        d_o = torch.empty(F + 64, dtype=torch.uint8, device=dev)
        got = ctypes.c_size_t()

        def call():
            rc = lib.sccg_reader_fetch_device(rd.ptr, arr, n, 0, d_o.data_ptr(), F, ctypes.byref(got), s)
            assert rc == 0 and got.value == F, (rc, got.value)

        ev, host = timed(call)
        ctx.profile(True, families=["fetch"])
        for _ in range(a.calls):
            call()
        kern = ctx.profile_get().get("fetch", (0.0, 0))
        ctx.profile(False)
        exact = d_o[:F].cpu().numpy().tobytes() == b"".join(truth[b:b + ln] for b in begins)
        out["fetch"][name] = {"bytes": F, "event_ms": spread(ev), "host_ms": spread(host),
                              "kernel_ms_mean": round(kern[0] / max(kern[1], 1), 4),
                              "launches_per_call": kern[1] / a.calls, "exact": exact}
        del d_o
    # ---- encoded fetch beside the two-step path (ASCII fetch, then a PyTorch lookup-table encode on
    # the same stream): index, one-hot f16 / f32 on the forward strand, ASCII with alternating strands
    comp = bytes.maketrans(b"ACGTRYKMBVDHacgtrykmbvdh", b"TGCAYRMKVBHDtgcayrmkvbhd")
    code = [4] * 256
    for k, ch in enumerate(b"ACGT"):
        code[ch] = code[ch + 32] = k
    lut_idx = torch.tensor(code, dtype=torch.uint8, device=dev)
    lut_comp = torch.tensor(list(comp), dtype=torch.uint8, device=dev)
    eye = torch.cat([torch.eye(4, device=dev), torch.zeros(1, 4, device=dev)])
    rows = {"index": ("index", "u8", torch.uint8, 1), "onehot_f16": ("onehot", "f16", torch.float16, 8),
            "onehot_f32": ("onehot", "f32", torch.float32, 16), "ascii_strands": ("ascii", "u8", torch.uint8, 1)}
    out["fetch_encoded"] = {}
    # (a library older than the encoded fetch, SCCG_LIB_PATH in A/B runs, has the rows above only)
    enc_shapes = ("1000x1kb", "100000x100b") if hasattr(lib, "sccg_reader_fetch_encoded_device") else ()
    for name, (n, ln) in {k: shapes[k] for k in enc_shapes}.items():
        begins = [rng.randrange(L - ln) for _ in range(n)]
        arr = (sccg.Region * n)(*[(b, b + ln) for b in begins])
        F = n * ln
        d_a = torch.empty(F + 64, dtype=torch.uint8, device=dev)
        got = ctypes.c_size_t()
        fwd = b"".join(truth[b:b + ln] for b in begins)
        for row, (enc, dt, tdt, bpb) in rows.items():
            strands = bytes(k & 1 for k in range(n)) if row == "ascii_strands" else None
            fmt = sccg.FetchFormat(sccg.ENCODINGS[enc], sccg.DTYPES[dt], 0, 0)
            d_o = torch.empty(F * bpb + 64, dtype=torch.uint8, device=dev)
            table = None if enc == "ascii" else lut_idx if enc == "index" else eye[lut_idx.long()].to(tdt).contiguous()
            two = [None]

            def call():
                rc = lib.sccg_reader_fetch_encoded_device(rd.ptr, arr, n, strands, ctypes.byref(fmt), d_o.data_ptr(), F * bpb,
                                                          ctypes.byref(got), s)
                assert rc == 0 and got.value == F * bpb, (rc, got.value)

            def two_step():
                rc = lib.sccg_reader_fetch_device(rd.ptr, arr, n, 0, d_a.data_ptr(), F, ctypes.byref(got), s)
                assert rc == 0 and got.value == F, (rc, got.value)
                a_ = d_a[:F]
                if enc == "ascii":   # complement everything, then put the reversed rows back to front
                    t = torch.where((torch.arange(n, device=dev) & 1).bool()[:, None], lut_comp[a_.int()].view(n, ln).flip(1),
                                    a_.view(n, ln))
                else:
                    t = table[a_.int()]
                two[0] = t

            ev, host = timed(call)
            ev2, host2 = timed(two_step)
            ctx.profile(True, families=["fetch"])
            for _ in range(a.calls):
                call()
            kern = ctx.profile_get().get("fetch", (0.0, 0))
            ctx.profile(False)
            if enc == "ascii":
                want = b"".join(truth[b:b + ln].translate(comp)[::-1] if k & 1 else truth[b:b + ln] for k, b in enumerate(begins))
            else:
                c = np.array(code, dtype=np.uint8)[np.frombuffer(fwd, dtype=np.uint8)]
                want = c.tobytes() if enc == "index" else np.vstack([np.eye(4), np.zeros((1, 4))]).astype(
                    np.float16 if dt == "f16" else np.float32)[c].tobytes()
            bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[two[0].element_size()]
            exact = d_o[:F * bpb].cpu().numpy().tobytes() == want
            exact2 = two[0].contiguous().view(bits).cpu().numpy().tobytes() == want
            med, med2 = statistics.median(ev), statistics.median(ev2)
            out["fetch_encoded"][f"{name}/{row}"] = {
                "bytes": F * bpb, "event_ms": spread(ev), "host_ms": spread(host),
                "kernel_ms_mean": round(kern[0] / max(kern[1], 1), 4), "launches_per_call": kern[1] / a.calls,
                "out_GBps": round(F * bpb / med / 1e6, 1), "exact": exact,
                "two_step_event_ms": spread(ev2), "two_step_host_ms": spread(host2), "two_step_exact": exact2,
                "two_step_over_encoded": round(med2 / med, 2)}
            del d_o
        del d_a
    if hasattr(lib, "sccg_cohort_fetch_device"):   # (absent from a library older than the cohort fetch)
        out["cohort"] = cohort_section(a, ctx, lib, torch, sccg, dev, stream, rd, d_ref, len(rfa), d_rec, len(rec_h), truth, code)
    if hasattr(lib, "sccg_reader_has_coords"):   # (absent from a library older than the origin fetch)
        out["origin"] = origin_section(a, ctx, lib, torch, sccg, dev, stream, d_ref, len(rfa), d_rec, len(rec_h), truth, rfa, code)
    rd.close()
    ctx.close()
    print(json.dumps(out))
    if "origin" in out and not all(v["exact"] for v in out["origin"]["fetch"].values() if isinstance(v, dict) and "exact" in v):
        raise SystemExit("bench_fetch: origin section: bytes differ from the target FASTA")
    if "cohort" in out and not all(v["exact"] for v in out["cohort"]["fetch"].values()):
        raise SystemExit("bench_fetch: cohort bytes differ from the target FASTA")
    if not all(v["exact"] and v["two_step_exact"] for v in out["fetch_encoded"].values()):
        raise SystemExit("bench_fetch: encoded bytes differ from the target FASTA")
    if not all(v["exact"] for v in out["fetch"].values()):
        raise SystemExit("bench_fetch: fetched bytes differ from the target FASTA")


if __name__ == "__main__":
    main()
