"""The truth of the segments call (sccg_*_segments), never the code under test: a numpy run-length coding
of originlib's per-base origins by the definition in sccg.h, and a second truth that needs no oracle --
the segments expanded back to per-base origins are what the GPU's own origin fetch of the same regions
returns, and a base copied from reference position r is the reference's base at r.  Every check also
asserts the shape of an answer: the segments tile each region and no two neighbours could merge."""
import random

import numpy as np

import originlib
from locatelib import record


def rle(org: np.ndarray, b: int, e: int) -> np.ndarray:
    """The segments of [b, e) as rows (pos, len, ref): maximal runs of origins ascending by one, of -1, of -2."""
    s = org[b:e].astype(np.int64)
    if s.size == 0:
        return np.zeros((0, 3), dtype=np.int64)
    goes_on = np.where(s[:-1] >= 0, s[1:] == s[:-1] + 1, s[1:] == s[:-1])
    starts = np.concatenate(([0], np.nonzero(~goes_on)[0] + 1))
    lens = np.diff(np.append(starts, s.size))
    return np.stack([starts + b, lens, s[starts]], axis=1).astype(np.int64)


def want(org_of, items):
    """(off, seg) of a batch: items (begin, end) with org_of one array, or (sample, begin, end) with a list."""
    parts, off = [np.zeros((0, 3), dtype=np.int64)], [0]
    for it in items:
        org, b, e = (org_of, it[0], it[1]) if len(it) == 2 else (org_of[it[0]], it[1], it[2])
        parts.append(rle(org, int(b), int(e)))
        off.append(off[-1] + len(parts[-1]))
    return np.array(off, dtype=np.int64), np.concatenate(parts)


def expand(seg: np.ndarray) -> np.ndarray:
    """The per-base origins that segment rows spell, concatenated."""
    if len(seg) == 0:
        return np.zeros(0, dtype=np.int64)
    ln = seg[:, 1]
    ref = np.repeat(seg[:, 2], ln)
    k = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
    return np.where(ref >= 0, ref + k, ref)


def check_shape(off, seg, bounds, what=""):
    """Layout, tiling and maximality: bounds = the (begin, end) of every region in list order."""
    assert off.dtype == np.int64 and seg.dtype == np.int64 and seg.ndim == 2 and seg.shape[1] == 3, what
    assert off.shape == (len(bounds) + 1,) and off[0] == 0 and off[-1] == len(seg), f"{what}: offsets {off[:4]}.. for {len(seg)} segments"
    assert np.all(np.diff(off) >= 0), what
    assert np.all(seg[:, 1] > 0) and np.all(seg[:, 2] >= -2), f"{what}: a segment without bases or with a ref below -2"
    for i, (b, e) in enumerate(bounds):
        g = seg[off[i]:off[i + 1]]
        if e <= b:
            assert len(g) == 0, f"{what}: empty region {i} has segments"
            continue
        assert len(g) > 0 and g[0, 0] == b and g[-1, 0] + g[-1, 1] == e, f"{what}: region {i} [{b}, {e}) is not covered: {g[:3].tolist()}"
        assert np.all(g[1:, 0] == g[:-1, 0] + g[:-1, 1]), f"{what}: region {i} [{b}, {e}) is not tiled"
        a, c = g[:-1], g[1:]
        merge = np.where(a[:, 2] >= 0, c[:, 2] == a[:, 2] + a[:, 1], c[:, 2] == a[:, 2])
        assert not merge.any(), f"{what}: region {i}: segments {int(np.nonzero(merge)[0][0])} and the next could merge: {g.tolist()[:6]}"


def check_oracle(got, exp, items, what=""):
    (goff, gseg), (eoff, eseg) = got, exp
    bad = np.nonzero(goff != eoff)[0]
    if bad.size == 0 and gseg.shape == eseg.shape and np.array_equal(gseg, eseg):
        return
    i = int(bad[0]) - 1 if bad.size else next(k for k in range(len(items)) if not np.array_equal(gseg[goff[k]:goff[k + 1]], eseg[eoff[k]:eoff[k + 1]]))
    i = max(i, 0)
    raise AssertionError(f"{what}: region {i} {tuple(items[i])}: got {gseg[goff[i]:goff[i + 1]][:8].tolist()}, "
                         f"want {eseg[eoff[i]:eoff[i + 1]][:8].tolist()} ({len(gseg)} segments, want {len(eseg)})")


def check(rd, org, regions, R=None, seq=None, what=""):
    """One reader call against both truths; returns (off, seg)."""
    regions = [(int(b), int(e)) for b, e in regions]
    got = rd.segments(regions)
    check_shape(got[0], got[1], regions, what)
    check_oracle(got, want(org, regions), regions, what)
    if regions and got[1].size:
        gpu = originlib.fetch(rd, regions)   # the GPU's own origin fetch of the same regions
        assert np.array_equal(expand(got[1]), gpu.astype(np.int64)), f"{what}: the segments do not expand to the origin fetch"
        if R is not None:
            originlib.check_independent(R, seq, gpu, originlib.positions_of(regions), what)
    return got


def check_cohort(co, orgs, items, R=None, seqs=None, what=""):
    items = [(int(s), int(b), int(e)) for s, b, e in items]
    got = co.segments(items)
    check_shape(got[0], got[1], [(b, e) for _, b, e in items], what)
    check_oracle(got, want(orgs, items), items, what)
    if items and got[1].size:
        gpu = np.frombuffer(co.fetch_encoded(items, "origin", "i32"), dtype="<i4")
        assert np.array_equal(expand(got[1]), gpu.astype(np.int64)), f"{what}: the segments do not expand to the origin fetch"
        if R is not None:
            at = 0
            for s, b, e in items:
                originlib.check_independent(R, seqs[s], gpu[at:at + e - b], np.arange(b, e, dtype=np.int64), f"{what} sample {s}")
                at += e - b
    return got


def every_pair(L):
    return [(b, e) for b in range(L + 1) for e in range(b, L + 1)]


def random_regions(L, n, hi, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        ln = rng.randint(0, min(hi, L))
        b = rng.randrange(L - ln + 1)
        out.append((b, b + ln))
    return out


def token_record(nR, k, seed, zero_every=0):
    """test_gpu_locate.token_record, restated: k tokens of nonzero length at seeded places of a reference
    of nR bases, literals between some, zero-length tokens mixed in."""
    rng = random.Random(seed)
    items = []
    for i in range(k):
        l = rng.randint(1, 40)
        items.append((rng.randrange(nR - l + 1), l))
        if i % 5 == 0:
            items.append(bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 3))))
        if zero_every and i % zero_every == 0:
            items.append((rng.randrange(nR), 0))
    return record(items)


def cli_lines(name: str, org, regions1):
    """`fetch --origin`'s output for 1-based inclusive regions, from the oracle's segments."""
    out = []
    for b1, e1 in regions1:
        out.append(">%s:%d-%d" % (name, b1, e1))
        for pos, ln, ref in rle(org, b1 - 1, e1).tolist():
            tail = "%d\t%d" % (ref + 1, ref + ln) if ref >= 0 else "*" if ref == -1 else "N"
            out.append("%d\t%d\t%s" % (pos + 1, pos + ln, tail))
    return out
