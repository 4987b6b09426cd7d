"""The truth of find with mismatches (where an IUPAC pattern occurs within K substitutions in regions of a
sequence, on either strand), from the sequence's bytes alone -- never the code under test: a numpy-vectorised
per-start mismatch count from a 256-entry byte-to-code table and the pattern's masks, and a second, naive
double loop the first is checked against.  Code 4 -- every byte that is not A, C, G or T in either case -- is a
mismatch against every letter, N included.  The reverse strand is searched with the reverse-complemented
pattern; a hit is reported at the leftmost forward position of its window."""
import functools

import numpy as np

import findlib
from findlib import STRANDS, every_pair, masks, random_pattern, random_sequence, revcomp_pattern, text  # noqa: F401

CODE = np.full(256, 4, dtype=np.uint8)
for _k, _c in enumerate("ACGT"):
    CODE[ord(_c)] = CODE[ord(_c.lower())] = _k
# MISS[mask, code]: 1 where the letter's mask lacks the code's bit; code 4 always
MISS = np.array([[0 if c < 4 and (mk >> c) & 1 else 1 for c in range(5)] for mk in range(16)], dtype=np.int64)


def distances(seq: bytes, pattern, begin: int, end: int):
    """d[j - begin] for every candidate start j of [begin, end): the letters of `pattern` (forward masks) that
    seq[j, j + m) does not satisfy.  Empty when the region is shorter than the pattern."""
    mk = np.frombuffer(masks(pattern), dtype=np.uint8)
    m, n = len(mk), end - begin - len(mk) + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    codes = CODE[np.frombuffer(seq, dtype=np.uint8)[begin:end]]
    d = np.zeros(n, dtype=np.int64)
    for t in range(m):
        d += MISS[mk[t], codes[t:t + n]]
    return d


def distances_naive(seq: bytes, pattern, begin: int, end: int):
    sets = [set((findlib.IUPAC[c] + findlib.IUPAC[c].lower()).encode()) for c in text(pattern).upper()]
    m = len(sets)
    out = []
    for j in range(begin, end - m + 1):
        d = 0
        for t in range(m):
            if seq[j + t] not in sets[t]:
                d += 1
        out.append(d)
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=64)
def _all_hits(seq: bytes, pattern: str, K: int, strands: str):
    """Every (pos, strand, d) with d <= K of the whole sequence, sorted, as an int64 [h, 3]: d(j, s) does not depend
    on the region, which only selects begin <= pos <= end - m."""
    pats = {0: pattern, 1: revcomp_pattern(pattern)}
    parts = []
    for s in STRANDS[strands]:
        d = distances(seq, pats[s], 0, len(seq))
        j = np.nonzero(d <= K)[0]
        parts.append(np.stack([j, np.full(len(j), s, dtype=np.int64), d[j]], axis=1).reshape(-1, 3))
    H = np.concatenate(parts).astype(np.int64)
    return H[np.lexsort((H[:, 1], H[:, 0]))]


def want(seqs, pattern, regions, K, strands="both", distances=None):
    """(off int64 [n + 1], rows int64 [h, 3]).  seqs: one sequence and regions (begin, end), or a list of them
    and items (sample, begin, end).  distances: None -- the vectorised count, once per sequence, the regions
    selecting from it; or a function (seq, pattern, begin, end) called per region and strand, as distances_naive."""
    m = len(text(pattern))
    regions = list(regions)
    one = isinstance(seqs, (bytes, bytearray))
    if distances is None:
        reg = np.array([(0,) + tuple(r) if one else tuple(r[:3]) for r in regions], dtype=np.int64).reshape(-1, 3)
        lo, hi, tables, base = np.zeros(len(reg), dtype=np.int64), np.zeros(len(reg), dtype=np.int64), [], 0
        for s in sorted(set(reg[:, 0].tolist())):   # the rows of sample s lie at [base, base + len(H)) of the table
            H = _all_hits(bytes(seqs if one else seqs[s]), text(pattern), K, strands)
            mine = reg[:, 0] == s
            lo[mine] = base + np.searchsorted(H[:, 0], reg[mine, 1], "left")
            hi[mine] = base + np.searchsorted(H[:, 0], reg[mine, 2] - m, "right")
            tables.append(H)
            base += len(H)
        cnt = np.maximum(hi - lo, 0)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        table = np.concatenate(tables) if tables else np.zeros((0, 3), dtype=np.int64)
        return off, table[np.repeat(lo - off[:-1], cnt) + np.arange(off[-1])].reshape(-1, 3)
    off, rows = [0], []
    for r in regions:
        seq, (b, e) = (seqs, r) if one else (seqs[r[0]], r[1:3])
        found = []
        for s in STRANDS[strands]:
            d = distances(seq, text(pattern) if s == 0 else revcomp_pattern(pattern), b, e)
            found += [(b + int(j), s, int(d[j])) for j in np.nonzero(d <= K)[0]]
        rows += sorted(found)
        off.append(len(rows))
    return np.array(off, dtype=np.int64), np.array(rows, dtype=np.int64).reshape(-1, 3)


def check(got, expected, regions, what=""):
    (goff, ghit), (woff, whit) = got, expected
    assert goff.dtype == np.int64 and ghit.dtype == np.int64 and ghit.ndim == 2 and ghit.shape[1] == 3, what
    assert goff.shape == woff.shape, f"{what}: {goff.shape[0]} offsets, want {woff.shape[0]}"
    if np.array_equal(goff, woff) and np.array_equal(ghit, whit):
        return got
    for i in range(len(woff) - 1):
        g = [tuple(r) for r in ghit[goff[i]:goff[i + 1]].tolist()]
        w = [tuple(r) for r in whit[woff[i]:woff[i + 1]].tolist()]
        assert goff[i] == woff[i] and g == w, (f"{what}: region {i} {tuple(regions[i])}: off {int(goff[i])} want {int(woff[i])}; "
                                              f"hits {g[:6]}... ({len(g)}) want {w[:6]}... ({len(w)})")
    raise AssertionError(f"{what}: total {int(goff[-1])} ({len(ghit)} rows), want {int(woff[-1])}")


def check_reader(rd, seq, pattern, regions, K, strands="both", what=""):
    regions = list(regions)
    return check(rd.find_approx(pattern, regions, K, strands), want(seq, pattern, regions, K, strands), regions,
                 f"{what} {text(pattern)} K={K} {strands}")


def check_cohort(co, seqs, pattern, items, K, strands="both", what=""):
    items = list(items)
    return check(co.find_approx(pattern, items, K, strands), want(seqs, pattern, items, K, strands), items,
                 f"{what} {text(pattern)} K={K} {strands}")


def check_independent(fetch_index, pattern, hits, K, what=""):
    """Every reported row's mismatches recomputed on the GPU's own bases: fetch_index(regions) returns the
    SCCG_ENC_INDEX codes of the windows [pos, pos + m) on the FORWARD strand; a row of strand 1 is held against
    the reverse-complemented pattern's masks.  Equal to the reported number, and <= K."""
    mks = {0: np.frombuffer(masks(pattern), dtype=np.uint8), 1: np.frombuffer(masks(revcomp_pattern(pattern)), dtype=np.uint8)}
    m = len(mks[0])
    hits = np.asarray(hits).reshape(-1, 3)
    if not len(hits):
        return
    codes = np.frombuffer(fetch_index([(int(p), int(p) + m) for p in hits[:, 0]]), dtype=np.uint8).reshape(-1, m)
    assert (codes <= 4).all(), what
    mk = np.stack([mks[int(s)] for s in hits[:, 1]])
    d = MISS[mk, codes].sum(axis=1)
    bad = np.nonzero(d != hits[:, 2])[0]
    assert bad.size == 0, f"{what}: row {int(bad[0])} {hits[bad[0]].tolist()} has {int(d[bad[0]])} mismatches on the fetched bases"
    assert (hits[:, 2] <= K).all() and (hits[:, 2] >= 0).all(), f"{what}: a row beyond K = {K}"
