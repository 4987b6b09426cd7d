"""The truth of find (where an IUPAC pattern occurs in regions of a sequence, on either strand), from the
sequence's bytes alone -- never the code under test: a regex with a lookahead built from the IUPAC classes,
and a second, naive per-base double loop the first is checked against.  The reverse strand is searched with
the reverse-complemented pattern; a hit is reported at the leftmost forward position of its window."""
import functools
import random
import re

import numpy as np

IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K",
              "B": "V", "V": "B", "D": "H", "H": "D", "N": "N"}
BIT = {"A": 1, "C": 2, "G": 4, "T": 8}
STRANDS = {"+": (0,), "-": (1,), "both": (0, 1)}


def text(pattern) -> str:
    return pattern.decode("latin-1") if isinstance(pattern, (bytes, bytearray)) else pattern


def revcomp_pattern(pattern) -> str:
    return "".join(COMPLEMENT[c] for c in reversed(text(pattern).upper()))


def masks(pattern) -> bytes:
    return bytes(sum(BIT[b] for b in IUPAC[c]) for c in text(pattern).upper())


@functools.lru_cache(maxsize=None)
def _regex(pattern):
    body = "".join("[" + IUPAC[c] + IUPAC[c].lower() + "]" for c in text(pattern).upper())
    return re.compile(("(?=" + body + ")").encode())


def starts_regex(seq: bytes, pattern, begin: int, end: int):
    """Forward hits of [begin, end): the slice ends the text, so no window crosses `end`."""
    return [begin + m.start() for m in _regex(pattern).finditer(seq[begin:end])]


def starts_naive(seq: bytes, pattern, begin: int, end: int):
    sets = [set((IUPAC[c] + IUPAC[c].lower()).encode()) for c in text(pattern).upper()]
    m = len(sets)
    out = []
    for j in range(begin, end - m + 1):
        ok = True
        for t in range(m):
            if seq[j + t] not in sets[t]:
                ok = False
                break
        if ok:
            out.append(j)
    return out


def want(seqs, pattern, regions, strands="both", starts=starts_regex):
    """(off int64 [n + 1], hits int64 [h, 2]).  seqs: one sequence and regions (begin, end), or a list of them
    and items (sample, begin, end)."""
    pats = {0: text(pattern), 1: revcomp_pattern(pattern)}
    off, rows = [0], []
    for r in regions:
        seq, (b, e) = (seqs, r) if isinstance(seqs, (bytes, bytearray)) else (seqs[r[0]], r[1:3])
        found = []
        for s in STRANDS[strands]:
            found += [(j, s) for j in starts(seq, pats[s], b, e)]
        rows += sorted(found)
        off.append(len(rows))
    return np.array(off, dtype=np.int64), np.array(rows, dtype=np.int64).reshape(-1, 2)


def check(got, expected, regions, what=""):
    (goff, ghit), (woff, whit) = got, expected
    assert goff.dtype == np.int64 and ghit.dtype == np.int64 and ghit.ndim == 2 and ghit.shape[1] == 2, what
    assert goff.shape == woff.shape, f"{what}: {goff.shape[0]} offsets, want {woff.shape[0]}"
    if np.array_equal(goff, woff) and np.array_equal(ghit, whit):
        return got
    for i in range(len(woff) - 1):
        g = [tuple(r) for r in ghit[goff[i]:goff[i + 1]].tolist()]
        w = [tuple(r) for r in whit[woff[i]:woff[i + 1]].tolist()]
        assert goff[i] == woff[i] and g == w, (f"{what}: region {i} {tuple(regions[i])}: off {int(goff[i])} want {int(woff[i])}; "
                                              f"hits {g[:6]}... ({len(g)}) want {w[:6]}... ({len(w)})")
    raise AssertionError(f"{what}: total {int(goff[-1])} ({len(ghit)} rows), want {int(woff[-1])}")


def check_cohort(co, seqs, pattern, items, strands="both", what=""):
    items = list(items)
    return check(co.find(pattern, items, strands), want(seqs, pattern, items, strands), items, f"{what} {text(pattern)} {strands}")


def check_independent(fetch_index, pattern, hits, what=""):
    """Every reported hit satisfies the masks on the GPU's own bases: fetch_index(regions, strand) returns the
    SCCG_ENC_INDEX codes of the windows [pos, pos + m), each on the strand of its hit."""
    mk = np.frombuffer(masks(pattern), dtype=np.uint8)
    m = len(mk)
    hits = np.asarray(hits).reshape(-1, 2)
    if not len(hits):
        return
    codes = np.frombuffer(fetch_index([(int(p), int(p) + m) for p in hits[:, 0]], [int(s) for s in hits[:, 1]]), dtype=np.uint8)
    codes = codes.reshape(-1, m)
    assert (codes < 4).all(), f"{what}: a hit window holds a base that is not A, C, G or T"
    ok = (mk[None, :] >> codes) & 1
    bad = np.nonzero(~ok.all(axis=1))[0]
    assert bad.size == 0, f"{what}: hit {int(bad[0])} {hits[bad[0]].tolist()} does not satisfy the pattern's masks"


def every_pair(L: int):
    return [(b, e) for b in range(L + 1) for e in range(b, L + 1)]


def random_sequence(n: int, seed: int, alphabet: bytes = b"ACGT") -> bytes:
    rng = random.Random(seed)
    return bytes(rng.choice(alphabet) for _ in range(n))


def random_pattern(rng, m: int, letters: str = "ACGTRYSWKMBDHVN") -> str:
    return "".join(rng.choice(letters) for _ in range(m))
