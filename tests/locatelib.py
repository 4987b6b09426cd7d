"""The truth of locate (reference position -> sequence position): originlib's per-base origins, inverted
with numpy -- never the code under test -- and a second truth that needs no inverse at all (the origin
fetch of a located position returns the reference position, and its base is the reference's)."""
import random

import numpy as np

import cohortlib
import originlib

NONE, REF_N = -1, -2


def inverse(rfa: bytes, rec: bytes):
    """(pos int64 [|R|], copies int32 [|R|]): per reference position the first sequence position whose
    origin it is and how many have it; NONE without one; REF_N on an uppercase N of a reference whose
    record indexes the erased form."""
    _, org = originlib.origins(rfa, rec)
    R = originlib.ref_sequence(rfa)
    pos = np.full(len(R), NONE, dtype=np.int64)
    at = np.nonzero(org >= 0)[0]
    vals, first = np.unique(org[at], return_index=True)   # (first occurrence of each value: at ascends)
    pos[vals] = at[first]
    copies = np.bincount(org[at], minlength=len(R)).astype(np.int32)
    if cohortlib.n_line(rec) != b",":
        is_n = np.frombuffer(R, dtype=np.uint8) == ord("N")
        assert not copies[is_n].any()
        pos[is_n] = REF_N
    return pos, copies


def check(got, want, q, what=""):
    (gp, gc), (wp, wc) = got, want
    q = np.asarray(q, dtype=np.int64).reshape(-1)
    assert gp.dtype == np.int64 and gc.dtype == np.int32 and gp.shape == gc.shape == q.shape, what
    bad = np.nonzero((gp != wp[q]) | (gc != wc[q]))[0]
    assert bad.size == 0, (f"{what}: query {int(bad[0])} (reference position {int(q[bad[0]])}): got pos {int(gp[bad[0]])} copies "
                           f"{int(gc[bad[0]])}, want pos {int(wp[q[bad[0]]])} copies {int(wc[q[bad[0]]])} ({bad.size} differ)")


def check_independent(rd, rfa: bytes, q, pos, what=""):
    """For every pos >= 0: the GPU's origin fetch of [pos, pos + 1) is the reference position asked for,
    and the base there, uppercased, is the reference's."""
    q, pos = np.asarray(q, dtype=np.int64).reshape(-1), np.asarray(pos)
    hit = pos >= 0
    regions = [(int(p), int(p) + 1) for p in pos[hit]]
    if not regions:
        return
    assert np.array_equal(originlib.fetch(rd, regions), q[hit].astype(np.int32)), f"{what}: origin(pos) is not the position asked"
    R = np.frombuffer(originlib.ref_sequence(rfa).upper(), dtype=np.uint8)
    bases = np.frombuffer(rd.fetch_encoded(regions, "ascii").upper(), dtype=np.uint8)
    assert np.array_equal(bases, R[q[hit]]), f"{what}: the base at pos is not the reference's"


def random_body(n: int, seed: int) -> bytes:
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def fasta(body: bytes, name: bytes = b"r") -> bytes:
    return b">" + name + b"\n" + b"".join(body[k:k + 60] + b"\n" for k in range(0, len(body), 60))


def record(items, lower: bytes = b"", nline: bytes = b"") -> bytes:
    """A record from absolute (p, l) tokens and literal bytes, in record order."""
    out, prev = b"", 0
    for it in items:
        if isinstance(it, bytes):
            out += it
        else:
            out += b"(%d,%d)" % (it[0] - prev, it[1])
            prev = it[0]
    return lower + b"\n" + nline + b"\n" + out
