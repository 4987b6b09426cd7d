"""The truth of the origin fetch (SCCG_ENC_ORIGIN), derived in plain Python from the record format and
the reference FASTA alone -- never from the code under test: cohortlib.hand_sequence with every base's
origin carried beside it, and a second truth that needs no oracle at all (a base copied from reference
position r IS the reference's base at r)."""
import re

import numpy as np

LITERAL, NRUN = -1, -2


def ref_sequence(rfa: bytes) -> bytes:
    """R: the reference file's lines that are neither empty nor headers, joined, whitespace removed
    (decompression.cpp:53-58), in its original case."""
    body = b"".join(ln for ln in rfa.split(b"\n") if ln and not ln.startswith(b">"))
    return bytes(c for c in body if c not in b" \t\n\v\f\r")


def _runs(line: bytes):
    out, at = [], 0
    for m in re.finditer(rb"\((-?\d+),(\d+)\)|(-?\d+)", line):
        at += int(m.group(1) if m.group(1) is not None else m.group(3))
        out.append((at, int(m.group(2)) if m.group(2) is not None else 1))
    return out


def rprime_to_r(R: bytes, nline: bytes) -> list[int]:
    """The R position of every R' position: with an N-run line only the byte 'N' is erased (a
    lowercase 'n' stays, decompression.cpp:108 before :110); with the N line "," nothing is."""
    table = []
    for k in range(len(R)):
        if nline != b"," and R[k] == ord("N"):
            continue
        table.append(k)
    return table


def origins(rfa: bytes, rec: bytes):
    """(sequence, int32 array): what the record spells and, per base, where it comes from -- the
    reference position a token copied it from, LITERAL, or NRUN."""
    lines = rec.split(b"\n")
    if lines[0].startswith(b">"):
        lines = lines[1:]
    lower, nline, enc = lines[0], lines[1], lines[2]
    R = ref_sequence(rfa)
    table = rprime_to_r(R, nline)
    rp = bytes(R[k] for k in table).upper()
    seq, org, p, i = bytearray(), [], 0, 0
    tok = re.compile(rb"\((-?\d+),(\d+)\)")
    while i < len(enc):
        m = tok.match(enc, i)
        if m:
            p += int(m.group(1))
            n = int(m.group(2))
            assert 0 <= p and p + n <= len(rp), "the test's record reaches beyond R'"
            seq += rp[p:p + n]
            org += table[p:p + n]
            i = m.end()
        else:
            seq.append(enc[i])
            org.append(LITERAL)
            i += 1
    if nline != b",":
        for s, l in _runs(nline):
            seq[s:s] = b"N" * l
            org[s:s] = [NRUN] * l
    for s, l in _runs(lower):
        seq[s:s + l] = bytes(seq[s:s + l]).lower()
    return bytes(seq), np.array(org, dtype=np.int32).reshape(-1)


def want(org: np.ndarray, regions, strands=None, revcomp_all=False) -> np.ndarray:
    """The flat int32 result of a batched fetch: a reversed region's values in reverse order, unchanged."""
    parts = [np.zeros(0, dtype=np.int32)]
    for k, (b, e) in enumerate(regions):
        s = org[b:e]
        parts.append(s[::-1] if revcomp_all or (strands is not None and strands[k]) else s)
    return np.concatenate(parts)


def check_independent(R: bytes, target: bytes, got: np.ndarray, positions: np.ndarray, what=""):
    """The truth that needs no oracle: got[k] is the origin of sequence position positions[k].  A value
    r >= 0 names the reference base the target's base is; -2 sits on an N of the target; nothing else
    than -1, -2 and a position inside R appears."""
    Ru = np.frombuffer(R.upper(), dtype=np.uint8)
    Tu = np.frombuffer(target.upper(), dtype=np.uint8)[positions]
    assert got.shape == positions.shape, f"{what}: {got.shape} values for {positions.shape} positions"
    assert int(got.min(initial=0)) >= NRUN and int(got.max(initial=0)) < len(Ru), f"{what}: a value outside [-2, |R|)"
    cop = got >= 0
    bad = np.nonzero(Ru[got[cop]] != Tu[cop])[0]
    assert bad.size == 0, (f"{what}: position {int(positions[cop][bad[0]])} is {chr(Tu[cop][bad[0]])} but its origin "
                           f"{int(got[cop][bad[0]])} holds {chr(Ru[got[cop][bad[0]]])}")
    nr = got == NRUN
    assert np.all(Tu[nr] == ord("N")), f"{what}: -2 on a base that is not N"


def positions_of(regions, strands=None, revcomp_all=False) -> np.ndarray:
    parts = [np.zeros(0, dtype=np.int64)]
    for k, (b, e) in enumerate(regions):
        a = np.arange(b, e, dtype=np.int64)
        parts.append(a[::-1] if revcomp_all or (strands is not None and strands[k]) else a)
    return np.concatenate(parts)


def fetch(rd, regions, strands=None, revcomp_all=False) -> np.ndarray:
    raw = rd.fetch_encoded(list(regions), "origin", "i32", strand=strands, revcomp=revcomp_all)
    return np.frombuffer(raw, dtype="<i4")


def check(rd, org: np.ndarray, regions, strands=None, revcomp_all=False, what=""):
    regions = list(regions)
    got = fetch(rd, regions, strands, revcomp_all)
    exp = want(org, regions, strands, revcomp_all)
    assert got.shape == exp.shape, f"{what}: {got.size} values, want {exp.size}"
    bad = np.nonzero(got != exp)[0]
    if bad.size:
        at, k, acc = int(bad[0]), 0, 0
        while acc + (regions[k][1] - regions[k][0]) <= at:
            acc += regions[k][1] - regions[k][0]
            k += 1
        raise AssertionError(f"{what}: region {k} {regions[k]} differs at base +{at - acc} (flat {at}): got "
                             f"{got[at:at + 8].tolist()}, want {exp[at:at + 8].tolist()} ({bad.size} differ)")
    return got
