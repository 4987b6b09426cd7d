"""Helpers of the shared-reference and cohort tests: the truth of the hand-written records derived in
Python from the record format alone, five targets made from one reference body by seeded edits, and
the truth of a cohort fetch built from the targets' bodies (never from the code under test)."""
import random
import re

import numpy as np

import fetchlib
import synthlib
from fetchlib import BPB, encode, revcomp, split_fasta

ALL_FORMATS = [("ascii", "u8"), ("index", "u8"), ("onehot", "u8"), ("onehot", "f16"), ("onehot", "bf16"), ("onehot", "f32")]
RFA, RFA_N, HAND = fetchlib.RFA, fetchlib.RFA_N, fetchlib.HAND
R_BODY = b"ACGT" * 50                 # RFA holds no N: both forms of R' are its body
KEPT_N = b"ACGTNNNNACGT" * 10         # RFA_N with its N kept: 120 bases
ERASED_N = b"ACGTACGT" * 10           # RFA_N with its N erased: 80 bases

# A record over RFA_N with an N-run line: its tokens index the 80-base erased form.
ERASED_REC = b"\n(4,4)(30,2)\n(0,30)AC(40,10)"
ERASED_SEQ = b"ACGTNNNNACGTACGTACGTACGTACGTACGTACNNACACGTACGTAC"
# (70,40) ends at 110: inside the 120-base kept form, beyond the 80-base erased one
ERASED_REC_BEYOND = b"\n(4,4)\n(70,40)"
# what three of fetchlib.HAND's records spell, written out by hand
HAND_SEQ = {
    "literals_only": b"ACGTTGCAAC",
    "token_first_and_last": b"ACGTACGTAC" + b"TTT" + b"ACGTACGTACGT",
    "n_line_is_comma": b"ACGTNNNNACGTACGTNNNNACGTACGTNN" + b"AC" + b"GT" + b"ACGTNNNNACGT" + b"ACGTNN",
}


def _runs(line: bytes):
    """A run line's (start, len) items (decompression.cpp:126-207): each start is the previous start
    plus the item's first number; a bare number is a run of one."""
    out, at = [], 0
    for m in re.finditer(rb"\((-?\d+),(\d+)\)|(-?\d+)", line):
        at += int(m.group(1) if m.group(1) is not None else m.group(3))
        out.append((at, int(m.group(2)) if m.group(2) is not None else 1))
    return out


def hand_sequence(rfa: bytes, rec: bytes) -> bytes:
    """The sequence a record spells, from the record format (decompression.cpp:105-262): R' by the N
    line, the record line's tokens (running start, length) and literals, N runs inserted in ascending
    order, the lowercase runs applied last."""
    lines = rec.split(b"\n")
    if lines[0].startswith(b">"):
        lines = lines[1:]
    lower, nline, enc = lines[0], lines[1], lines[2]
    body = split_fasta(rfa)[1]
    rp = (body if nline == b"," else body.replace(b"N", b"")).upper()
    out, p, i = bytearray(), 0, 0
    while i < len(enc):
        m = re.compile(rb"\((-?\d+),(\d+)\)").match(enc, i)
        if m:
            p += int(m.group(1))
            out += rp[p:p + int(m.group(2))]
            i = m.end()
        else:
            out.append(enc[i])   # (a ')' outside a token is a literal too)
            i += 1
    if nline != b",":
        for s, l in _runs(nline):
            out[s:s] = b"N" * l
    for s, l in _runs(lower):
        out[s:s + l] = bytes(out[s:s + l]).lower()
    return bytes(out)


# ---------------------------------------------------------------------------------------------
# five targets over one reference
# ---------------------------------------------------------------------------------------------
REF_LEN = 60_000
KINDS = ["snp", "indel", "nruns", "lowercase", "block"]


def wrap60(name: bytes, body: bytes) -> bytes:
    return b">" + name + b"\n" + b"".join(body[k:k + 60] + b"\n" for k in range(0, len(body), 60))


def _snps(a: bytearray, rng, rate):
    for k in range(len(a)):
        if a[k] in b"ACGTacgt" and rng.random() < rate:
            up = bytes([a[k]]).upper()
            c = rng.choice([x for x in b"ACGT" if x != up[0]])
            a[k] = c | (a[k] & 0x20)


def _random_block(a: bytearray, rng, at, n):
    a[at:at + n] = bytes(rng.choice(b"ACGT") for _ in range(n))


def make_target(ref_body: bytes, kind: str, seed: int) -> bytes:
    """A target body: the reference body under the seeded edits of `kind`."""
    rng = random.Random(seed)
    a = bytearray(ref_body)
    _snps(a, rng, 1e-3)
    if kind == "indel":
        k = 4000
        while k < len(a) - 4000:
            n = rng.randint(1, 12)
            if rng.random() < 0.5:
                del a[k:k + n]
            else:
                a[k:k] = bytes(rng.choice(b"ACGT") for _ in range(n))
            k += rng.randint(500, 3000)
    elif kind == "nruns":
        # leaves local mode, so its N are runs of the N line: the reference's own terminal gaps cut
        # short, a run at the very start and end, runs one base apart, and runs inside the block
        _random_block(a, rng, 20_000, 10_000)
        del a[5:2900]
        del a[len(a) - 2950:len(a) - 7]
        for at, n in ((10_000, 3), (10_004, 5), (10_010, 1), (10_012, 1), (25_000, 70), (25_071, 2), (40_000, 1100)):
            a[at:at + n] = b"N" * n
    elif kind == "lowercase":
        k = 3000
        while k < len(a) - 3000:
            n = rng.randint(1, 20)
            a[k:k + n] = bytes(a[k:k + n]).swapcase()
            k += n + rng.randint(1, 40)
    elif kind == "block":
        _random_block(a, rng, 30_000, 10_000)
    elif kind != "snp":
        raise ValueError(kind)
    return bytes(a)


def make_cohort_inputs(seed: int = 5):
    """(reference FASTA, {kind: (target FASTA, target body)})."""
    rfa, _ = synthlib.synth_pair("hg", REF_LEN, REF_LEN, seed)
    body = split_fasta(rfa)[1]
    assert len(body) == REF_LEN
    out = {}
    for i, kind in enumerate(KINDS):
        tb = make_target(body, kind, 100 + i)
        out[kind] = (wrap60(b"s" + str(i).encode() + b" " + kind.encode(), tb), tb)
    return rfa, out


def n_line(rec: bytes) -> bytes:
    lines = rec.split(b"\n")
    if lines[0].startswith(b">"):
        lines = lines[1:]
    return lines[1]


def sample_boundaries(truth: bytes, rec: bytes, cap: int = 60, seed: int = 11):
    """fetchlib.Pair.boundaries for one sample: N / non-N and case transitions of its truth, token
    starts and ends in sequence coordinates; each kind capped, seeded."""
    a = np.frombuffer(truth, dtype=np.uint8)
    L = len(truth)
    runs, toks, D = fetchlib.parse_record(rec)
    keep = np.ones(L, dtype=bool)
    for s, l in runs:
        keep[s:s + l] = False
    d2j = np.append(np.nonzero(keep)[0], L)
    assert len(d2j) == D + 1, "the test's record parse disagrees with the target"
    is_n = (a | 0x20) == ord("n")
    low = (a >= ord("a")) & (a <= ord("z"))
    kinds = {"n": np.nonzero(is_n[1:] != is_n[:-1])[0] + 1, "case": np.nonzero(low[1:] != low[:-1])[0] + 1,
             "tok_start": d2j[[o for o, _ in toks]], "tok_end": d2j[[o + l for o, l in toks]]}
    rng = random.Random(seed)
    return {k: sorted(rng.sample([int(x) for x in v], min(cap, len(v)))) for k, v in kinds.items()}


# ---------------------------------------------------------------------------------------------
# the truth of a cohort fetch
# ---------------------------------------------------------------------------------------------
def want_items(truths, items, encoding, dtype="u8", revcomp_all=False, upper=False) -> bytes:
    """items: (sample, begin, end[, reverse]) over truths[sample]."""
    parts = []
    for it in items:
        s = truths[it[0]][it[1]:it[2]]
        if upper:
            s = s.upper()
        parts.append(revcomp(s) if revcomp_all or (len(it) > 3 and it[3]) else s)
    return encode(b"".join(parts), encoding, dtype)


def check_items(co, truths, items, encoding="index", dtype="u8", revcomp_all=False, upper=False, what=""):
    """One cohort fetch of `items` against the truths' slices; names the first item that differs."""
    items = list(items)
    got = co.fetch_encoded(items, encoding=encoding, dtype=dtype, revcomp=revcomp_all, upper=upper)
    want = want_items(truths, items, encoding, dtype, revcomp_all, upper)
    if got == want:
        return
    bpb = BPB[(encoding, dtype)]
    assert len(got) == len(want), f"{what}: {len(got)} bytes, want {len(want)}"
    at = next(i for i in range(len(got)) if got[i] != want[i]) // bpb
    k, acc = 0, 0
    while acc + (items[k][2] - items[k][1]) <= at:
        acc += items[k][2] - items[k][1]
        k += 1
    raise AssertionError(f"{what} {encoding}/{dtype}: item {k} {items[k]} differs at base +{at - acc} (flat base {at}): "
                         f"got {got[at * bpb:at * bpb + 2 * bpb].hex()}, want {want[at * bpb:at * bpb + 2 * bpb].hex()}")
