"""Helpers shared by the encoded-fetch tests: the truth of an encoded fetch built in numpy / Python
from a slice of reference-derived bytes (never from the code under test), a small parse of a record
file, the synthetic pairs and the hand-written records of the reader tests."""
import random
import re

import numpy as np

import synthlib

COMP = bytes.maketrans(b"ACGTRYKMBVDHacgtrykmbvdh", b"TGCAYRMKVBHDtgcayrmkvbhd")
CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = CODE[_c + 32] = _i
# the bit patterns of 0 and 1 per one-hot element type
ONE = {"u8": (np.uint8, 1), "f16": (np.uint16, 0x3C00), "bf16": (np.uint16, 0x3F80), "f32": (np.uint32, 0x3F800000)}
BPB = {("ascii", "u8"): 1, ("index", "u8"): 1, ("onehot", "u8"): 4, ("onehot", "f16"): 8, ("onehot", "bf16"): 8,
       ("onehot", "f32"): 16}


def split_fasta(fa: bytes) -> tuple[bytes, bytes]:
    """(header line, sequence): a FASTA text without its header line and its line ends."""
    hdr, _, body = fa.partition(b"\n")
    return hdr, body.replace(b"\n", b"")


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


def strand_bytes(truth: bytes, regions, strands, upper=False) -> list[bytes]:
    """Each region's ASCII bytes on its strand."""
    out = []
    for (b, e), r in zip(regions, strands):
        s = truth[b:e].upper() if upper else truth[b:e]
        out.append(revcomp(s) if r else s)
    return out


def encode(seq: bytes, encoding: str, dtype: str = "u8") -> bytes:
    """The encoded form of ASCII bytes already on their strand (complementing the letters and then
    taking codes is 3 - code on the codes)."""
    if encoding == "ascii":
        return seq
    code = CODE[np.frombuffer(seq, dtype=np.uint8)]
    if encoding == "index":
        return code.tobytes()
    t, one = ONE[dtype]
    eye = np.vstack([np.eye(4, dtype=np.uint8), np.zeros((1, 4), dtype=np.uint8)])
    return (eye[code].astype(t) * t(one)).tobytes()


def want_encoded(truth: bytes, regions, strands, encoding: str, dtype: str = "u8", upper=False) -> bytes:
    return encode(b"".join(strand_bytes(truth, regions, strands, upper)), encoding, dtype)


def check_encoded(rd, truth: bytes, regions, strands=None, encoding="index", dtype="u8", revcomp_all=False, upper=False,
                  what=""):
    """One batched fetch_encoded of `regions` against the truth's slices; names the first base that
    differs."""
    regions = list(regions)
    eff = [1] * len(regions) if revcomp_all else ([0] * len(regions) if strands is None else strands)
    got = rd.fetch_encoded(regions, encoding=encoding, dtype=dtype, strand=strands, revcomp=revcomp_all, upper=upper)
    want = want_encoded(truth, regions, eff, encoding, dtype, upper)
    if got == want:
        return
    bpb = BPB[(encoding, dtype)]
    assert len(got) == len(want), f"{what}: {len(got)} bytes, want {len(want)}"
    at = next(i for i in range(len(got)) if got[i] != want[i]) // bpb
    k, acc = 0, 0
    while acc + (regions[k][1] - regions[k][0]) <= at:
        acc += regions[k][1] - regions[k][0]
        k += 1
    raise AssertionError(f"{what} {encoding}/{dtype}: region {k} {regions[k]} strand {eff[k]} differs at base +{at - acc} "
                         f"(flat base {at}): got {got[at * bpb:at * bpb + 2 * bpb].hex()}, "
                         f"want {want[at * bpb:at * bpb + 2 * bpb].hex()}")


def clamp(regions, length):
    out = []
    for b, e in regions:
        b, e = max(0, min(b, length)), max(0, min(e, length))
        out.append((b, max(b, e)))
    return out


def parse_record(rec: bytes):
    """A small parse of a record file: (N runs [(start, len)], tokens [(decoded offset, len)],
    decoded length).  Run starts are running sums of the items' first numbers; a bare number is a
    run of one; a token's length bytes are decoded at its offset, every other byte of the record
    line is one decoded byte."""
    lines = rec.split(b"\n")
    if lines[0].startswith(b">"):
        lines = lines[1:]
    nline, enc = lines[1], lines[2]
    runs, at = [], 0
    if nline != b",":
        for m in re.finditer(rb"\((-?\d+),(\d+)\)|(-?\d+)", nline):
            at += int(m.group(1) if m.group(1) is not None else m.group(3))
            runs.append((at, int(m.group(2)) if m.group(2) is not None else 1))
    toks, o, prev = [], 0, 0
    for m in re.finditer(rb"\((-?\d+),(\d+)\)", enc):
        o += m.start() - prev
        toks.append((o, int(m.group(2))))
        o += int(m.group(2))
        prev = m.end()
    return runs, toks, o + len(enc) - prev


class Pair:
    """A synthetic pair compressed once: its target body is the truth."""

    def __init__(self, ctx, prof, rl, tl, seed):
        self.rfa, self.tfa = synthlib.synth_pair(prof, rl, tl, seed)
        self.rec = ctx.compress(self.rfa, self.tfa)
        self.hdr, self.truth = split_fasta(self.tfa)
        self.length = len(self.truth)
        runs, self.toks, D = parse_record(self.rec)
        keep = np.ones(self.length, dtype=bool)
        for s, l in runs:
            keep[s:s + l] = False
        self.d2j = np.append(np.nonzero(keep)[0], self.length)   # decoded offset -> sequence position
        assert len(self.d2j) == D + 1, "the test's record parse disagrees with the target"

    def boundaries(self):
        """{kind: positions}: every N / non-N and case transition of the truth, every token start
        and end in sequence coordinates; each kind capped at 500, seeded."""
        a = np.frombuffer(self.truth, dtype=np.uint8)
        is_n = (a | 0x20) == ord("n")
        low = (a >= ord("a")) & (a <= ord("z"))
        kinds = {"n": np.nonzero(is_n[1:] != is_n[:-1])[0] + 1, "case": np.nonzero(low[1:] != low[:-1])[0] + 1,
                 "tok_start": self.d2j[[o for o, _ in self.toks]], "tok_end": self.d2j[[o + l for o, l in self.toks]]}
        rng = random.Random(11)
        return {k: sorted(rng.sample([int(x) for x in v], min(500, len(v)))) for k, v in kinds.items()}


# the hand-written records of the reader tests (reference FASTA, record)
RFA = b">r\n" + b"ACGT" * 50 + b"\n"
RFA_N = b">r\n" + b"ACGTNNNNACGT" * 10 + b"\n"
HAND = {
    "literals_only": (RFA, b"\n\nACGTTGCAAC"),
    "stray_close_paren": (RFA, b"\n\nAC)GT(4,6)T)"),
    "token_first_and_last": (RFA, b"\n\n(0,10)TTT(20,12)"),
    "n_runs_start_end_adjacent": (RFA, b"\n(0,3)(10,2)(2,3)(18,4)\n(0,10)GG(10,10)"),
    "lowercase_spanning_n": (RFA, b"(5,20)\n(10,4)\n(3,14)GATTACA(40,9)"),
    "with_header": (RFA, b">hdr x\n(2,3)(7,2)\n(4,2)\nAC(8,30)T"),
    "without_header": (RFA, b"(2,3)(7,2)\n(4,2)\nAC(8,30)T"),
    "n_line_is_comma": (RFA_N, b"\n,\n(0,30)AC(10,20)"),
    "long_token_many_blocks": (RFA, b"\n\n" + b"(0,150)" + b"(1,0)" * 40 + b"GG(-38,100)" + b"T" * 130 + b"(3,7)"),
}
