"""FASTA pairs over arbitrary byte values and awkward '>' line layouts (parity tests).

Pure Python / numpy, seeded, deterministic (numpy's frozen RandomState stream).  The other generators
(fuzzgen.py, tools/synth.c) stay inside ACGT, N, a few IUPAC capitals and CRLF; these produce every
byte value a FASTA body can hold without touching the record's own token punctuation, on both sides
of a pair, and references / targets whose '>' lines sit where the strip kernels change state (word,
lane, 4 KiB tile, 16 KiB header-search step, scan block).

Geometry named here is the strip kernels': a word is 4 bytes, a lane 64, a tile 4096 file bytes; the
target's header search advances 16384 bytes a step; a scan block is 1024 tiles.
"""
from __future__ import annotations

import numpy as np

WORD, LANE, TILE, HDR_STEP, SCAN_BLOCK = 4, 64, 4096, 16384, 1024 * 4096

# '\n' ends a line; '(' ')' ',' digits and signs are the record's token punctuation (delta_encode's
# scan pairs them with real tokens): those stay with the paren generators of fuzzgen.py.
EXCLUDED = b"\n(),0123456789+-"
ALPHABET = bytes(c for c in range(256) if c not in EXCLUDED)

# Named representatives of the byte classes the kernels tell apart (or must not).
CLASSES = {
    "space": 0x20, "tab": 0x09, "vt": 0x0B, "ff": 0x0C, "cr": 0x0D,
    "nul": 0x00, "0x01": 0x01, "0x1f": 0x1F, "del": 0x7F,
    "@": 0x40, "[": 0x5B, "`": 0x60, "{": 0x7B,          # the neighbours of 'A'..'Z' and 'a'..'z'
    ">": 0x3E,                                            # never placed at a line start
    "R": 0x52, "r": 0x72, "Y": 0x59, "n": 0x6E, "N": 0x4E,
    "0x80": 0x80, "0xc1": 0xC1, "0xe1": 0xE1,             # 'A' / 'a' with bit 7 set
    "0xdf": 0xDF, "0xff": 0xFF,                           # the case-fold mask itself
}
_SLUG = {"@": "at", "[": "lbracket", "`": "backtick", "{": "lbrace", ">": "gt"}


def slug(cls: str) -> str:
    """A class name that is safe in a file name or a test id."""
    return _SLUG.get(cls, cls)


_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_ALPHA = np.frombuffer(ALPHABET, dtype=np.uint8)


def acgt(rs: np.random.RandomState, n: int) -> np.ndarray:
    return _ACGT[rs.randint(0, 4, n)]


def odd_bytes(rs: np.random.RandomState, n: int) -> np.ndarray:
    return _ALPHA[rs.randint(0, len(_ALPHA), n)]


def to_fasta(seq, header: bytes | None = b">seq", width: int = 60, crlf: bool = False,
             final_newline: bool = True) -> bytes:
    """`seq` (bytes or uint8 array, any byte but '\\n') in lines of `width`."""
    a = np.frombuffer(bytes(seq), dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq
    n = len(a)
    rows = (n + width - 1) // width
    eol = 2 if crlf else 1
    m = np.full((rows, width + eol), 10, dtype=np.uint8)
    if crlf:
        m[:, width] = 13
    pad = np.zeros(rows * width, dtype=np.uint8)
    pad[:n] = a
    m[:, :width] = pad.reshape(rows, width)
    body = m.reshape(-1).tobytes()
    if rows:
        last = n - (rows - 1) * width                      # bases on the last line
        body = body[:(rows - 1) * (width + eol) + last] + (b"\r\n" if crlf else b"\n")
        if not final_newline:
            body = body[:-eol]
    head = b"" if header is None else header + (b"\r\n" if crlf else b"\n")
    return head + body


def odd_sequences(seed: int, n: int, kind: str = "local"):
    """(ref, tgt) uint8 arrays: an ACGT reference with about 1 in 40 bytes drawn from ALPHABET; the
    target a copy with 1% SNPs, further odd bytes (1 in 300), soft-masked runs and two inserted N runs -- so
    most odd bytes are shared and sit inside k-mers that match.  kind "global": 5 kb inserted early."""
    rs = np.random.RandomState(70_000 + seed)
    ref = acgt(rs, n).copy()
    odd = rs.random_sample(n) < 1 / 40
    ref[odd] = odd_bytes(rs, int(odd.sum()))
    tgt = ref.copy()
    snp = rs.random_sample(n) < 0.01
    tgt[snp] = acgt(rs, int(snp.sum()))
    more = rs.random_sample(n) < 1 / 300
    tgt[more] = odd_bytes(rs, int(more.sum()))
    for _ in range(max(2, n // 1500)):                     # soft-masked runs (ASCII letters fold, nothing else)
        a = int(rs.randint(0, n))
        b = min(n, a + int(rs.choice([1, 2, 3, 40, 300])))
        s = tgt[a:b]
        up = (s >= 65) & (s <= 90)
        s[up] += 32
    for _ in range(2):                                     # inserted, not overwritten: erasing them leaves T' aligned with R'
        a = int(rs.randint(0, n))
        tgt = np.concatenate([tgt[:a], np.full(int(rs.choice([1, 7, 130])), ord("N"), dtype=np.uint8), tgt[a:]])
    if kind == "global":
        a = int(rs.randint(0, min(3000, n)))
        tgt = np.concatenate([tgt[:a], acgt(rs, 5000), tgt[a:]])
    elif kind != "local":
        raise ValueError(kind)
    return ref, tgt


def odd_pair(seed: int, n: int, kind: str = "local") -> tuple[bytes, bytes]:
    """(ref_fa, tgt_fa) of odd_sequences; line widths and CRLF vary with the seed.  A random '>' may
    land at a line start (a dropped reference line, or the target's header): that is the format."""
    ref, tgt = odd_sequences(seed, n, kind)
    rw = [60, 61, 70, 50][seed % 4]
    tw = [50, 60, 80, 63][(seed // 2) % 4]
    return (to_fasta(ref, b">ref odd", rw, crlf=seed % 5 == 4),
            to_fasta(tgt, b">tgt odd" if seed % 3 else None, tw, crlf=seed % 4 == 3, final_newline=seed % 7 != 6))


# ---- one class byte at every offset that matters ---------------------------------------------------
def placed(cls: str, side: str, n: int = 17_000, seed: int = 0) -> tuple[bytes, bytes]:
    """(ref_fa, tgt_fa): `side` ("tgt" or "ref") holds the class byte at every in-word offset 0..3,
    at lane offsets 0, 1, 62, 63 and at tile offsets 0, 1, 4094, 4095 (file offsets; never on a line
    end), as the first byte of a line, the last byte before '\\n' and the last byte of the file
    (which has no final newline), alone and in runs of 2, 3 (more than two holes in a lane) and 65 (a
    whole lane and more).  The other side is the same ACGT sequence, plain; `seed` picks the sequence."""
    if side not in ("tgt", "ref"):
        raise ValueError(side)
    b = CLASSES[cls]
    rs = np.random.RandomState(80_000 + 256 * seed + b)
    seq = acgt(rs, n)
    width = 100
    hdr = b">p"
    fa = bytearray(to_fasta(seq, hdr, width, final_newline=False))
    body0 = len(hdr) + 1
    used: set[int] = set()

    def free(p: int, ln: int) -> bool:
        if p < body0 or p + ln > len(fa):
            return False
        if any(fa[q] == 10 for q in range(p, p + ln)):
            return False
        if b == 0x3E and fa[p - 1] == 10:                  # '>' never at a line start
            return False
        return not any(q in used for q in range(p - 1, p + ln + 1))   # runs keep their length

    def put_at(p: int, ln: int = 1) -> None:
        assert free(p, ln), (cls, p, ln)
        fa[p:p + ln] = bytes([b]) * ln
        used.update(range(p, p + ln))

    def put(mod: int, off: int, ln: int = 1, start: int = 0) -> None:
        p = start - start % mod + off
        while not free(p, ln):
            p += mod
            assert p < len(fa), (cls, mod, off, ln)
        put_at(p, ln)

    for o in (0, 1, 4094, 4095):                           # tile offsets
        put(TILE, o, start=TILE)
    put(TILE, 4095, 3, start=2 * TILE)                     # a run of 3 across a tile edge
    for o in (0, 1, 62, 63):                               # lane offsets
        put(LANE, o, start=300)
    for o in range(4):                                     # in-word offsets
        put(WORD, o, start=700 + 40 * o)
    put(LANE, 10, 2, start=1200)
    put(LANE, 63, 2, start=1400)                           # a run of 2 across a lane edge
    put(LANE, 20, 3, start=1600)                           # three holes in one lane
    put(LANE, 0, 65, start=2000)                           # a whole lane and one more byte
    put(LANE, 40, 65, start=2400)                          # parts of three lanes
    nls = [i for i, c in enumerate(fa) if c == 10]
    if b != 0x3E:
        put_at(nls[30] + 1)                                # first byte of a line
    put_at(nls[33] - 1)                                    # last byte before '\n'
    put_at(len(fa) - 1)                                    # last byte of a file without a final newline
    plain = to_fasta(seq, hdr, 60)
    return (plain, bytes(fa)) if side == "tgt" else (bytes(fa), plain)


# ---- '>' line layouts ------------------------------------------------------------------------------
class _Builder:
    """A FASTA written piece by piece: sequence lines taken from `seq` in order, raw bytes between."""

    def __init__(self, seq: bytes, eol: bytes = b"\n"):
        self.seq, self.i, self.out, self.eol = bytes(seq), 0, bytearray(), eol

    def raw(self, b: bytes) -> "_Builder":
        self.out += b
        return self

    def line(self, nbases: int) -> "_Builder":
        assert self.i + nbases <= len(self.seq), "the sequence is too short for this layout"
        self.out += self.seq[self.i:self.i + nbases] + self.eol
        self.i += nbases
        return self

    def lines(self, nbases: int, width: int = 60) -> "_Builder":
        while nbases > 0:
            self.line(min(width, nbases))
            nbases -= width
        return self

    def until(self, pos: int, width: int = 60) -> "_Builder":
        """Sequence lines until the file is exactly `pos` bytes long (its last byte a line end)."""
        e = len(self.eol)
        gap = pos - len(self.out)
        assert gap >= 1 + e, (pos, len(self.out))
        while gap > 2 * (width + e):
            self.line(width)
            gap -= width + e
        if gap > width + e:
            a = gap // 2
            self.line(a - e)
            gap -= a
        self.line(gap - e)
        assert len(self.out) == pos
        return self

    def rest(self, width: int = 60, final_newline: bool = True) -> bytes:
        self.lines(len(self.seq) - self.i, width)
        out = bytes(self.out)
        return out if final_newline else out[:len(out) - len(self.eol)]


REF_LAYOUTS = ("many_records", "gulfs", "crlf", "spaced_gt", "last_gt_no_newline", "gt_at_tile", "gt_lane63",
               "gt_long_tile", "no_first_header")


def ref_layout(seq: bytes, case: str) -> bytes:
    """A reference FASTA over `seq` (>= 14,000 bytes) with more than one '>' line.  Every '>' line
    is dropped and every other non-empty line is sequence (compression.cpp:187-200)."""
    b = _Builder(seq)
    if case == "many_records":   # '>' lines of length 0..9000, some back to back, blank lines between
        for k, ln in enumerate([0, 1, 62, 63, 64, 4094, 4095, 4096, 9000]):
            b.raw(b">" + bytes([ord("a") + k]) * ln + b"\n")
            if k % 3 == 1:
                b.raw(b"\n>\n\n>back to back\n")
            b.lines(700 + 61 * k)
        return b.rest()
    if case == "gulfs":          # blank-line gulfs (one wider than 64 tiles) before and after '>' lines
        b.raw(b"\n\n>r one\n").lines(1500)
        b.raw(b"\n" * (5 * TILE + 13) + b">r two\n").lines(1500)
        b.raw(b">r three\n" + b"\n" * (70 * TILE + 13)).lines(1500)
        b.raw(b"\n" * (TILE - 1) + b">r four\n" + b"\n" * TILE)
        return b.rest()
    if case == "crlf":           # CRLF everywhere; a blank line is "\r", which is not empty
        b = _Builder(seq, b"\r\n")
        b.raw(b">r one\r\n").lines(2000)
        b.raw(b"\r\n\r\n>r two\r\n>\r\n").lines(3000, 70)
        b.raw(b">r three\r\n\r\n")
        return b.rest(61)
    if case == "spaced_gt":      # ' >' and tab '>' lines and '>' inside lines are sequence; '>' lines are not
        b.raw(b">r one\n").lines(1000)
        b.raw(b" >spaced is sequence\n").lines(500)
        b.raw(b"\t>tabbed\n\r>after cr\n>dropped > with > inside\n").lines(500)
        b.raw(b"ACG>TA>>C\n>\n >\n").lines(500)
        return b.rest()
    if case == "last_gt_no_newline":
        b.raw(b">r one\n").lines(3000)
        b.raw(b">r two\n")
        return b.rest() + b">the last line, without a line end"
    if case == "gt_at_tile":     # '>' exactly at byte 4096 t, the '\n' before it at 4096 t - 1
        b.raw(b">r\n").until(TILE).raw(b">at a tile edge\n")
        b.until(2 * TILE).raw(b">\n")
        b.until(3 * TILE).raw(b">" + b"x" * (TILE - 2) + b"\n")   # a '>' line that is exactly one tile
        return b.rest()
    if case == "gt_lane63":      # a '>' line that begins in lane 63 of a tile and ends in the next tile
        b.raw(b">r\n").until(TILE - 20).raw(b">" + b"l" * 50 + b"\n")
        b.until(2 * TILE - 1).raw(b">" + b"m" * 63 + b"\n")       # '>' is the tile's last byte
        b.until(3 * TILE - LANE).raw(b">" + b"k" * 200 + b"\n")   # ... the first byte of lane 63
        return b.rest()
    if case == "gt_long_tile":   # a '>' line longer than a tile: one whole tile holds no line start
        b.raw(b">r\n").until(TILE + 100).raw(b">" + b"L" * 9000 + b"\n").lines(900)
        b.raw(b">" + b"M" * (3 * TILE) + b"\n")
        return b.rest()
    if case == "no_first_header":   # the file begins with sequence; '>' lines come later
        b.lines(2000).raw(b">late\n").lines(2000).raw(b">later\n")
        return b.rest()
    raise ValueError(case)


def header_seams(rfa: bytes) -> list[int]:
    """For every '>' line of a reference: how many sequence bytes (whitespace removed) the lines
    before it hold -- the position in R where the records on either side of it meet."""
    out, kept = [], 0
    for ln in rfa.split(b"\n"):
        if ln.startswith(b">"):
            out.append(kept)
        else:
            kept += sum(1 for c in ln if c not in b" \t\v\f\r")
    return out


TGT_LAYOUTS = ("line2", "line68", "line69", "line70", "middle", "end", "end_no_newline", "empty_header", "long_5000",
               "odd_bytes", "second_gt", "inner_gt_only", "at_16384", "straddle_16384", "longer_than_16k",
               "long_from_16000")


def tgt_header_layout(seq: bytes, case: str) -> bytes:
    """A target FASTA over `seq` (>= 20,000 bytes) whose header -- the first line that starts with
    '>' -- is not its first line; the lines before it are sequence, and so is any later '>' line
    (compression.cpp:207-218)."""
    b = _Builder(seq)
    if case == "line2":
        return b.line(60).raw(b">t on line two\n").rest()
    if case in ("line68", "line69", "line70"):   # 61-byte lines: the '>' at byte 4087, 4148, 4209
        return b.lines(60 * (int(case[4:]) - 1)).raw(b">t after a tile\n").rest()
    if case == "middle":
        return b.lines(len(seq) // 2, 70).raw(b">t in the middle\n").rest(70)
    if case == "end":
        return b.rest() + b">t at the end\n"
    if case == "end_no_newline":
        return b.rest() + b">t at the end"
    if case == "empty_header":
        return b.line(60).line(60).raw(b">\n").rest()
    if case == "long_5000":
        return b.line(60).raw(b">" + b"h" * 4999 + b"\n").rest()
    if case == "odd_bytes":      # tab, a high byte and token punctuation in the header line
        return b.line(60).raw(b">t\tname \x80\xc1 (5, [x] {y}\n").rest()
    if case == "second_gt":
        b.line(60).raw(b">t first header\n").lines(3000)
        return b.raw(b">second is sequence\n").rest()
    if case == "inner_gt_only":  # '>' inside lines and behind a space only: there is no header
        b.line(60).raw(b" >not a header\n").lines(1200).raw(b"AC>GT\n")
        return b.rest()
    if case == "at_16384":       # the header begins at byte 16384, the '\n' before it at 16383
        return b.until(HDR_STEP).raw(b">t at the search step\n").rest()
    if case == "straddle_16384":
        return b.until(HDR_STEP - 10).raw(b">t across the search step\n").rest()
    if case == "longer_than_16k":
        return b.line(60).raw(b">" + b"H" * 17_000 + b"\n").rest()
    if case == "long_from_16000":   # a header longer than a step that begins late in the first step
        return b.until(16_000).raw(b">" + b"G" * 17_000 + b"\n").rest()
    raise ValueError(case)


# ---- tiles that alternate between the write pass's paths ----------------------------------------------
def tile_mix(seed: int = 0, rounds: int = 3) -> tuple[bytes, bytes]:
    """(ref_fa, tgt_fa): a target whose 4 KiB tiles alternate between plain (ACGT in 63-base lines),
    non-plain through one odd byte without a digit, non-plain through a lane with three whitespace
    bytes (two trailing spaces before CRLF, a tab-separated line) and all-whitespace.  The reference
    is the same sequence, plain."""
    rs = np.random.RandomState(90_000 + seed)
    out = bytearray(b">" + b"m" * (TILE - 2) + b"\n")     # the header fills tile 0
    seq = bytearray()

    def bases(k: int) -> bytes:
        s = acgt(rs, k).tobytes()
        seq.extend(s)
        return s

    def plain_tile() -> bytearray:
        t = bytearray()
        for _ in range(TILE // LANE):
            t += bases(LANE - 1) + b"\n"
        return t

    odd = [0x40, 0xC1, 0x7B, 0x00, 0x52, 0x6E]
    for r in range(rounds):
        out += plain_tile()
        t = plain_tile()                                   # one odd byte, at a different lane each round
        p = (17 * r + 5) * LANE + (r % 4) + 8
        c = odd[r % len(odd)]
        seq_at = len(seq) - (TILE - TILE // LANE) + (p - p // LANE)
        t[p] = c
        seq[seq_at] = c
        out += t
        t = bytearray()                                    # a lane with three whitespace bytes
        t += bases(60) + b"  \r\n"
        t += bases(15) + b"\t" + bases(15) + b"\t" + bases(15) + b"\t" + bases(15) + b"\n"
        for _ in range(TILE // LANE - 2):
            t += bases(LANE - 1) + b"\n"
        out += t
        out += (b" \t\r\v\f  \n" * (TILE // 8))            # all whitespace
    out += plain_tile()
    assert len(out) % TILE == 0
    s = bytes(seq)
    snp = bytearray(s)
    for i in range(500, len(snp), 997):                    # the reference differs by a few SNPs
        snp[i] = ord("A") if snp[i] != ord("A") else ord("C")
    return to_fasta(bytes(snp), b">ref", 60), bytes(out)


# ---- a pair that crosses a scan block ----------------------------------------------------------------
def scan_edge_pair(seed: int = 0, n: int = 4_300_000) -> tuple[bytes, bytes]:
    """(ref_fa, tgt_fa) of odd_sequences(n) laid out so that file byte 4096 * 1024 (the first byte
    of the second scan block) lies inside a '>' line of the reference, which a 65-byte run of odd
    bytes follows, and inside a 65-byte run of odd bytes of the target."""
    ref, tgt = odd_sequences(1000 + seed, n, "local")
    rs = np.random.RandomState(95_000 + seed)
    run_r, run_t = odd_bytes(rs, 65), odd_bytes(rs, 65)
    rb = _Builder(ref.tobytes()).raw(b">ref scan\n").until(SCAN_BLOCK - 32)
    rb.raw(b">" + b"e" * 62 + b"\n")                       # bytes [edge - 32, edge + 32)
    ref[rb.i:rb.i + 65] = run_r
    rb.seq = ref.tobytes()
    rfa = rb.rest()
    tb = _Builder(tgt.tobytes()).raw(b">tgt scan\n").until(SCAN_BLOCK - 40)
    tgt[tb.i + 8:tb.i + 73] = run_t                        # file bytes [edge - 32, edge + 33)
    tb.seq = tgt.tobytes()
    tb.line(100)
    return rfa, tb.rest(70)
