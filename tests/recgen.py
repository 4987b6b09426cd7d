"""Hand-built record files at the edges of the decoder's grammar, each labelled by construction.

The decoder is otherwise tested on records the compressor wrote: unsigned, unpadded numbers,
ascending runs, three or four lines.  This module writes the records a compressor never writes but
decompression.cpp defines a result for, and the ones it fails on.  Pure Python, seeded, no GPU.

THE GRAMMAR (what decomp.hip accepts; everything else it reports as SCCG_E_PARSE)

  integer    an optional '+' or '-' and 1 to 10 decimal digits, the value within int32.
  run line   items separated by any number of ',' (also leading and trailing ones):
               "(d,l)"   d, l integers, l >= 0, at most 25 bytes; a ',' right after ')' is consumed;
               "d"       a bare integer, a run of one; ',' or the line's end follows it.
             An item's start is the previous item's start plus d (0 before the first).  Starts are
             >= 0, ascending and disjoint (start >= previous start + previous l; adjacent and
             zero-length runs are fine), every end within int32.  No other byte occurs.
  N line     a run line; the line "," alone means "no N runs, keep the reference's own N"
             (decompression.cpp:105-109).  The last N run ends within decoded length + N count.
             Lowercase runs may pass the sequence end: the part beyond is dropped (:255-262).
  record     "(d,l)" tokens as above (p = previous p + d, 0 <= p, p + l <= |R'|, else
  line       SCCG_E_RANGE); every byte outside a token is a literal, ',' digits ')' and all.
             A '(' always opens a token.
  file       an optional header line (first byte '>'), the lowercase line, the N line, the record
             line; '\n' ends a line, the last may lack it; anything after the record line is
             ignored; a missing line is SCCG_E_FORMAT.

THE THREE CLASSES

  exact      inside the grammar: status and bytes equal the oracle's (= decompression.cpp's).
  reject_ok  decompression.cpp defines a result (std::stoi skips leading blanks, stops at junk and
             takes any number of leading zeros; it sorts the expanded run positions, so descending
             and overlapping lowercase runs work) but the text is outside the grammar: the GPU gives
             the oracle's exact bytes or SCCG_E_PARSE, nothing else.
  error      the oracle fails: the GPU fails with FORMAT, PARSE or RANGE -- the class named in
             `expect` when the record holds one fault.  With two faults the GPU reports PARSE from
             any line before RANGE (the oracle: the first in reading order).

`undefined` marks cases where decompression.cpp itself has no defined behaviour (a find() that
returns npos, a negative substr length, N positions past the end): the compiled reference is not
asked about those.  Only members of families b and f carry it.

Moved by argument from decompression.cpp, not from the GPU's behaviour:
  * a bare run-line number that reaches the end of a 512-byte tile's staged bytes (tile end + 64)
    starts inside the tile, so it is at least 65 bytes wide: more than 10 digits, outside the
    grammar whatever its value.  Those records are `reject_ok` (family e), not `exact`.
  * overlapping N runs give :244-252 duplicate positions, after which it reads
    reconstructed_genome past its end: `error`, undefined, filed with the run-list family b.
"""
from __future__ import annotations

import random
import re
from collections import namedtuple

Case = namedtuple("Case", "name ref_fa record klass expect undefined family")

EXACT, REJECT_OK, ERROR = "exact", "reject_ok", "error"
FORMAT, PARSE, RANGE = "SCCG_E_FORMAT", "SCCG_E_PARSE", "SCCG_E_RANGE"


def _case(name, ref_fa, record, klass=EXACT, expect=None, undefined=False):
    assert klass in (EXACT, REJECT_OK, ERROR) and (expect is None or klass == ERROR)
    assert not undefined or name[0] in "bf"
    return Case(name, ref_fa, record, klass, expect, undefined, name[0])


def fasta(seq: bytes, header: bytes = b">ref", width: int = 60) -> bytes:
    return header + b"\n" + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def _bases(n: int, seed: int) -> bytes:
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def stripped(ref_fa: bytes, keep_n: bool = False) -> bytes:
    """R' of decompression.cpp:47-58, 105-110 for the plain references used here."""
    s = b"".join(l for l in ref_fa.split(b"\n") if l and l[:1] != b">")
    return (s if keep_n else s.replace(b"N", b"")).upper()   # (:108 erases 'N' before :110's toupper)


# the references: plain bases; bases with N runs and lowercase (the erased form is shorter)
SEQ_A = _bases(1500, 1)
REF_A = fasta(SEQ_A)
SEQ_N = b"".join((_bases(37, 10 + i) + (b"NNNNN" if i % 2 else b"nnn") + _bases(20, 40 + i).lower()) for i in range(6))
REF_N = fasta(SEQ_N, b">with n", 50)
SEQ_S = _bases(200, 2)
REF_S = fasta(SEQ_S, b">r")
REFS = {"A": REF_A, "N": REF_N, "S": REF_S}


# ---------------------------------------------------------------------------------------------
# numbers and items of an exact byte width
# ---------------------------------------------------------------------------------------------
def field(v: int, fw: int, rng: random.Random) -> bytes:
    """v in exactly fw bytes (1..11): a sign where needed or, by chance, where it fits; zeros."""
    digits = str(abs(v))
    if v < 0 or fw == 11 or (fw > len(digits) and rng.random() < 0.5):
        assert fw - 1 >= len(digits), (v, fw)
        sign = b"-" if v < 0 or (v == 0 and rng.random() < 0.3) else b"+"
        return sign + digits.rjust(fw - 1, "0").encode()
    assert len(digits) <= fw <= 10, (v, fw)
    return digits.rjust(fw, "0").encode()


def split_width(w: int, rng: random.Random) -> tuple[int, int]:
    """Field widths of a "(d,l)" item of w bytes (5..25)."""
    t = w - 3
    fd = rng.randint(max(1, t - 11), min(11, t - 1))
    return fd, t - fd


def fits(v: int, fw: int) -> bool:
    return len(str(abs(v))) <= (fw - 1 if v < 0 or fw == 11 else min(fw, 10))


def item(d: int, l: int, w: int, rng: random.Random) -> bytes:
    for _ in range(64):
        fd, fl = split_width(w, rng)
        if fits(d, fd) and fits(l, fl):
            out = b"(" + field(d, fd, rng) + b"," + field(l, fl, rng) + b")"
            assert len(out) == w
            return out
    raise AssertionError((d, l, w))


def run_filler(n: int, rng: random.Random) -> tuple[bytes, int]:
    """n bytes of a run line before the items under test: mostly ',', some small items.  Returns
    the text and the running start it leaves (its last item is a run of one or none)."""
    out, at = b"", 0
    while len(out) < n:
        pick = rng.random()
        piece, step = b",", 0
        if pick < 0.08 and at < 300:
            piece, step = b"1,", 1
        elif pick < 0.14 and at < 300:
            piece, step = b"(2,1)" + (b"," if rng.random() < 0.5 else b""), 2
        elif pick < 0.18 and at < 300:
            piece, step = b"(1,0)", 1
        if len(out) + len(piece) > n:
            piece, step = b",", 0
        out += piece
        at += step
    return out, at


def sweep_record(off: int) -> bytes:
    """Family a: on all three lines a few wide items start `off` bytes into the line."""
    rng = random.Random(1000 + off)
    nref = len(SEQ_A)
    lines = []
    for line in range(2):                       # lowercase line, N line
        text, at = run_filler(off, rng)
        prev_end = at + 1
        for k in range(4):
            w = 5 + (off * 4 + k * 7 + line * 3) % 21
            ln = rng.randint(0, 9)
            d = max(prev_end - at, 0) + rng.randint(0, 6) if (k or off) else rng.randint(0, 6)
            if d > 9:
                w = max(w, 6 + len(str(d)))
            text += item(d, ln, w, rng)
            at += d
            prev_end = at + ln
            text += b"," if rng.random() < 0.5 else b""
        if rng.random() < 0.5:
            d = max(prev_end - at, 0) + rng.randint(0, 3)
            text += b"%d" % d
            at += d
            prev_end = at + 1
        lines.append((text, prev_end))
    enc = bytes(rng.choice(b"ACGT") for _ in range(off))
    p = 0
    for k in range(4):
        w = 5 + (off * 4 + k * 7 + 11) % 21
        fd, fl = split_width(w, rng)
        ln = rng.randint(0, min(60, 10 ** min(fl - (fl == 11), 3) - 1))
        span = 10 ** min(fd - 1, 4) - 1 if fd > 1 else 0
        lo, hi = max(0, p - span), min(nref - 60, p + (10 ** min(fd, 4) - 1 if fd < 11 else span))   # (ln <= 60)
        q = rng.randint(lo, hi)
        tok = b"(" + field(q - p, fd, rng) + b"," + field(ln, fl, rng) + b")"
        assert len(tok) == w, (off, k, q - p, ln, w)
        enc += tok + bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 3)))
        p = q
    enc += bytes(rng.choice(b"ACGT,9)") for _ in range(10))
    # the N runs must end within decoded + N: pad the record line with literals where they do not
    dec = decoded_length(enc)
    nruns = parse_runs(lines[1][0])
    ntot = sum(l for _, l in nruns)
    need = max((s + l for s, l in nruns), default=0) - (dec + ntot)
    if need > 0:
        enc += bytes(rng.choice(b"ACGT") for _ in range(need))
    hdr = b">sweep %d\n" % off if off % 2 else b""
    return hdr + lines[0][0] + b"\n" + lines[1][0] + b"\n" + enc + (b"\n" if off % 3 else b"")


# ---------------------------------------------------------------------------------------------
# a small model of a record inside the grammar: which sequence positions its tile edges touch
# ---------------------------------------------------------------------------------------------
_TOK = re.compile(rb"\(([+-]?\d+),([+-]?\d+)\)")
_ITEM = re.compile(rb"\(([+-]?\d+),([+-]?\d+)\)|([+-]?\d+)")


def parse_runs(line: bytes, spans: bool = False):
    """[(start, len)] of a run line inside the grammar (with spans: [(byte offset, start, len)])."""
    if line == b",":
        return []
    out, at = [], 0
    for m in _ITEM.finditer(line):
        at += int(m.group(1) if m.group(1) is not None else m.group(3))
        ln = int(m.group(2)) if m.group(2) is not None else 1
        out.append((m.start(), at, ln) if spans else (at, ln))
    return out


def decoded_length(enc: bytes) -> int:
    n, prev = 0, 0
    for m in _TOK.finditer(enc):
        n += m.start() - prev + int(m.group(2))
        prev = m.end()
    return n + len(enc) - prev


def lines_of(record: bytes):
    """(header or None, lowercase line, N line, record line) by decompression.cpp:66-101."""
    ls = record.split(b"\n")
    hdr = None
    if ls[0][:1] == b">":
        hdr, ls = ls[0], ls[1:]
    return hdr, ls[0], ls[1], ls[2]


def probe_positions(record: bytes, length: int) -> list[int]:
    """Sequence positions the record's tile edges touch: the decoded bytes of the record line's
    1 KiB and 64-byte-block-of-a-tile edges (every multiple of 512), the runs whose items lie near a
    multiple of 512 of their run line, and both ends of the sequence.  For records inside the
    grammar; anything unparsable just gives the ends."""
    pos = {0, length}
    try:
        _, lower, nline, enc = lines_of(record)
        nruns = parse_runs(nline)

        def seq_pos(o):   # decoded offset -> sequence position (N runs ascending)
            for s, l in nruns:
                if s <= o:
                    o += l
            return o
        o, prev, edges = 0, 0, list(range(512, len(enc) + 1, 512))
        for m in list(_TOK.finditer(enc)) + [None]:
            a, b = (m.start(), m.end()) if m else (len(enc), len(enc))
            for e in edges:
                if prev <= e < a:
                    pos.add(seq_pos(o + e - prev))
                elif a <= e < b:
                    pos.add(seq_pos(o + a - prev))
                    pos.add(seq_pos(o + a - prev + int(m.group(2))))
            o += a - prev + (int(m.group(2)) if m else 0)
            prev = b
        for line in (lower, nline):
            for at, s, l in parse_runs(line, spans=True):
                if at % 512 < 40 or at % 512 > 512 - 40:
                    pos.update((s, s + l))
    except (ValueError, IndexError):
        pass
    return sorted(p for p in pos if 0 <= p <= length)


# ---------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------
def family_a() -> list[Case]:
    out = [_case(f"a_off{off:04d}", REF_A, sweep_record(off)) for off in range(0, 1101)]
    rng = random.Random(7)
    # the 25-byte extremes, values in range after the running sum
    for edge in (512, 1024):
        for shift in (0, 1, 12, 24, 25, 31, 32, 33):
            lit = _bases(edge - shift, edge + shift)
            enc = lit + b"(+0000001400,+0000000100)" + b"AC" + b"(-0000001400,+0000000033)" + b"(+0000000000,-0000000000)GT"
            low = b"," * (edge - shift) + b"(+0000000002,+0000000003)(+0000000003,+0000000000),(+0000000000,+0000000002)"
            nl = b"," * (edge - shift) + b"(+0000000000,+0000000002),(+0000000004,+0000000001)"
            out.append(_case(f"a_extreme25_{edge}_{shift:02d}", REF_A, low + b"\n" + nl + b"\n" + enc + b"\n"))
    # +0, -0 and negative deltas that return to valid positions
    out.append(_case("a_signed_zero", REF_A, b"(+0,2)(+5,-0)(-0,1)\n(-0,+1),(+3,1)\n(+0,10)AC(-0,5)(+90,7)(-90,7)(-0,+0)G(+1499,1)(-1499,+1)\n"))
    out.append(_case("a_negative_returns", REF_A, b"(9,1)\n(4,2)\n(1000,50)(-1000,50)(+500,00020)(-00500,1)T\n"))
    # a literal run of more than 32 bytes without a parenthesis across a tile edge, between tokens
    for edge in (64, 512, 1024, 2048):
        for lead in (20, 33, 40):
            lit = bytes(rng.choice(b"0123456789,+-ACGT") for _ in range(80))
            pre = _bases(edge - lead - 7, edge)
            enc = pre + b"(100,12)" + lit + b"(-50,30)" + b"ACGT"
            assert enc.index(lit) < edge < enc.index(lit) + 80
            out.append(_case(f"a_long_literal_{edge}_{lead}", REF_A, b"\n\n" + enc))
    # items ending exactly at, and one byte around, the tile edges of both run lines
    for edge in (512, 1024):
        for w in (5, 13, 25):
            for end in (edge - 1, edge, edge + 1):
                pad = b"," * (end - w)
                it = item(3, 2, w, rng)
                low = pad + it + b"(4,1),2"
                out.append(_case(f"a_item_ends_{edge}_{w}_{end - edge:+d}", REF_A, low + b"\n" + low + b"\n(7,90)ACGT\n"))
    return out


def family_b() -> list[Case]:
    c = []
    enc30 = b"(10,30)"

    def add(name, lower, nline, enc=enc30, ref=REF_S, **kw):
        c.append(_case("b_" + name, ref, lower + b"\n" + nline + b"\n" + enc + b"\n", **kw))
    add("zero_len_alone", b"(5,0)", b"(7,0)")
    add("zero_len_only_first", b"(0,0)", b"(0,0)")
    add("zero_len_between_adjacent", b"(3,4)(4,0)(0,5)", b"(2,2)(2,0)(0,3)")
    add("adjacent", b"(2,3)(3,4)(4,1)1,1", b"(1,2)(2,2)2,1")
    add("comma_after_close_mixed", b"(2,3),(4,2)(5,1)7,(3,2)", b"(1,1),(3,1)(2,1)4,(3,2)")
    add("empty_items", b",,(2,3),,4,,(3,1),", b",,(1,2),,5,,,(2,1),,")
    add("only_commas", b",,,", b",,")
    add("lower_wholly_past_end", b"(10,5)(40,5)", b"")
    add("lower_partly_past_end", b"(28,5)", b"")
    add("lower_partly_past_end_with_n", b"(3,2)(28,9)", b"(4,3)")
    add("lower_starts_at_end", b"(30,4)", b"")
    add("lower_far_past_end", b"(2,1)(2147483000,600)", b"")
    add("lower_over_n_run", b"(5,20)", b"(10,4)")
    add("n_at_first_and_last", b"", b"(0,3)(33,2)")
    add("n_bare_last", b"", b"30")
    add("n_only", b"(1,2)", b"(0,4)", enc=b"")
    add("n_ends_one_past", b"", b"(0,3)(34,2)", klass=ERROR, expect=PARSE, undefined=True)
    add("n_bare_one_past", b"", b"31", klass=ERROR, expect=PARSE, undefined=True)
    add("n_overlap", b"", b"(5,10)(3,10)", klass=ERROR, expect=PARSE, undefined=True)
    add("n_line_comma_kept", b"(3,50)", b",", enc=b"(0,30)AC(10,20)(100,90)", ref=REF_N)
    add("n_line_two_commas_erased", b"(3,50)", b",,", enc=b"(0,30)AC(10,20)(100,90)", ref=REF_N)
    add("n_line_comma_kept_last_base", b"", b",", enc=b"(%d,1)" % (len(stripped(REF_N, True)) - 1), ref=REF_N)
    add("n_line_erased_last_base", b"", b"", enc=b"(%d,1)" % (len(stripped(REF_N)) - 1), ref=REF_N)
    return c


def family_c() -> list[Case]:
    c = []
    odd = bytes([0]) + bytes(range(0x80, 0x100))
    c.append(_case("c_punctuation", REF_S, b"(2,40)\n(5,3)\nAC,GT12+3-4)>X \t\rZ(3,4)),,9(10,20)+-7)\n"))
    c.append(_case("c_odd_bytes", REF_S, b"(2,200)\n(5,3)\n" + odd + b"(3,4)" + odd[::-1] + b"(0,9)" + odd[:70] + b"\n"))
    c.append(_case("c_close_after_token", REF_S, b"\n\n(3,4))(5,6)))A)(0,2)"))
    c.append(_case("c_only_close_parens", REF_S, b"\n\n" + b")" * 130))
    c.append(_case("c_header_with_token", REF_S, b">h(1,2),x (\n(2,3)\n(4,2)\nAC(8,30)T\n"))
    c.append(_case("c_digits_before_token", REF_S, b"(1,5)\n\n12,34(3,4)56,78(1,2)9\n"))
    c.append(_case("c_cr_in_record_line", REF_S, b"\n\nAC(0,5)\r\n"))
    for edge in (64, 1024):   # literals that look like the inside of a token, up to a tile edge
        lit = (b"1,2)" * 300)[:edge - 3]
        c.append(_case(f"c_token_like_literals_{edge}", REF_S, b"\n\n" + lit + b"(3,4)" + lit[:50] + b"(1,1)"))
    return c


def family_d() -> list[Case]:
    c = []
    c.append(_case("d_no_final_newline_token", REF_S, b"(1,2)\n(3,1)\nAC(3,40)"))
    c.append(_case("d_no_final_newline_literal", REF_S, b">h\n(1,2)\n(3,1)\n(3,40)AC"))
    junk = [b"(9999,5)", b"(1x,2)(", b"((", b"(0,5)(500,30)", b"", b">x", b"(2147483648,1)"]
    for hdr in (b"", b">h\n"):
        for k in (1, 2, 27, 28, 29, 31, 32, 33, 200):
            tail = b"".join(junk[i % len(junk)] + b"\n" for i in range(k))
            c.append(_case(f"d_extra_lines_{'hdr' if hdr else 'nohdr'}_{k}", REF_S, hdr + b"(1,2)\n(3,1)\nAC(3,40)GT\n" + tail))
    c.append(_case("d_extra_lines_no_last_newline_40", REF_S, b"(1,2)\n(3,1)\nAC(3,40)GT" + b"\n((" * 40))
    c.append(_case("d_first_line_empty", REF_S, b"\n\nACGT(0,9)\n"))
    c.append(_case("d_header_alone", REF_S, b">\n\n\n(0,5)\n"))
    c.append(_case("d_empty_record_line_then_more", REF_S, b">h\n\n\n\n(0,5)\n"))
    for name, rec in (("nl", b"\n"), ("nl_nl", b"\n\n"), ("hdr_nl_nl_nl", b">h\n\n\n"), ("hdr_only", b">h"),
                      ("hdr_two_lines", b">h\n(1,2)\n(3,4)"), ("two_lines", b"(1,2)\n(3,4)\n")):
        c.append(_case("d_missing_line_" + name, REF_S, rec, klass=ERROR, expect=FORMAT))
    # CRLF: stoi("\r") throws on a run line's tail, and ",\r" is not ","
    c.append(_case("d_crlf_full", REF_S, b">h\r\n(2,3)\r\n(4,2)\r\nAC(8,30)T\r\n", klass=ERROR, expect=PARSE))
    c.append(_case("d_crlf_empty_run_lines", REF_S, b"\r\n\r\nAC(8,30)T\r\n", klass=ERROR, expect=PARSE))
    c.append(_case("d_crlf_comma_n_line", REF_N, b"\n,\r\n(0,30)\r\n", klass=ERROR, expect=PARSE))
    return c


def family_e() -> list[Case]:
    c = []
    shapes = {"eleven_digits": (b"(00000000005,3)", b"00000000005"), "leading_blank": (b"( 5,3)", b" 5"),
              "trailing_junk": (b"(5x,3)", b"5x"), "blank_before_comma": (b"(5 ,3)", None), "junk_in_len": (b"(5,3x)", None),
              "twenty_digits": (b"(5,00000000000000000003)", b"00000000000000000005"),
              "thirty_digits": (b"(5,000000000000000000000000000003)", None)}
    for name, (tup, bare) in shapes.items():
        c.append(_case(f"e_{name}_token", REF_S, b"(1,2)\n(3,1)\nAC" + tup + b"GT\n", klass=REJECT_OK))
        c.append(_case(f"e_{name}_lower", REF_S, b"(1,2)" + tup + b"\n(3,1)\nAC(3,40)GT\n", klass=REJECT_OK))
        c.append(_case(f"e_{name}_n", REF_S, b"(1,2)\n(1,1)" + tup + b"\nAC(3,40)GT\n", klass=REJECT_OK))
        if bare:
            c.append(_case(f"e_{name}_bare_lower", REF_S, b"(1,2)," + bare + b",3\n(3,1)\nAC(3,40)GT\n", klass=REJECT_OK))
            c.append(_case(f"e_{name}_bare_n", REF_S, b"\n1," + bare + b"\nAC(3,40)GT\n", klass=REJECT_OK))
    c.append(_case("e_lower_descending", REF_S, b"(10,5)(-5,3)\n\n(0,30)\n", klass=REJECT_OK))
    c.append(_case("e_lower_overlapping", REF_S, b"(5,10)(3,10)\n\n(0,30)\n", klass=REJECT_OK))
    c.append(_case("e_lower_repeated_bare", REF_S, b"4,0,0\n\n(0,30)\n", klass=REJECT_OK))
    # a bare number wider than the staged window, and ones that end at the staged limit exactly
    for line in ("lower", "n"):
        for end in (575, 576, 577, 640, 1088):
            for width in (65, 70, 600):
                if width > end:
                    continue
                text = b"," * (end - width) + b"5".rjust(width, b"0")
                tail = b"" if end % 2 else b",2"
                rec = (text + tail + b"\n(3,1)\n" if line == "lower" else b"(1,2)\n" + text + tail + b"\n") + b"AC(3,40)GT\n"
                c.append(_case(f"e_wide_bare_{line}_{end}_{width}", REF_S, rec, klass=REJECT_OK))
    return c


def family_f() -> list[Case]:
    c = []
    faults = {"double_open": (b"((1,2)", False), "no_close": (b"(1,2", True), "no_comma": (b"(12)", True),
              "empty_delta": (b"(,2)", False), "empty_len": (b"(1,)", False), "empty_tuple": (b"()", True),
              "beyond_int32": (b"(2147483648,1)", False), "len_beyond_int32": (b"(1,99999999999)", False),
              "open_at_last_byte": (b"(", True)}
    for name, (bad, undef) in faults.items():
        c.append(_case(f"f_{name}_token", REF_S, b"(1,2)\n(3,1)\nAC(3,4)GT" + bad, klass=ERROR, expect=PARSE, undefined=undef))
        c.append(_case(f"f_{name}_lower", REF_S, b"(1,2)" + bad + b"\n(3,1)\nAC(3,40)GT\n", klass=ERROR, expect=PARSE, undefined=undef))
        c.append(_case(f"f_{name}_n", REF_S, b"(1,2)\n(3,1)" + bad + b"\nAC(3,40)GT", klass=ERROR, expect=PARSE, undefined=undef))
    # more item starts than a run line of that size can hold runs (every '(' opens an item)
    for n in (64, 513, 3000):
        c.append(_case(f"f_many_opens_lower_{n}", REF_S, b"(" * n + b"1,1\n\nACGT\n", klass=ERROR, expect=PARSE, undefined=True))
        c.append(_case(f"f_many_opens_n_{n}", REF_S, b"\n" + b"(" * n + b"1,1\nACGT\n", klass=ERROR, expect=PARSE, undefined=True))
    # a token one base past |R'|, as the first, a middle and the last token, erased and kept form
    for form, nline, nref in (("erased", b"", len(stripped(REF_N))), ("kept", b",", len(stripped(REF_N, True)))):
        good = b"(0,10)AC(5,%d)" % (nref - 5)
        c.append(_case(f"f_fits_exactly_{form}", REF_N, b"\n" + nline + b"\n" + good + b"GT(-3,3)\n"))
        c.append(_case(f"f_past_end_first_{form}", REF_N, b"\n" + nline + b"\n(1,%d)AC(5,5)(1,1)\n" % nref, klass=ERROR, expect=RANGE))
        c.append(_case(f"f_past_end_middle_{form}", REF_N, b"\n" + nline + b"\n(0,10)AC(5,%d)GT(-3,3)\n" % (nref - 4), klass=ERROR, expect=RANGE))
        c.append(_case(f"f_past_end_last_{form}", REF_N, b"\n" + nline + b"\n(0,10)AC(5,5)(%d,2)" % (nref - 6), klass=ERROR, expect=RANGE))
    # p < 0: the numbers parse, the position is outside the reference -> RANGE (substr throws
    # std::out_of_range at decompression.cpp:230 after the :223 test passed)
    c.append(_case("f_negative_start_first", REF_S, b"\n\n(-1,2)AC\n", klass=ERROR, expect=RANGE))
    c.append(_case("f_negative_start_later", REF_S, b"\n\n(5,3)AC(-6,2)GT(9,1)\n", klass=ERROR, expect=RANGE))
    c.append(_case("f_extreme_token", REF_S, b"\n\n(-2147483648,+2147483647)\n", klass=ERROR, expect=RANGE))
    c.append(_case("f_extreme_len", REF_S, b"\n\n(+0000000000,+2147483647)\n", klass=ERROR, expect=RANGE))
    # two faults: the GPU reports PARSE before RANGE whatever their order in the file
    c.append(_case("f_two_range_then_parse", REF_S, b"\n\n(0,5)(500,3)AC(1x,2)\n", klass=ERROR, expect=PARSE))
    c.append(_case("f_two_range_then_parse_far", REF_S, b"\n\n(500,3)" + b"AC" * 700 + b"(1,2\n", klass=ERROR, expect=PARSE))
    c.append(_case("f_two_parse_then_range", REF_S, b"(x,2)\n\n(0,5)(500,3)\n", klass=ERROR, expect=PARSE))
    c.append(_case("f_two_parse_n_then_range", REF_S, b"\n(3,1)(\n(0,5)(500,3)\n", klass=ERROR, expect=PARSE, undefined=True))
    return c


TWO_FAULT = ("f_two_",)   # names whose oracle class is the first fault in reading order, not `expect`


def cases() -> list[Case]:
    """Every case but the long-line family g, in a fixed order, names unique."""
    out = family_a() + family_b() + family_c() + family_d() + family_e() + family_f()
    assert len({c.name for c in out}) == len(out)
    return out


# ---------------------------------------------------------------------------------------------
# family g: a run line of more than 64 Ki tiles (32 MiB), which takes the scan-based parser
# ---------------------------------------------------------------------------------------------
G_RUNS = 1_400_000
G_REF_BASES = 3_000_000


def long_line_case() -> tuple[bytes, bytes, bytes]:
    """(reference FASTA, record with the long lowercase line, the same with the run lines swapped).
    The long line: 24-byte padded items "(+000000002,+000000001)," with plain "(d,l)" and bare items
    in its first, middle and last KiB; the other run line is short."""
    import numpy as np
    rng = np.random.default_rng(5)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, G_REF_BASES)].tobytes()
    ref = fasta(seq, b">long", 100_000)
    pad = b"(+000000002,+000000001),"
    plain = b"(2,1),2,(2,1)2,2,,(2,0)(2,1),"
    parts = [plain * 30, pad * (G_RUNS // 2), plain * 30, pad * (G_RUNS // 2), plain * 30, b"2,2,(2,1)"]
    long_line = b"".join(parts)
    assert len(long_line) > 32 * 1024 * 1024 + 1024
    short = b"(5,3)(2999000,5),7"
    enc = b"(0,1000000)ACGT(999000,1500000)(-900000,499000)" + b"(+0000000100,+0000001000)" * 3 + b"GT"
    return ref, b">long\n" + long_line + b"\n" + short + b"\n" + enc + b"\n", b">long\n" + short + b"\n" + long_line + b"\n" + enc + b"\n"
