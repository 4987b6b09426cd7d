"""GPU parity over arbitrary byte values and multi-header layouts (tests/bytegen.py).

The strip, k-mer key, fetch and formatter kernels classify bytes by bit tricks that are exact by
argument over a FASTA alphabet (case fold by bit 5, a 2-bit code round trip, SWAR range tests, a line's
fate from its first byte carried across lanes, tiles and scan blocks).  Here every byte value a FASTA
body can hold beside the record's token punctuation appears on both sides of a pair, at every word /
lane / tile offset, and '>' lines sit wherever those kernels change state.  The truth is always the
CPU oracle (itself pinned to the compiled reference on the same generators, test_oracle_golden.py),
the compiled reference's fixtures, or fetchlib / originlib -- never the library under test.
"""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bytegen
import fetchlib
import oraclelib
import originlib
from pkg import sccg

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu

# At the match seam bytes are raw: no FASTA, no tokens -- '\n', '(' and digits are bytes like any other.
RAW = bytegen.ALPHABET + bytegen.EXCLUDED


@pytest.fixture(scope="module")
def ctx():
    c = sccg.Context(0)
    yield c
    c.close()


def _check_pair(ctx, rfa, tfa, **overrides):
    """Record and reconstruction against the oracle; returns (record, oracle's mode, stats of the compress)."""
    want = oraclelib.compress_params(rfa, tfa, **overrides) if overrides else oraclelib.compress(rfa, tfa)
    mode = oraclelib.last_mode()[0]
    got = ctx.compress(rfa, tfa, **overrides)
    st = ctx.stats()
    assert got == want
    assert ctx.reconstruct(want, rfa) == oraclelib.decompress(want, rfa)
    return want, mode, st


# ---- match seam ------------------------------------------------------------------------------------------
def _near_copy(rng, sr: bytes, odd_rate: float) -> bytearray:
    """A copy of sr whose odd bytes sometimes change by bit 5 alone (R / r), bit 7 alone (A / 0xc1) or
    to another byte, and whose bases take a few SNPs: k-mers that differ in one odd byte only."""
    st = bytearray(sr)
    for i, c in enumerate(st):
        u = rng.random()
        if c in b"ACGT":
            if u < 0.004:
                st[i] = rng.choice(b"ACGT")
            elif u < 0.006:
                st[i] = c ^ rng.choice([0x20, 0x80])
        elif u < odd_rate:
            st[i] = rng.choice([c ^ 0x20, c ^ 0x80, c ^ 0xA0, rng.choice(RAW)])
    return st


def _odd_seq(rng, n: int, rate: float) -> bytearray:
    s = bytearray(rng.choice(b"ACGT") for _ in range(n))
    for i in range(n):
        if rng.random() < rate:
            s[i] = rng.choice(RAW)
    for i in range(5, n, 37):   # letters and their bit-5 / bit-7 images, always present
        s[i] = rng.choice(b"RrYyNn@`[{A\xc1a\xe1\xdf\xff")
    return s


@pytest.mark.parametrize("n", [13, 200, 999, 1000])
@pytest.mark.parametrize("seed", range(6))
def test_match_seam_local_odd_bytes(ctx, seed, n):
    rng = random.Random(7000 + 10 * seed + n)
    sr = bytes(_odd_seq(rng, n, 0.05))
    st = _near_copy(rng, sr[:rng.randint(n // 2, n)], 0.25)
    st += bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 1000 - len(st))))
    st = bytes(st)
    for k in (14, 10):
        assert ctx.match(sr, st, k, 0, False, 1000 * seed) == oraclelib.match(sr, st, k, 0, False, 1000 * seed)


@pytest.mark.parametrize("k", [14, 14, 14, 17, 21, 32])
@pytest.mark.parametrize("seed", range(2))
def test_match_seam_global_odd_bytes(ctx, seed, k):
    rng = random.Random(7500 + 40 * seed + k)
    n = rng.randint(2000, 40000) if k == 14 else rng.randint(2000, 20000)
    sr = _odd_seq(rng, n, 0.02)
    for _ in range(n // 300):   # repeats that hold odd bytes
        a, b = rng.randrange(n - 40), rng.randrange(n - 40)
        sr[b:b + 33] = sr[a:a + 33]
    sr = bytes(sr)
    st = _near_copy(rng, sr, 0.1)
    cut = rng.randint(0, len(st))
    st = bytes(st[:cut]) + bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 3000))) + bytes(st[cut + rng.choice([0, 50, 300]):])
    assert ctx.match(sr, st, k, 100, True) == oraclelib.match(sr, st, k, 100, True)


# ---- whole pairs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n,kind", [(0, 6000, "local"), (1, 6000, "local"), (2, 6000, "global"),
                                         (3, 30_000, "local"), (4, 30_000, "global")])
def test_odd_pair_full_strips(ctx, seed, n, kind):
    """Fewer than 512 segments: the strips write T, T', R and R'."""
    rfa, tfa = bytegen.odd_pair(seed, n, kind)
    _, mode, st = _check_pair(ctx, rfa, tfa)
    assert mode == (kind == "global")   # (the generator's promise, by the oracle)
    assert st["mode_global"] == int(mode)


@pytest.mark.parametrize("seed,kind", [(5, "local"), (6, "global")])
def test_odd_pair_lean_strips(ctx, seed, kind):
    """600 segments: lean strips, the mode by the switch probe -- a pair that stays local (T and R
    written afterwards) and one that switches."""
    rfa, tfa = bytegen.odd_pair(seed, 600_000, kind)
    _, mode, st = _check_pair(ctx, rfa, tfa)
    assert mode == (kind == "global")
    assert st["mode_global"] == int(mode)


@pytest.mark.parametrize("seed,n", [(7, 30_000), (8, 600_000)])
def test_odd_pair_local0(ctx, seed, n):
    rfa, tfa = bytegen.odd_pair(seed, n, "local")
    _check_pair(ctx, rfa, tfa, local=0)


def test_odd_pair_across_a_scan_block(ctx):
    """4.3 MB: more than 1024 tiles, with a '>' line of the reference and a run of odd bytes of the
    target on the first byte of the second scan block."""
    rfa, tfa = bytegen.scan_edge_pair(0)
    edge = bytegen.SCAN_BLOCK
    assert rfa[:edge].rfind(b"\n>") > edge - 64 and b"\n" not in rfa[edge - 30:edge + 30]   # inside the '>' line
    assert sum(c not in b"ACGTacgt" for c in tfa[edge - 32:edge + 33]) > 55
    _, mode, st = _check_pair(ctx, rfa, tfa)
    assert st["mode_global"] == int(mode)


# ---- one class at every offset -------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["tgt", "ref"])
@pytest.mark.parametrize("cls", list(bytegen.CLASSES), ids=bytegen.slug)
def test_placed_class(ctx, cls, side):
    rfa, tfa = bytegen.placed(cls, side, seed=2)
    _check_pair(ctx, rfa, tfa)


# ---- plain and non-plain tiles ----------------------------------------------------------------------------
def test_tile_mix(ctx):
    rfa, tfa = bytegen.tile_mix(0)
    _check_pair(ctx, rfa, tfa)


KC_CHILD = r"""
import json, sys
sys.path.insert(0, HERE)
import torch
import bytegen
import oraclelib
from pkg import sccg
torch.zeros(1, device=torch.device("cuda", 0))   # torch's HIP runtime before the library context
out = []
with sccg.Context(0) as ctx:
    for rfa, tfa in (bytegen.tile_mix(0), bytegen.odd_pair(20, 30_000, "local"), bytegen.odd_pair(21, 30_000, "global")):
        out.append(ctx.compress(rfa, tfa) == oraclelib.compress(rfa, tfa))
print(json.dumps(out))
"""


def test_tile_mix_and_odd_pairs_without_the_mask_cache():
    """SCCG_STRIP_KC=0 (read once per process: a child): the write pass classifies every tile again
    instead of taking plain tiles' holes from the summary -- the same records."""
    env = dict(os.environ, SCCG_STRIP_KC="0")
    p = subprocess.run([sys.executable, "-c", f"HERE = {HERE!r}\n" + KC_CHILD], env=env, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == [True, True, True]


# ---- reference layouts -------------------------------------------------------------------------------------
def _layout_sequences(kind: str):
    ref, tgt = bytegen.odd_sequences(600 if kind == "local" else 601, 21_000, kind)
    ref[5000:5040] = ord("N")            # the R' -> R map of the origin fetch has something to skip
    ref[9000:9007] = ord("n")
    return ref, tgt


_LAYOUT_SEQ = {kind: _layout_sequences(kind) for kind in ("local", "global")}


def _ref_layout_pair(case: str, kind: str):
    ref, tgt = _LAYOUT_SEQ[kind]
    return bytegen.ref_layout(ref.tobytes(), case), bytegen.to_fasta(tgt, b">t", 70)


@pytest.mark.parametrize("kind", ["local", "global"])
@pytest.mark.parametrize("case", bytegen.REF_LAYOUTS)
def test_ref_layout_pair(ctx, case, kind):
    rfa, tfa = _ref_layout_pair(case, kind)
    _, mode, _ = _check_pair(ctx, rfa, tfa)
    assert mode == (kind == "global")


def _seam_windows(rfa: bytes, length: int):
    out = []
    for s in bytegen.header_seams(rfa):
        for p in (s, s + 5000):   # (the global pair's target is 5000 bases ahead of its reference)
            out += [(p - 40, p), (p, p + 40), (p - 7, p + 9)]
    return fetchlib.clamp(out, length)


@pytest.mark.parametrize("kind", ["local", "global"])
@pytest.mark.parametrize("case", bytegen.REF_LAYOUTS)
def test_ref_layout_reader(ctx, case, kind):
    """A shared reference opened from the layout, a reader over the oracle's record: the whole target
    and windows at every '>' line's neighbours."""
    rfa, tfa = _ref_layout_pair(case, kind)
    rec = oraclelib.compress(rfa, tfa)
    hdr, truth = fetchlib.split_fasta(oraclelib.decompress(rec, rfa))
    with ctx.open_reference(rfa) as ref, ref.open_reader(rec) as rd:
        assert rd.length == len(truth) and rd.header == hdr
        regions = [(0, len(truth))] + _seam_windows(rfa, len(truth))
        assert rd.fetch(regions) == [truth[b:e] for b, e in regions]


@pytest.mark.parametrize("case", bytegen.REF_LAYOUTS)
def test_ref_layout_origin(ctx, case):
    """SCCG_REF_COORDS / "origin" over a global record: a value >= 0 names the byte of the stripped
    reference that the target's base is (both uppercased), -2 sits on an N, and all of it is
    originlib's truth."""
    rfa, tfa = _ref_layout_pair(case, "global")
    rec = oraclelib.compress(rfa, tfa)
    assert oraclelib.last_mode()[0]
    _, truth = fetchlib.split_fasta(oraclelib.decompress(rec, rfa))
    seq, org = originlib.origins(rfa, rec)
    assert seq == truth
    with ctx.open_reference(rfa, coords=True) as ref, ref.open_reader(rec) as rd:
        assert rd.has_coords
        regions = [(0, len(truth))]
        got = originlib.check(rd, org, regions, what=case)
        originlib.check_independent(originlib.ref_sequence(rfa), truth, got, originlib.positions_of(regions), what=case)
        assert (got >= 0).sum() > len(truth) // 2 and (got == originlib.NRUN).any()


# ---- target header layouts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bytegen.TGT_LAYOUTS)
def test_tgt_header_layout(ctx, case):
    ref, tgt = _LAYOUT_SEQ["local" if len(case) % 2 else "global"]
    rfa, tfa = bytegen.to_fasta(ref, b">r", 70), bytegen.tgt_header_layout(tgt.tobytes(), case)
    rec, _, _ = _check_pair(ctx, rfa, tfa)
    hdr = next((ln for ln in tfa.split(b"\n") if ln.startswith(b">")), None)
    if hdr is None:
        assert not rec.startswith(b">")
    else:
        assert rec.split(b"\n", 1)[0] == hdr


# ---- fetch over odd bytes ----------------------------------------------------------------------------------
def _edge_regions(truth: bytes, limit: int = 150):
    """Regions that end on, begin at and straddle every odd byte and every case-run edge."""
    a = np.frombuffer(truth, dtype=np.uint8)
    odd = np.nonzero(~np.isin(a, np.frombuffer(b"ACGTacgt", dtype=np.uint8)))[0]
    low = (a >= ord("a")) & (a <= ord("z"))
    edges = np.nonzero(low[1:] != low[:-1])[0] + 1
    out = []
    for p in [int(x) for x in odd[:limit]] + [int(x) for x in edges[:limit]]:
        out += [(p - 30, p), (p - 30, p + 1), (p, p + 17), (p, p + 1)]
    return fetchlib.clamp(out, len(truth))


def test_fetch_over_odd_bytes(ctx, golden_cases):
    """A reader over a record of the compiled reference whose target holds every kind of byte: ASCII
    on both strands and uppercased, index, one-hot.  fetchlib.COMP complements letters only and
    bytes.upper() is ASCII-only: the contract of the fetch kernels' complement, fold and base code."""
    c = next(c for c in golden_cases if c["name"] == "bytes_global_00")
    hdr, truth = fetchlib.split_fasta(c["fasta"])
    assert len(set(truth)) > 150
    regions = [(0, len(truth))] + _edge_regions(truth)
    strands = [i % 2 for i in range(len(regions))]
    with ctx.open_reader(c["record"], c["ref_fa"]) as rd:
        assert rd.length == len(truth) and rd.header == hdr
        assert rd.fetch(regions) == [truth[b:e] for b, e in regions]
        assert rd.fetch(regions, upper=True) == [truth[b:e].upper() for b, e in regions]
        for upper in (False, True):
            fetchlib.check_encoded(rd, truth, regions, None, "ascii", upper=upper, what="forward")
            fetchlib.check_encoded(rd, truth, regions, strands, "ascii", upper=upper, what="strands")
            fetchlib.check_encoded(rd, truth, regions, None, "ascii", revcomp_all=True, upper=upper, what="revcomp")
        for enc, dt in (("index", "u8"), ("onehot", "u8"), ("onehot", "f16")):
            fetchlib.check_encoded(rd, truth, regions, strands, enc, dt, what="strands")
            fetchlib.check_encoded(rd, truth, regions, None, enc, dt, revcomp_all=True, what="revcomp")


# ---- hand-built records --------------------------------------------------------------------------------------
def _hand_record(variant: str):
    rng = random.Random(31)
    ref = "".join(rng.choice("ACGT") for _ in range(3000))
    rfa = bytegen.to_fasta(ref.encode(), b">r", 60)
    alpha = bytegen.ALPHABET
    enc = b"(0,40)" + alpha + b"(100,33)" + alpha[::-1] + b"(7,64)" + alpha[::3] + b"GATTACA" + alpha[1::2] + b"(500,200)"
    dec_len = 40 + 33 + 64 + 200 + len(alpha) * 2 + len(alpha[::3]) + 7 + len(alpha[1::2])
    if variant == "lower_all":          # tolower meets every byte value
        return rfa, b"(0,%d)\n\n%s" % (dec_len, enc)
    if variant == "lower_and_n_runs":   # lowercase runs at odd offsets, N runs cut through the literals
        lower = b"(3,60)(100,1)(2,2)(5,3)(30,150)(200,97)"
        nline = b"(45,5)(20,1)(1,1)(60,64)(100,3)(150,65)"
        return rfa, lower + b"\n" + nline + b"\n" + enc
    if variant == "header_kept_form":   # a header, the N line ",": nothing erased from the reference
        return rfa, b">hand \x80\xc1\n(1,%d)\n,\n%s" % (dec_len - 2, enc)
    raise ValueError(variant)


@pytest.mark.parametrize("variant", ["lower_all", "lower_and_n_runs", "header_kept_form"])
def test_hand_records_over_every_byte(ctx, variant):
    """Record lines built by hand whose literals run through all of ALPHABET under lowercase runs
    ('@' '[' '`' '{' 0xc1 must not fold) and N runs, through the formatter and through a reader."""
    rfa, rec = _hand_record(variant)
    want = oraclelib.decompress(rec, rfa)
    assert ctx.reconstruct(rec, rfa) == want
    hdr, truth = fetchlib.split_fasta(want)
    with ctx.open_reader(rec, rfa) as rd:
        assert rd.header == hdr
        assert rd.fetch([(0, len(truth))]) == [truth]
        regions = [(0, len(truth))] + _edge_regions(truth, 60)
        fetchlib.check_encoded(rd, truth, regions, [i % 2 for i in range(len(regions))], "ascii", what=variant)
        fetchlib.check_encoded(rd, truth, regions, None, "index", what=variant)
