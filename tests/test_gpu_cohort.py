"""Shared reference and cohort fetch on the GPU (sccg_reference_*, sccg_reader_open_shared*,
sccg_cohort_*, sccg.Reference / sccg.Cohort): readers that share one R', and one fetch over many of
them in which every region names its sample.

The truth is never the code under test: a target FASTA body (a synthetic pair's, or one of five
targets made in Python from one reference body by seeded edits) or, for the hand-written records, the
sequence derived from the record format in cohortlib.  Equality with the private reader's and the
per-reader fetches is asserted second."""
import ctypes
import random

import numpy as np
import pytest

import cohortlib
import fetchlib
from cohortlib import ALL_FORMATS, HAND, RFA, RFA_N, check_items, want_items
from fetchlib import split_fasta
from pkg import sccg

pytestmark = pytest.mark.gpu
E = sccg.ERR_CODES


@pytest.fixture(scope="module")
def ctx():
    c = sccg.Context(0)
    yield c
    c.close()


class CohortCase:
    """Five targets over one reference, compressed once: three shared readers (samples 0, 2, 4) and
    two private ones (1, 3), and the cohort over them."""

    def __init__(self, ctx):
        self.rfa, targets = cohortlib.make_cohort_inputs()
        self.kinds = list(cohortlib.KINDS)
        self.tfas = [targets[k][0] for k in self.kinds]
        self.truths = [targets[k][1] for k in self.kinds]
        self.recs = [ctx.compress(self.rfa, t) for t in self.tfas]
        self.ref = ctx.open_reference(self.rfa)
        self.readers = [self.ref.open_reader(r) if i % 2 == 0 else ctx.open_reader(r, self.rfa) for i, r in enumerate(self.recs)]
        self.cohort = sccg.Cohort(self.readers)
        self.lengths = [len(t) for t in self.truths]

    def close(self):
        self.cohort.close()
        for rd in self.readers:
            rd.close()
        self.ref.close()


@pytest.fixture(scope="module")
def case(ctx):
    c = CohortCase(ctx)
    yield c
    c.close()


def status(fn, *a, **k):
    try:
        fn(*a, **k).close()
    except sccg.SccgError as e:
        return e.rc, str(e)
    return 0, ""


# ---------------------------------------------------------------------------------------------
# 1. shared reference, hand-written records
# ---------------------------------------------------------------------------------------------
def exhaustive(L):
    return [(0, L)] + [(i, i + 1) for i in range(L)] + [(i, j) for i in range(L + 1) for j in range(i, min(L, i + 40) + 1)]


def check_shared_against_private(ctx, ref, rfa, rec, truth, what):
    with ref.open_reader(rec) as sh, ctx.open_reader(rec, rfa) as pr:
        L = len(truth)
        assert sh.length == L == pr.length, what
        assert sh.header == pr.header, what
        regions = exhaustive(L)
        got = sh.fetch(regions)
        assert got == [truth[b:e] for b, e in regions], what
        assert got == pr.fetch(regions), what
        assert sh.fetch(regions, upper=True) == [truth[b:e].upper() for b, e in regions], what
        strands = [k & 1 for k in range(len(regions))]
        for enc, dt in (("index", "u8"), ("onehot", "bf16"), ("ascii", "u8")):
            fetchlib.check_encoded(sh, truth, regions, strands, enc, dt, what=what)
            assert sh.fetch_encoded(regions, enc, dt, strand=strands) == pr.fetch_encoded(regions, enc, dt, strand=strands), what
        assert sh.device_bytes < pr.device_bytes, what


def test_shared_reference_hand_written_records(ctx):
    names = sorted(k for k, (rfa, _) in HAND.items() if rfa is RFA)
    assert len(names) == len(HAND) - 1
    with ctx.open_reference(RFA) as ref:
        for name in names:
            rec = HAND[name][1]
            truth = cohortlib.hand_sequence(RFA, rec)
            if name in cohortlib.HAND_SEQ:
                assert truth == cohortlib.HAND_SEQ[name], name
            check_shared_against_private(ctx, ref, RFA, rec, truth, name)


def test_shared_reference_holds_both_forms(ctx):
    comma = HAND["n_line_is_comma"][1]
    assert cohortlib.hand_sequence(RFA_N, comma) == cohortlib.HAND_SEQ["n_line_is_comma"]
    assert cohortlib.hand_sequence(RFA_N, cohortlib.ERASED_REC) == cohortlib.ERASED_SEQ
    assert len(cohortlib.ERASED_N) == 80 and len(cohortlib.KEPT_N) == 120
    with ctx.open_reference(RFA_N) as ref:
        assert ref.device_bytes >= 80 + 120
        check_shared_against_private(ctx, ref, RFA_N, comma, cohortlib.HAND_SEQ["n_line_is_comma"], "kept form")
        check_shared_against_private(ctx, ref, RFA_N, cohortlib.ERASED_REC, cohortlib.ERASED_SEQ, "erased form")
        # a token valid in the 120-base kept form only, in a record that indexes the erased one
        for rc, msg in (status(ref.open_reader, cohortlib.ERASED_REC_BEYOND),
                        status(ctx.open_reader, cohortlib.ERASED_REC_BEYOND, RFA_N)):
            assert rc == E["SCCG_E_RANGE"], msg
        # (the same token under a "," line is inside the kept form)
        with ref.open_reader(b"\n,\n(70,40)") as rd:
            assert rd.fetch([(0, 40)]) == [cohortlib.KEPT_N[70:110]]


def test_shared_reference_without_the_form_a_record_needs(ctx):
    comma = HAND["n_line_is_comma"][1]
    with ctx.open_reference(RFA_N, forms=("erased",)) as ref:
        rc, msg = status(ref.open_reader, comma)
        assert rc == E["SCCG_E_UNSUPPORTED"] and "kept" in msg, msg
        with ref.open_reader(cohortlib.ERASED_REC) as rd:
            assert rd.fetch([(0, rd.length)]) == [cohortlib.ERASED_SEQ]
        one = ref.device_bytes
    with ctx.open_reference(RFA_N, forms=("kept",)) as ref:
        rc, msg = status(ref.open_reader, cohortlib.ERASED_REC)
        assert rc == E["SCCG_E_UNSUPPORTED"] and "erased" in msg, msg
        with ref.open_reader(comma) as rd:
            assert rd.fetch([(0, rd.length)]) == [cohortlib.HAND_SEQ["n_line_is_comma"]]
    with ctx.open_reference(RFA_N) as ref:
        assert ref.device_bytes > one
    with pytest.raises(ValueError):
        ctx.open_reference(RFA_N, forms=("both",))


BAD = [(b"\n\nAC(1x,3)GT", "SCCG_E_PARSE"), (b">h\n\n", "SCCG_E_FORMAT"), (b"\n,\n(0,20)(500,30)", "SCCG_E_RANGE"),
       (b">h\n\n(3,2)\n(0,20)(500,30)", "SCCG_E_RANGE")]


@pytest.mark.parametrize("rec,want", BAD, ids=["malformed", "truncated", "overlong_kept", "overlong_erased"])
def test_shared_open_statuses_are_the_private_open_s(ctx, rec, want):
    with ctx.open_reference(RFA) as ref:
        shared = status(ref.open_reader, rec)
        private = status(ctx.open_reader, rec, RFA)
        assert shared[0] == private[0] == E[want], (shared, private)
        # a truncated record is SCCG_E_FORMAT before the form is looked at
        with ctx.open_reference(RFA, forms=("erased",)) as half:
            assert status(half.open_reader, b">h\n\n")[0] == E["SCCG_E_FORMAT"]
        # the reference still serves a good record afterwards
        with ref.open_reader(HAND["literals_only"][1]) as rd:
            assert rd.fetch([(0, 10)]) == [b"ACGTTGCAAC"]


# ---------------------------------------------------------------------------------------------
# 2. memory
# ---------------------------------------------------------------------------------------------
def test_shared_readers_do_not_hold_the_reference(ctx):
    p = fetchlib.Pair(ctx, "hg", 200_000, 201_000, 3)
    body = split_fasta(p.rfa)[1]
    erased, kept = len(body.replace(b"N", b"")), len(body)
    rp = kept if cohortlib.n_line(p.rec) == b"," else erased
    assert rp > 150_000
    ref = ctx.open_reference(p.rfa)
    assert ref.device_bytes >= erased + kept
    shared = [ref.open_reader(p.rec) for _ in range(3)]
    private = [ctx.open_reader(p.rec, p.rfa) for _ in range(3)]
    try:
        for sh, pr in zip(shared, private):
            assert pr.device_bytes - sh.device_bytes >= rp, (pr.device_bytes, sh.device_bytes, rp)
            assert sh.device_bytes > 0
        assert sum(r.device_bytes for r in shared) + ref.device_bytes < sum(r.device_bytes for r in private)
        rng = random.Random(2)
        regions = [(0, p.length)] + [(b, min(p.length, b + rng.randint(0, 3000))) for b in
                                     (rng.randrange(p.length) for _ in range(100))]
        ref.close()   # the readers hold it
        for rd in shared:
            assert rd.fetch(regions) == [p.truth[b:e] for b, e in regions]
        fetchlib.check_encoded(shared[1], p.truth, regions, [k & 1 for k in range(len(regions))], "onehot", "f16", what="closed ref")
        assert shared[0].fetch(regions) == private[0].fetch(regions)
    finally:
        ref.close()
        for rd in shared + private:
            rd.close()


# ---------------------------------------------------------------------------------------------
# 3. cohort parity
# ---------------------------------------------------------------------------------------------
def test_cohort_inputs(ctx, case):
    """The records reconstruct to their targets and ask for both forms of R'."""
    for tfa, truth, rec in zip(case.tfas, case.truths, case.recs):
        hdr, body = split_fasta(ctx.reconstruct(rec, case.rfa))
        assert (hdr, body) == (tfa.partition(b"\n")[0], truth)
    commas = [cohortlib.n_line(r) == b"," for r in case.recs]
    assert any(commas) and not all(commas), commas
    assert commas[0] and not commas[2] and not commas[4]   # both forms among the shared readers
    assert len(cohortlib._runs(cohortlib.n_line(case.recs[2]))) >= 8
    assert case.cohort.samples == 5
    assert [rd.length for rd in case.readers] == case.lengths
    assert len(set(case.lengths)) > 1


def random_items(case, rng, n, lo, hi):
    out = []
    for _ in range(n):
        s = rng.randrange(5)
        ln = min(rng.randint(lo, hi), case.lengths[s])
        b = rng.randrange(case.lengths[s] - ln + 1)
        out.append((s, b, b + ln, rng.randint(0, 1)))
    return out


@pytest.mark.parametrize("enc,dt", ALL_FORMATS, ids=[f"{e}-{d}" for e, d in ALL_FORMATS])
def test_cohort_parity(case, enc, dt):
    co, T, Ls = case.cohort, case.truths, case.lengths
    rng = random.Random(71)

    def chk(items, what, **k):
        check_items(co, T, items, enc, dt, what=what, **k)

    rnd = random_items(case, rng, 300, 1, 3000)
    chk(rnd, "random")
    # the second assertion: the per-reader encoded fetches of the same regions
    per = b"".join(case.readers[s].fetch_encoded([(b, e)], enc, dt, strand=[r]) for s, b, e, r in rnd[:40])
    assert co.fetch_encoded(rnd[:40], enc, dt) == per
    # a wave's 1,024 and a block's 4,096 bases exactly, the sample changing at the tile's edge
    chk([(0, 5000, 6024, 1), (1, 7000, 11096, 0), (2, 100, 1124, 0), (3, 0, 4096, 1)], "whole tiles")
    # region edges at flat 1023, 1024, 1025 and 4095, 4096, 4097, every edge a change of sample, and
    # regions straddling those multiples
    lens = [1023, 1, 1, 3070, 1, 1, 1, 5000, 1024, 4096]
    assert {1023, 1024, 1025, 4095, 4096, 4097} <= set(np.cumsum(lens).tolist())
    for first in (0, 1):
        items = []
        for k, n in enumerate(lens):
            s = (k + first) % 5
            b = rng.randrange(Ls[s] - n)
            items.append((s, b, b + n, (k + first) & 1))
        chk(items, f"tile edges {first}")
    chk([(4, 31_000, 31_900), (0, 20_000, 20_300), (3, 3_500, 7_000, 1), (2, 24_990, 25_100)], "straddling")
    # many spans with different sources in one wave
    tiny = []
    for k in range(200):
        s = k % 5 if k % 7 else (k + 2) % 5
        ln = rng.randint(1, 5)
        b = rng.randrange(Ls[s] - ln)
        tiny.append((s, b, b + ln, rng.randint(0, 1)))
    chk(tiny, "1-5 bases")
    # runs of empty regions between samples
    items = []
    for s in range(5):
        items += [((s + 1) % 5, 9, 9, k & 1) for k in range(70)] + [(s, 2990 + s, 3100, s & 1)]
    items += [(0, 0, 0)] * 70 + [(1, Ls[1], Ls[1], 1)]
    chk(items, "empties")
    assert co.fetch_encoded([(k % 5, 4, 4, k & 1) for k in range(50)], enc, dt) == b""
    assert co.fetch_encoded([], enc, dt) == b""
    assert co.fetch_encoded([], enc, dt, revcomp=True) == b""
    # the same region from all five samples, a reader twice in a row included
    chk([(s, 9_990, 10_020, s & 1) for s in (0, 1, 2, 3, 4, 4, 0)], "same region")
    chk([(s, 2_000, 8_000) for s in range(5)], "same long region")
    # a region ending at each sample's own length; whole samples
    chk([(s, Ls[s] - 100 - s, Ls[s], (s + 1) & 1) for s in range(5)] + [(s, Ls[s] - 1, Ls[s]) for s in range(5)], "ends")
    chk([(2, 0, Ls[2], 1), (1, 0, Ls[1])], "whole samples")
    # SCCG_FETCH_REVCOMP with and without region flags: every region reversed either way
    chk(rnd[:60], "revcomp + flags", revcomp_all=True)
    chk([it[:3] for it in rnd[:60]], "revcomp", revcomp_all=True)
    if enc == "ascii":
        chk(rnd[:60], "upper", upper=True)


# the smallest lengths that cross a 16-byte piece, a wave's 1,024 bases and a block's 4,096 (the
# encoded reader tests' list)
LENGTHS = [15, 50000, 17, 4097, 4096, 63, 4095, 1, 65, 16, 64]


def test_cohort_of_one_reader_is_that_reader(ctx, case):
    """The two arms of the fetch kernels' shared template against each other: a cohort made of one
    reader alone answers (0, b, e, rev) with the bytes of that reader's fetch_encoded, for every
    format and for origin -- regions of LENGTHS around one position (they change region inside a
    lane), forward, reversed and alternating, with a run of empty regions in the middle."""
    hand_rfa, hand_rec = HAND["lowercase_spanning_n"]
    n_run = next(k for k, c in enumerate(case.truths[2]) if k > 20_000 and c in b"N")   # inside the generated target
    for rfa, rec, c, truth in ((case.rfa, case.recs[2], n_run, case.truths[2]),
                               (hand_rfa, hand_rec, 12, cohortlib.hand_sequence(hand_rfa, hand_rec))):
        with ctx.open_reference(rfa, coords=True) as ref, ref.open_reader(rec) as rd, sccg.Cohort([rd]) as co:
            L = rd.length
            assert L == len(truth) and rd.has_coords
            regions = fetchlib.clamp([(c - n // 3, c - n // 3 + n) for n in LENGTHS], L)
            regions[6:6] = [(c, c)] * 70
            assert sum(e - b for b, e in regions) > min(L, 50_000)
            for strands in ([0] * len(regions), [1] * len(regions), [k & 1 for k in range(len(regions))]):
                items = [(0, b, e, r) for (b, e), r in zip(regions, strands)]
                for enc, dt in ALL_FORMATS + [("origin", "i32")]:
                    want = rd.fetch_encoded(regions, enc, dt, strand=strands)
                    assert co.fetch_encoded(items, enc, dt) == want, (len(rec), strands[:2], enc, dt)
                    if enc == "ascii":
                        assert want == b"".join(fetchlib.strand_bytes(truth, regions, strands)), (len(rec), strands[:2])


@pytest.mark.parametrize("s", range(5), ids=cohortlib.KINDS)
def test_cohort_boundaries_per_sample(case, s):
    """N, case and token boundaries of sample s as region begins and ends, other samples between."""
    bnd = cohortlib.sample_boundaries(case.truths[s], case.recs[s])
    assert bnd["tok_start"] and bnd["tok_end"] and bnd["case"], {k: len(v) for k, v in bnd.items()}
    xs = sorted({x for v in bnd.values() for x in v})
    L = case.lengths[s]
    items = []
    for k, x in enumerate(xs):
        (b, e), = fetchlib.clamp([(x - 17, x + 16)], L)
        items.append((s, b, x, k & 1))
        items.append(((s + 1 + k) % 5, 3000 + k, 3000 + k + (k % 3)))
        items.append((s, x, e, (k + 1) & 1))
    for enc, dt in (("ascii", "u8"), ("index", "u8"), ("onehot", "f16")):
        check_items(case.cohort, case.truths, items, enc, dt, what=cohortlib.KINDS[s])
    long_ = [(s, x, min(L, x + 4097), k & 1) for k, x in enumerate(xs[::6])]
    check_items(case.cohort, case.truths, long_, "index", what=cohortlib.KINDS[s] + " [x, x+4097)")


def test_cohort_device_form(case):
    import torch
    dev = torch.device("cuda", 0)
    co, T, Ls = case.cohort, case.truths, case.lengths
    items = [(3, 5, 5), (2, 20_001, 25_000, 1), (0, 3, 4, 1), (4, Ls[4] - 900, Ls[4]), (1, 0, 37, 1), (2, 24_000, 26_000)]
    G = 64
    for enc, dt, es in (("ascii", "u8", 1), ("index", "u8", 1), ("onehot", "u8", 1), ("onehot", "f16", 2), ("onehot", "f32", 4)):
        want = want_items(T, items, enc, dt)
        assert co.fetch_encoded_device(items, 0, 0, enc, dt) == len(want)   # size query
        for off in (0, 1, 3):   # one element off: the element-wise stores (one-hot), a tile cut at its start
            at = G + off * es
            d_o = torch.full((at + len(want) + G + 16,), 0xAA, dtype=torch.uint8, device=dev)
            assert d_o.data_ptr() % 16 == 0
            n = co.fetch_encoded_device(items, d_o.data_ptr() + at, len(want), enc, dt)
            torch.cuda.synchronize()
            got = d_o.cpu().numpy().tobytes()
            assert n == len(want)
            assert got[at:at + n] == want, (enc, dt, off)
            assert got[:at] == b"\xaa" * at and got[at + n:] == b"\xaa" * (len(got) - at - n), (enc, dt, off)


# ---------------------------------------------------------------------------------------------
# 4. errors
# ---------------------------------------------------------------------------------------------
def test_cohort_errors(ctx, case):
    import torch
    dev = torch.device("cuda", 0)
    co, Ls, lib = case.cohort, case.lengths, case.cohort.lib
    short, long_ = min(range(5), key=lambda s: Ls[s]), max(range(5), key=lambda s: Ls[s])
    assert Ls[short] + 10 < Ls[long_]
    good = (long_, Ls[short], Ls[short] + 10)   # fine in the longer sample
    assert co.fetch_encoded([good], "index") == fetchlib.encode(case.truths[long_][Ls[short]:Ls[short] + 10], "index")
    bads = [((-1, 0, 5), "sample -1"), ((5, 0, 5), "sample 5"), ((short, Ls[short], Ls[short] + 10), f"sample {short}"),
            ((short, Ls[short] - 3, Ls[short] + 1), f"sample {short}"), ((0, -1, 5), "sample 0"), ((0, 9, 8), "sample 0")]
    fmt = sccg.FetchFormat(1, 0, 0, 0)
    for bad, word in bads:
        for items in ([bad], [(0, 0, 10), good, bad, (1, 20, 30), (9, 0, 1)]):
            k = len(items) // 2 if len(items) > 1 else 0
            for enc, dt in (("index", "u8"), ("onehot", "f32")):
                with pytest.raises(sccg.SccgError) as ei:
                    co.fetch_encoded(items, enc, dt)
                assert ei.value.rc == E["SCCG_E_INVALID"]
                assert f"region {k} " in str(ei.value) and word in str(ei.value), str(ei.value)
            # the output is untouched: the host form's buffer, the device form's memory
            rows, arr = co._items(items)
            buf = sccg.Buf()
            assert lib.sccg_cohort_fetch(co.ptr, arr, len(rows), ctypes.byref(fmt), ctypes.byref(buf)) == E["SCCG_E_INVALID"]
            assert not buf.data and buf.len == 0
            d_o = torch.full((4096,), 0xAA, dtype=torch.uint8, device=dev)
            with pytest.raises(sccg.SccgError) as ei:
                co.fetch_encoded_device(items, d_o.data_ptr(), 4096, "index")
            assert ei.value.rc == E["SCCG_E_INVALID"] and f"region {k} " in str(ei.value)
            torch.cuda.synchronize()
            assert bool((d_o == 0xAA).all().item())
    # flag bit 1 (through the C ABI: the Python items only carry bit 0)
    arr = (sccg.CohortRegion * 3)((0, 10, 0, 1), (0, 10, 1, 2), (0, 10, 1, 4))
    buf = sccg.Buf()
    assert lib.sccg_cohort_fetch(co.ptr, arr, 3, ctypes.byref(fmt), ctypes.byref(buf)) == E["SCCG_E_INVALID"]
    assert not buf.data
    msg = lib.sccg_last_error(ctx.ptr).decode()
    assert "region 1 " in msg and "flag" in msg, msg
    # the invalid formats of the encoded fetch
    arr = (sccg.CohortRegion * 1)((0, 10, 0, 0))
    for f in (sccg.FetchFormat(1, 1, 0, 0), sccg.FetchFormat(7, 0, 0, 0), sccg.FetchFormat(1, 0, 8, 0), sccg.FetchFormat(1, 0, 0, 1),
              sccg.FetchFormat(2, 4, 0, 0), sccg.FetchFormat(0, 3, 0, 0)):
        buf = sccg.Buf()
        assert lib.sccg_cohort_fetch(co.ptr, arr, 1, ctypes.byref(f), ctypes.byref(buf)) == E["SCCG_E_INVALID"]
        assert not buf.data
        assert "format" in lib.sccg_last_error(ctx.ptr).decode()
    # an output at an odd byte cannot hold f16 elements
    items = [(0, 5_000, 5_100), (4, 31_000, 31_050, 1)]
    d_o = torch.full((8 * 150 + 128,), 0xAA, dtype=torch.uint8, device=dev)
    with pytest.raises(sccg.SccgError) as ei:
        co.fetch_encoded_device(items, d_o.data_ptr() + 65, 8 * 150, "onehot", "f16")
    assert ei.value.rc == E["SCCG_E_INVALID"]
    # a size query, then one byte short: SCCG_E_NOMEM, the bytes needed, nothing written
    for enc, dt in (("index", "u8"), ("onehot", "f16")):
        need = fetchlib.BPB[(enc, dt)] * 150
        assert co.fetch_encoded_device(items, 0, 0, enc, dt) == need
        with pytest.raises(sccg.SccgError) as ei:
            co.fetch_encoded_device(items, d_o.data_ptr() + 64, need - 1, enc, dt)
        assert ei.value.rc == E["SCCG_E_NOMEM"] and ei.value.needed == need
    torch.cuda.synchronize()
    assert bool((d_o == 0xAA).all().item())


def test_cohort_create_errors(ctx, case):
    lib = ctx.lib
    out = ctypes.c_void_p(0x5A5A)
    ptrs = (ctypes.c_void_p * 2)(case.readers[0].ptr.value, case.readers[1].ptr.value)
    assert lib.sccg_cohort_create(ptrs, 0, ctypes.byref(out)) == E["SCCG_E_INVALID"]   # n_samples == 0
    assert not out.value
    with pytest.raises(ValueError):
        sccg.Cohort([])
    ptrs = (ctypes.c_void_p * 2)(case.readers[0].ptr.value, None)
    out = ctypes.c_void_p(0x5A5A)
    assert lib.sccg_cohort_create(ptrs, 2, ctypes.byref(out)) == E["SCCG_E_INVALID"]
    assert not out.value and "reader 1" in lib.sccg_last_error(ctx.ptr).decode()
    # readers of two contexts
    with sccg.Context(0) as other:
        with other.open_reader(HAND["literals_only"][1], RFA) as foreign:
            with pytest.raises(sccg.SccgError) as ei:
                sccg.Cohort([case.readers[0], case.readers[3], foreign])
            assert ei.value.rc == E["SCCG_E_INVALID"] and "reader 2" in str(ei.value), str(ei.value)
            with sccg.Cohort([foreign, foreign]) as co2:   # a reader twice, on its own context
                assert co2.samples == 2
                assert co2.fetch_encoded([(1, 0, 10), (0, 2, 4, 1)], "ascii") == b"ACGTTGCAAC" + fetchlib.revcomp(b"GT")


# ---------------------------------------------------------------------------------------------
# 5. one launch
# ---------------------------------------------------------------------------------------------
def test_cohort_fetch_is_one_launch(ctx, case):
    rng = random.Random(9)
    many = random_items(case, rng, 1000, 1, 200)
    assert {it[0] for it in many} == set(range(5))
    counts = []
    try:
        for items in ([(3, 1234, 2345, 1)], many):
            ctx.profile(True, families=["fetch"])
            check_items(case.cohort, case.truths, items, "onehot", "f16", what="profiled")
            got = ctx.profile_get()
            assert set(got) == {"fetch"}, got
            counts.append(got["fetch"][1])
    finally:
        ctx.profile(False)
    assert counts == [1, 1], counts


# ---------------------------------------------------------------------------------------------
# 6. fetch_tensor
# ---------------------------------------------------------------------------------------------
def test_cohort_fetch_tensor(case):
    import torch
    co, T = case.cohort, case.truths
    rng = random.Random(41)
    items = [(k % 5, b, b + 257, k & 1) for k, b in enumerate(rng.randrange(50_000) for _ in range(64))]
    for dtype, name in ((torch.uint8, "u8"), (torch.float16, "f16"), (torch.bfloat16, "bf16"), (torch.float32, "f32")):
        t = co.fetch_tensor(items, "onehot", dtype)
        torch.cuda.synchronize()
        assert tuple(t.shape) == (64, 257, 4) and t.dtype == dtype
        assert t.device == torch.device("cuda", 0)
        bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
        assert t.view(bits).cpu().numpy().tobytes() == want_items(T, items, "onehot", name), name
    t = co.fetch_tensor(items)
    assert t.dtype == torch.float16 and tuple(t.shape) == (64, 257, 4)
    t = co.fetch_tensor(items, "index")
    assert tuple(t.shape) == (64, 257) and t.dtype == torch.uint8
    assert t.cpu().numpy().tobytes() == want_items(T, items, "index")
    ragged = [(0, 10, 20), (4, 500, 500), (2, 1000, 1300, 1), (3, 7, 8)]
    t = co.fetch_tensor(ragged, "onehot", torch.float32, revcomp=True)
    assert tuple(t.shape) == (311, 4) and t.dtype == torch.float32
    assert t.view(torch.int32).cpu().numpy().tobytes() == want_items(T, ragged, "onehot", "f32", revcomp_all=True)
    assert tuple(co.fetch_tensor(ragged, "index").shape) == (311,)


# ---------------------------------------------------------------------------------------------
# 7. coexistence
# ---------------------------------------------------------------------------------------------
def test_cohort_survives_other_calls_and_readers_survive_the_cohort(ctx, case):
    rng = random.Random(13)
    items = random_items(case, rng, 120, 1, 2500)
    co = sccg.Cohort(case.readers[::-1])   # a second cohort over the same readers, samples reversed
    mine = [(4 - s, b, e, r) for s, b, e, r in items]
    try:
        check_items(co, case.truths[::-1], mine, "onehot", "u8", what="before")
        rec = ctx.compress(case.rfa, case.tfas[1])
        assert rec == case.recs[1]
        assert split_fasta(ctx.reconstruct(case.recs[4], case.rfa))[1] == case.truths[4]
        for rd, truth in zip(case.readers, case.truths):   # the readers' own fetches in between
            assert rd.fetch([(2_990, 3_050)]) == [truth[2_990:3_050]]
        check_items(co, case.truths[::-1], mine, "onehot", "u8", what="after compress + reconstruct")
        check_items(case.cohort, case.truths, items, "ascii", what="the first cohort")
    finally:
        co.close()
    for s, rd in enumerate(case.readers):
        regions = [(b, e) for k, b, e, _ in items if k == s]
        assert rd.fetch(regions) == [case.truths[s][b:e] for b, e in regions]
    check_items(case.cohort, case.truths, items, "index", what="the first cohort after the second closed")
