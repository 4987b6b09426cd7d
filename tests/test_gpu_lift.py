"""Lift on the GPU (sccg_reader_lift*, sccg_cohort_lift*): intervals of the reference onto a sample,
run-length coded.

The truth is never the code under test (liftlib): the numpy run-length coding of locatelib's per-position
inverse.  Two more truths need no oracle and are asserted on the GPU's own outputs: the blocks expanded per
base are what locate returns for the same positions, and the origin fetch of a block's sequence stretch is
the block's reference stretch.  Every check also asserts that the blocks tile each interval and that no two
neighbours could merge."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import cohortlib
import fetchlib
import liftlib
import locatelib
import originlib
import segmentslib
from cohortlib import HAND, RFA_N
from locatelib import fasta, random_body, record
from pkg import sccg

pytestmark = pytest.mark.gpu
E = sccg.ERR_CODES
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FETCH = os.path.join(REPO, "sccg-genome-compression_amd", "bin", "fetch")
WORKED_WHOLE = [(0, 4, 0), (4, 4, -2), (8, 8, 8), (16, 4, -2), (20, 8, 16), (28, 4, -2), (32, 8, 24), (40, 4, -2), (44, 2, 32),
                (46, 6, -1), (52, 4, -2), (56, 4, -1), (60, 4, 38), (64, 4, -2), (68, 6, 42), (74, 2, -1), (76, 4, -2), (80, 8, -1),
                (88, 4, -2), (92, 8, -1), (100, 4, -2), (104, 8, -1), (112, 4, -2), (116, 4, -1)]
WORKED_2_70 = [(2, 2, 2)] + WORKED_WHOLE[1:14] + [(68, 2, 42)]


@pytest.fixture(scope="module")
def ctx():
    c = sccg.Context(0)
    yield c
    c.close()


def rows(blk):
    return [tuple(r) for r in blk.tolist()]


class Pair:
    """A reader with locating enabled over (rfa, rec) and the oracle's pos per reference position."""

    def __init__(self, ctx, rfa, rec, private=False):
        self.pos = locatelib.inverse(rfa, rec)[0]
        self.nR = len(self.pos)
        self.ref = None if private else ctx.open_reference(rfa, coords=True)
        self.rd = ctx.open_reader(rec, rfa) if private else self.ref.open_reader(rec)
        self.rd.enable_locate()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.rd.close()
        if self.ref is not None:
            self.ref.close()

    def check(self, intervals, what, free=True):
        return liftlib.check(self.rd, self.pos, intervals, what, free)

    def whole(self, what):
        return rows(self.check([(0, self.nR)], what + " whole")[1])

    def every_pair(self, what, L=120):
        """Every (begin, end) pair of the first L reference bases in ONE call."""
        return self.check(liftlib.every_pair(min(self.nR, L)), what + " every pair")


# ---------------------------------------------------------------------------------------------
# 1. hand-written records; the worked example
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND) + ["erased_rec"])
def test_hand_written_records(ctx, name):
    rfa, rec = (RFA_N, cohortlib.ERASED_REC) if name == "erased_rec" else HAND[name]
    modes = [False] + ([True] if cohortlib.n_line(rec) == b"," else [])   # (a private reader of an erased form has no coordinates)
    for private in modes:
        with Pair(ctx, rfa, rec, private) as p:
            what = f"{name} private={private}"
            whole = p.whole(what)
            p.every_pair(what)
            if p.nR > 120:
                p.check([(p.nR - 120 + b, p.nR - e) for b in range(0, 120, 7) for e in range(0, 120 - b, 5)], what + " tail pairs")
            if name == "erased_rec":
                assert whole == WORKED_WHOLE
                off, blk = p.rd.lift([(0, 120), (2, 70)])
                assert off.tolist() == [0, 24, 39] and rows(blk[24:]) == WORKED_2_70
            if name == "literals_only":   # no token at all: no index is allocated
                assert all(r[2] < 0 for r in whole) and len(whole) >= 1
            if cohortlib.n_line(rec) == b",":
                assert all(r[2] != -2 for r in whole)


# ---------------------------------------------------------------------------------------------
# 2. continuity across elementary intervals: the definition speaks of bases, not of tokens
# ---------------------------------------------------------------------------------------------
BODY600 = random_body(600, 17)
CONTINUITY = {
    # items, the interval asked, its blocks
    "touching": ([(100, 30), (130, 20)], (100, 150), [(100, 50, 0)]),
    "literal_between": ([(100, 30), b"G", (130, 20)], (100, 150), [(100, 30, 0), (130, 20, 31)]),
    "zero_between": ([(100, 30), (500, 0), (7, 0), (130, 20)], (100, 150), [(100, 50, 0)]),
    "nested_later": ([(300, 50), b"AC", (310, 10), (310, 10), (320, 1)], (300, 350), [(300, 50, 0)]),
    "nested_later_wider": ([(300, 50), b"AC", (310, 10), (310, 10), (320, 1)], (290, 360), [(290, 10, -1), (300, 50, 0), (350, 10, -1)]),
    # the first token ends inside a later, longer one: a cut at its end
    "first_ends_inside_later": ([(100, 20), b"T", (90, 60)], (90, 150), [(90, 10, 21), (100, 20, 0), (120, 30, 51)]),
    "gap_of_one": ([(100, 30), (131, 20)], (100, 151), [(100, 30, 0), (130, 1, -1), (131, 20, 30)]),
    "overlap_of_one": ([(100, 30), (129, 20)], (100, 149), [(100, 30, 0), (130, 19, 31)]),
    "backwards": ([(100, 30), (50, 20)], (50, 130), [(50, 20, 30), (70, 30, -1), (100, 30, 0)]),
}


@pytest.mark.parametrize("name", sorted(CONTINUITY))
def test_continuity(ctx, name):
    items, (b, e), want = CONTINUITY[name]
    with Pair(ctx, fasta(BODY600), record(items)) as p:
        off, blk = p.check([(b, e), (0, 600), (b + 1, e - 1), (b, b + 1), (e - 1, e)], name)
        assert rows(blk[:off[1]]) == want, name
        p.check(liftlib.every_pair(170)[::3] + [(x, y) for x in range(280, 370, 3) for y in range(x, 370, 2)], name + " pairs")


def test_overlap_record_order_wins(ctx):
    items = [(120, 30), b"T", (100, 30), (110, 25), b"GG", (300, 50), (310, 10), (310, 10), (300, 50), (320, 1),
             (400, 10), (410, 10), (390, 10), (0, 5), (595, 5)]
    with Pair(ctx, fasta(random_body(600, 3)), record(items)) as p:
        whole = p.whole("overlap")
        # (120,30) is the record's first token, (100,30) covers 100..119 first; (400,10)(410,10) go on, (390,10) comes later
        assert (100, 20, 31) in whole and (120, 30, 0) in whole and (300, 50, 88) in whole
        assert any(r[0] == 390 and r[1] == 10 for r in whole) and any(r[0] == 400 and r[1] == 20 for r in whole)
        p.check([(x, y) for x in range(95, 155) for y in range(x, 155)] + [(x, y) for x in range(385, 425) for y in range(x, 425)], "overlap pairs")


# ---------------------------------------------------------------------------------------------
# 3. N runs of the reference and of the target
# ---------------------------------------------------------------------------------------------
def n_reference(seed=1):
    """test_gpu_locate.n_reference, restated: runs of N at both ends, single, with a lowercase n among them."""
    b = random_body
    body = b"NNN" + b(50, seed) + b"NNNN" + b(30, seed + 1) + b"n" + b(20, seed + 2) + b"N" + b(40, seed + 3) + b"NnN" + b(25, seed + 4) + b"NN"
    return fasta(body), body


@pytest.mark.parametrize("rfa_kind", ["rfa_n", "variant"])
def test_reference_and_target_n_runs(ctx, rfa_kind):
    variant = rfa_kind == "variant"
    rfa, body = n_reference() if variant else (RFA_N, cohortlib.KEPT_N)
    nRp = len(body) - body.count(b"N")
    # the erased form; target N runs before, between and behind the tokens; the third token covers the variant's 'n'
    toks = [(0, 30), b"AC", (nRp - 40, 40), (76 if variant else 20, 12)]
    rec = record(toks, lower=b"(3,9)", nline=b"(0,2)(30,4)(%d,3)" % (84 + 6 - 30))
    R = originlib.ref_sequence(rfa)
    runs = [(m.start(), m.end()) for m in re.finditer(rb"N+", R)]
    with Pair(ctx, rfa, rec) as p:
        whole = p.whole(rfa_kind)
        p.every_pair(rfa_kind, L=len(R))   # every begin and end: inside, at the first and at the last base of every run
        assert [r[:2] for r in whole if r[2] == -2] == [(a, e - a) for a, e in runs]
        for a, e in runs:
            asked = [(a, e), (a, a + 1), (e - 1, e)] + ([(a - 1, a)] if a else []) + ([(e, e + 1)] if e < len(R) else [])
            off, blk = p.check(asked, f"{rfa_kind} run [{a}, {e})")
            assert rows(blk[:3]) == [(a, e - a, -2), (a, 1, -2), (e - 1, 1, -2)]
            assert all(r[2] != -2 and r[1] == 1 for r in rows(blk[3:]))
        if variant:
            low = R.index(b"n")
            assert rows(p.rd.lift([(low, low + 1)])[1])[0][2] >= 0   # a lowercase n is a base of R'
    # erased runs exactly at tokens' R' boundaries: RFA_N's R' 4 lies behind the run at R 4..7, R' 12 behind the one at 16..19
    with Pair(ctx, RFA_N, record([(0, 4), (4, 8), b"T", (12, 4)], nline=b"")) as p:
        assert p.whole("run at a token boundary")[:5] == [(0, 4, 0), (4, 4, -2), (8, 8, 4), (16, 4, -2), (20, 4, 13)]
        p.every_pair("run at a token boundary")
    # the kept form over the same references: no -2 block, an N is a base like any other
    kept = record([(0, 30), b"AC", (len(R) - 40, 40), (2, 12)], nline=b",")
    for private in (False, True):
        with Pair(ctx, rfa, kept, private) as p:
            assert all(r[2] != -2 for r in p.whole(f"{rfa_kind} kept private={private}"))
            p.every_pair(f"{rfa_kind} kept private={private}", L=len(R))


def test_target_n_runs(ctx):
    rfa = fasta(BODY600)
    cases = {
        "inside_a_token": ([(100, 30)], b"(10,5)", [(100, 10, 0), (110, 20, 15)]),
        "at_a_junction": ([(100, 30), (130, 20)], b"(30,3)", [(100, 30, 0), (130, 20, 33)]),
        "before_and_behind": ([(100, 30), (130, 20)], b"(0,2)(52,3)", [(100, 50, 2)]),
        "two_touching_inside": ([(100, 30)], b"(10,2)(2,3)", [(100, 10, 0), (110, 20, 15)]),
        "between_literal_and_token": ([b"ACGT", (100, 30)], b"(4,2)", [(100, 30, 6)]),
        "inside_a_later_token_only": ([(100, 30), b"T", (100, 30)], b"(41,2)", [(100, 30, 0)]),
    }
    for name, (items, nline, want) in cases.items():
        with Pair(ctx, rfa, record(items, nline=nline)) as p:
            off, blk = p.check([(100, 150 if len(items) > 1 and items[-1] == (130, 20) else 130)], name)
            assert rows(blk) == want, name
            p.check([(x, y) for x in range(95, 155, 2) for y in range(x, 156)], name + " pairs")


# ---------------------------------------------------------------------------------------------
# 4. index sizes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,zero_every", [(1, 0), (2, 1), (64, 0), (65, 3), (3000, 7)])
def test_token_counts(ctx, k, zero_every):
    nR = 1500 if k < 100 else 20_000
    rfa = fasta(random_body(nR, 40 + k))
    rec = segmentslib.token_record(nR, k, 7 * k + zero_every, zero_every)
    with Pair(ctx, rfa, rec) as p:
        what = f"{k} tokens"
        whole = p.whole(what)
        assert any(r[2] >= 0 for r in whole)
        if k >= 3000:
            assert len(whole) > 1000 and any(r[2] == -1 for r in whole)   # (later tokens hide behind earlier ones)
        p.check(liftlib.random_regions(nR, 3000, 200, 9 + k), what + " 3,000 intervals")
        for n in (0, 1, 63, 64, 65):
            iv = liftlib.random_regions(nR, n, 200, 50 + n)
            if n > 3:
                iv[1] = (iv[0][0], iv[0][0])   # empty
                iv[2] = iv[0]                  # repeated
                iv[3] = (max(iv[0][0] - 5, 0), iv[0][1])   # overlapping
                iv[-1] = (nR, nR)              # empty at the end
            off, blk = p.check(iv, f"{what} n={n}")
            if n == 0:
                assert off.tolist() == [0] and blk.shape == (0, 3)
        p.check(sorted(liftlib.random_regions(nR, 200, 200, 77), reverse=True), what + " descending")
        off, blk = p.check([(5, 5), (0, 0), (nR, nR)], what + " only empty intervals")
        assert off.tolist() == [0, 0, 0, 0] and len(blk) == 0


# ---------------------------------------------------------------------------------------------
# 5. pile-up
# ---------------------------------------------------------------------------------------------
def test_pile_up(ctx):
    """test_gpu_locate.test_pile_up's record: 4,500 short tokens on one window of 64 bases."""
    rng = random.Random(4)
    toks = [(700 + rng.randrange(60), rng.randint(1, 4)) for _ in range(4500)]
    items = [(10, 50), b"AC"]
    for k, t in enumerate(toks):
        items.append(t)
        if k % 97 == 0:
            items.append(b"T")
    with Pair(ctx, fasta(random_body(2000, 9)), record(items + [(1500, 100)])) as p:
        off, blk = p.check([(700, 764), (0, 2000)] + [(r, r + 1) for r in range(695, 770)], "pile-up")
        assert off[1] >= 10 and rows(blk[off[1]:off[2]])[:2] == [(0, 10, -1), (10, 50, 0)]


# ---------------------------------------------------------------------------------------------
# 6. cross-check with segments
# ---------------------------------------------------------------------------------------------
def test_lift_is_segments_transposed(ctx):
    """Tokens over disjoint reference intervals: every copied base has one copy, so the maximal diagonal
    runs seen from the reference are those seen from the sequence."""
    rng = random.Random(21)
    nR, at, toks = 6000, 3, []
    while at < nR - 60:
        l = rng.randint(1, 50)
        toks.append((at, l))
        at += l + rng.choice([0, 0, 1, 2, 9])   # touching, or a deleted stretch
    order = list(range(len(toks)))
    for k in range(0, len(order) - 8, 8):   # blocks of eight tokens swapped: rearrangements
        if rng.random() < 0.3:
            order[k:k + 4], order[k + 4:k + 8] = order[k + 4:k + 8], order[k:k + 4]
    items = []
    for k in order:
        items.append(toks[k])
        if rng.random() < 0.2:
            items.append(bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 3))))
    rfa, rec = fasta(random_body(nR, 77)), record(items, nline=b"(40,3)(500,2)(2,6)(900,1)")
    pos, copies = locatelib.inverse(rfa, rec)
    assert copies.max() == 1
    seq, org = originlib.origins(rfa, rec)
    with Pair(ctx, rfa, rec) as p:
        blk = p.check([(0, nR)], "disjoint tokens")[1]
        seg = segmentslib.check(p.rd, org, [(0, len(org))], what="disjoint tokens")[1]
        lifted = {(r, l, q) for r, l, q in rows(blk) if q >= 0}
        aligned = {(r, l, q) for q, l, r in rows(seg) if r >= 0}
        assert lifted == aligned and len(lifted) > 50


# ---------------------------------------------------------------------------------------------
# 7. eight samples over one shared reference (test_gpu_locate.LocateCohort, built the same way)
# ---------------------------------------------------------------------------------------------
class LiftCohort:
    def __init__(self, ctx):
        self.rfa, targets = cohortlib.make_cohort_inputs()
        body = fetchlib.split_fasta(self.rfa)[1]
        bodies = [targets[k][1] for k in cohortlib.KINDS]
        bodies += [cohortlib.make_target(body, kind, seed) for kind, seed in (("indel", 201), ("nruns", 202), ("block", 203))]
        self.truths = bodies
        self.recs = [ctx.compress(self.rfa, cohortlib.wrap60(b"s%d" % i, b)) for i, b in enumerate(bodies)]
        self.inv = [locatelib.inverse(self.rfa, r) for r in self.recs]
        self.pos = [w[0] for w in self.inv]
        self.nR = len(self.pos[0])
        self.ref = ctx.open_reference(self.rfa, coords=True)
        self.private = [i % 2 == 1 and cohortlib.n_line(r) == b"," for i, r in enumerate(self.recs)]
        self.readers = [ctx.open_reader(r, self.rfa) if pv else self.ref.open_reader(r) for pv, r in zip(self.private, self.recs)]
        self.late = self.ref.open_reader(self.recs[0])   # sample 8: joins the cohort before it enables locating
        for rd in self.readers:
            rd.enable_locate()
        self.cohort = sccg.Cohort(self.readers + [self.late])
        self.late.enable_locate()

    def close(self):
        self.cohort.close()
        self.late.close()
        for rd in self.readers:
            rd.close()
        self.ref.close()


@pytest.fixture(scope="module")
def case(ctx):
    c = LiftCohort(ctx)
    yield c
    c.close()


def cohort_items(case, n, hi, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        ln = rng.randint(0, hi)
        b = rng.randrange(case.nR - ln + 1)
        out.append((rng.randrange(8), b, b + ln))
    return out


def test_cohort_lift(ctx, case):
    assert any(case.private) and not all(case.private), case.private   # private kept-form and shared readers mixed
    assert any(cohortlib.n_line(r) != b"," for r in case.recs)
    items = cohort_items(case, 5000, 300, 1)
    off, blk = liftlib.check_cohort(case.cohort, case.pos, items, case.readers, "cohort")
    assert (blk[:, 2] >= 0).any() and (blk[:, 2] == -1).any()
    for s in range(8):   # the readers' own answers are the cohort's
        idx = [k for k, it in enumerate(items) if it[0] == s]
        roff, rblk = case.readers[s].lift([items[k][1:] for k in idx])
        assert np.array_equal(rblk, np.concatenate([blk[off[k]:off[k + 1]] for k in idx])), s
        assert np.array_equal(np.diff(roff), np.array([off[k + 1] - off[k] for k in idx])), s
    for n in (0, 1, 63, 64, 65):
        liftlib.check_cohort(case.cohort, case.pos, cohort_items(case, n, 300, 10 + n), None, f"cohort n={n}")
    whole = [(s, 0, case.nR) for s in (7, 2, 0, 5)]   # whole references, one of them an N-run sample
    off, blk = liftlib.check_cohort(case.cohort, case.pos, whole, None, "cohort whole references")
    assert len(blk) > 100
    expect("SCCG_E_UNSUPPORTED", "interval 1", lambda: case.cohort.lift([(0, 0, 5), (8, 0, 5), (0, 0, case.nR + 1)]))
    assert case.late.can_locate and rows(case.late.lift([(0, 500)])[1]) == rows(case.readers[0].lift([(0, 500)])[1])


# ---------------------------------------------------------------------------------------------
# 8. tensor and device forms
# ---------------------------------------------------------------------------------------------
def test_lift_tensor(case):
    import torch
    rd = case.readers[2]
    iv = liftlib.random_regions(case.nR, 100, 500, 3) + [(7, 7)]
    eoff, eblk = liftlib.want(case.pos[2], iv)
    off, blk = rd.lift_tensor(iv)
    assert off.dtype == torch.int64 and blk.dtype == torch.int64 and off.device == torch.device("cuda", 0) and blk.is_cuda
    assert off.cpu().tolist() == eoff.tolist() and np.array_equal(blk.cpu().numpy(), eblk)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        off, blk = rd.lift_tensor(iv, stream=s)
    assert np.array_equal(blk.cpu().numpy(), eblk)
    items = cohort_items(case, 100, 500, 4)
    eoff, eblk = liftlib.want(case.pos, items)
    off, blk = case.cohort.lift_tensor(items)
    assert off.cpu().tolist() == eoff.tolist() and np.array_equal(blk.cpu().numpy(), eblk)
    off, blk = rd.lift_tensor([])
    assert off.cpu().tolist() == [0] and tuple(blk.shape) == (0, 3)


def test_size_query_capacity_alignment(case):
    import torch
    dev = torch.device("cuda", 0)
    lib, rd, co = case.readers[0].lib, case.readers[0], case.cohort
    iv = [(5, 5), (100, 9000), (3, 4), (50_000, case.nR)]
    eoff, eblk = liftlib.want(case.pos[0], iv)
    need = len(eblk)
    assert need >= 4
    arr = (sccg.Region * len(iv))(*iv)
    items = (sccg.CohortRegion * len(iv))(*[(b, e, 0, 0) for b, e in iv])
    n = ctypes.c_size_t(0)
    for call, ptr, a in ((lib.sccg_reader_lift_device, rd.ptr, arr), (lib.sccg_cohort_lift_device, co.ptr, items)):
        d_off = torch.full((len(iv) + 1 + 4,), 77, dtype=torch.int64, device=dev)
        d_blk = torch.full((need + 4, 3), 77, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        n.value = 0
        assert call(ptr, a, len(iv), None, None, 0, ctypes.byref(n), None) == 0 and n.value == need   # size query
        assert call(ptr, a, len(iv), d_off.data_ptr(), None, 0, ctypes.byref(n), None) == 0 and n.value == need
        torch.cuda.synchronize()
        assert bool((d_off == 77).all().item())   # a size query writes nothing
        n.value = 0
        assert call(ptr, a, len(iv), d_off.data_ptr(), d_blk.data_ptr(), need - 1, ctypes.byref(n), None) == E["SCCG_E_NOMEM"]
        assert n.value == need and str(need) in lib.sccg_last_error(rd.ctx.ptr).decode()
        assert call(ptr, a, len(iv), d_off.data_ptr() + 4, d_blk.data_ptr(), need, ctypes.byref(n), None) == E["SCCG_E_INVALID"]
        assert "d_off" in lib.sccg_last_error(rd.ctx.ptr).decode()
        assert call(ptr, a, len(iv), d_off.data_ptr(), d_blk.data_ptr() + 4, need, ctypes.byref(n), None) == E["SCCG_E_INVALID"]
        assert "d_blk" in lib.sccg_last_error(rd.ctx.ptr).decode()
        d_off.fill_(77)
        d_blk.fill_(77)
        torch.cuda.synchronize()   # (the fills run on torch's stream, the call on the context's own, which does not wait for it)
        assert call(ptr, a, len(iv), d_off.data_ptr(), d_blk.data_ptr(), need, ctypes.byref(n), None) == 0 and n.value == need   # exact
        assert d_off.cpu().tolist() == eoff.tolist() + [77] * 4
        assert np.array_equal(d_blk.cpu().numpy()[:need], eblk) and bool((d_blk[need:] == 77).all().item())
        d_blk.fill_(77)   # without offsets
        torch.cuda.synchronize()
        assert call(ptr, a, len(iv), None, d_blk.data_ptr(), need + 4, ctypes.byref(n), None) == 0 and n.value == need
        assert np.array_equal(d_blk.cpu().numpy()[:need], eblk) and bool((d_blk[need:] == 77).all().item())


# ---------------------------------------------------------------------------------------------
# 9. errors write nothing
# ---------------------------------------------------------------------------------------------
def expect(rc_name, text, call):
    with pytest.raises(sccg.SccgError) as ei:
        call()
    assert ei.value.rc == E[rc_name] and text in str(ei.value), str(ei.value)


def test_errors_write_nothing(ctx, case):
    import torch
    dev = torch.device("cuda", 0)
    rd, co, nR = case.readers[0], case.cohort, case.nR
    lib = rd.lib
    I, U = E["SCCG_E_INVALID"], E["SCCG_E_UNSUPPORTED"]
    hoff = (ctypes.c_int64 * 4)(*[77] * 4)
    buf = sccg.Buf()
    n = ctypes.c_size_t(77)
    d_off = torch.full((8,), 77, dtype=torch.int64, device=dev)
    d_blk = torch.full((64, 3), 77, dtype=torch.int64, device=dev)
    ok = (sccg.Region * 2)((0, 10), (5, 9))
    # a reader that has not enabled locating: the size query and the empty list too
    with case.ref.open_reader(case.recs[0]) as fresh:
        expect("SCCG_E_UNSUPPORTED", "enable", lambda: fresh.lift([(0, 10)]))
        expect("SCCG_E_UNSUPPORTED", "enable", lambda: fresh.lift([]))
        expect("SCCG_E_UNSUPPORTED", "enable", lambda: fresh.lift_tensor([(0, 10)]))
        assert lib.sccg_reader_lift_device(fresh.ptr, ok, 2, None, None, 0, ctypes.byref(n), None) == U   # size query
        assert lib.sccg_reader_lift_device(fresh.ptr, ok, 2, d_off.data_ptr(), d_blk.data_ptr(), 64, ctypes.byref(n), None) == U
        assert lib.sccg_reader_lift(fresh.ptr, ok, 2, hoff, ctypes.byref(buf)) == U
    # bad intervals, flags, samples: the first offender is named
    expect("SCCG_E_INVALID", "interval 1", lambda: rd.lift([(0, 5), (5, nR + 1), (-1, 3)]))
    expect("SCCG_E_INVALID", "interval 0", lambda: rd.lift([(-1, 3)]))
    expect("SCCG_E_INVALID", "interval 2", lambda: rd.lift([(0, 5), (5, 5), (9, 8)]))
    expect("SCCG_E_INVALID", "interval 1", lambda: co.lift([(0, 0, 5), (1, 0, 5, True)]))   # flag bit 0
    expect("SCCG_E_INVALID", "flag", lambda: co.lift([(1, 0, 5, True)]))
    expect("SCCG_E_INVALID", "sample 9", lambda: co.lift([(0, 0, 5), (9, 0, 5)]))
    expect("SCCG_E_INVALID", "sample -1", lambda: co.lift([(-1, 0, 5)]))
    expect("SCCG_E_INVALID", "interval 1", lambda: co.lift([(0, 0, 5), (3, 0, nR + 1)]))
    expect("SCCG_E_INVALID", "interval 1", lambda: co.lift_tensor([(0, 0, 5), (1, 0, 5, True)]))
    # sample 8 had not enabled locating when the cohort was created; the first offender in list order decides
    expect("SCCG_E_UNSUPPORTED", "interval 1", lambda: co.lift([(0, 0, 5), (8, 0, 5), (0, 0, nR + 1)]))
    expect("SCCG_E_INVALID", "interval 0", lambda: co.lift([(0, 0, nR + 1), (8, 0, 5)]))
    expect("SCCG_E_UNSUPPORTED", "sample 8", lambda: co.lift_tensor([(8, 0, 5)]))
    # raw calls over sentinel-filled outputs
    bad_r = (sccg.Region * 2)((0, 10), (5, nR + 1))
    flag2 = (sccg.CohortRegion * 2)((0, 5, 0, 0), (0, 5, 1, 2))
    flag1 = (sccg.CohortRegion * 2)((0, 5, 0, 0), (0, 5, 1, 1))
    badsample = (sccg.CohortRegion * 2)((0, 5, 0, 0), (0, 5, 9, 0))
    badrange = (sccg.CohortRegion * 2)((0, 5, 0, 0), (6, 5, 1, 0))
    late = (sccg.CohortRegion * 2)((0, 5, 0, 0), (0, 5, 8, 0))
    assert lib.sccg_reader_lift(rd.ptr, bad_r, 2, hoff, ctypes.byref(buf)) == I
    assert lib.sccg_reader_lift(rd.ptr, None, 2, hoff, ctypes.byref(buf)) == I
    assert lib.sccg_reader_lift(rd.ptr, ok, 2, hoff, None) == I
    assert lib.sccg_reader_lift_device(rd.ptr, bad_r, 2, d_off.data_ptr(), d_blk.data_ptr(), 64, ctypes.byref(n), None) == I
    assert lib.sccg_reader_lift_device(rd.ptr, None, 2, d_off.data_ptr(), d_blk.data_ptr(), 64, ctypes.byref(n), None) == I
    assert lib.sccg_reader_lift_device(rd.ptr, ok, 2, d_off.data_ptr(), d_blk.data_ptr(), 64, None, None) == I
    assert lib.sccg_reader_lift_device(rd.ptr, ok, 2, d_off.data_ptr() + 4, d_blk.data_ptr(), 64, ctypes.byref(n), None) == I
    assert lib.sccg_reader_lift_device(rd.ptr, ok, 2, d_off.data_ptr(), d_blk.data_ptr() + 4, 64, ctypes.byref(n), None) == I
    for regs, rc, word in ((flag2, I, "flag"), (flag1, I, "flag"), (badsample, I, "sample 9"), (badrange, I, "outside"), (late, U, "sample 8")):
        assert lib.sccg_cohort_lift(co.ptr, regs, 2, hoff, ctypes.byref(buf)) == rc, word
        msg = lib.sccg_last_error(ctx.ptr).decode()
        assert word in msg and "interval 1" in msg, msg
        assert lib.sccg_cohort_lift_device(co.ptr, regs, 2, d_off.data_ptr(), d_blk.data_ptr(), 64, ctypes.byref(n), None) == rc, word
        assert lib.sccg_cohort_lift_device(co.ptr, regs, 2, None, None, 0, ctypes.byref(n), None) == rc, word   # size query
    assert lib.sccg_cohort_lift(co.ptr, None, 2, hoff, ctypes.byref(buf)) == I
    assert lib.sccg_cohort_lift(co.ptr, flag1, 2, hoff, None) == I
    assert lib.sccg_cohort_lift_device(co.ptr, flag1, 2, d_off.data_ptr(), d_blk.data_ptr(), 64, None, None) == I
    torch.cuda.synchronize()
    assert list(hoff) == [77] * 4 and not buf.data and buf.len == 0 and n.value == 77
    assert bool((d_off == 77).all().item()) and bool((d_blk == 77).all().item())
    # and the good call over the same buffers works
    assert lib.sccg_reader_lift_device(rd.ptr, ok, 2, d_off.data_ptr(), d_blk.data_ptr(), 64, ctypes.byref(n), None) == 0
    eoff, eblk = liftlib.want(case.pos[0], [(0, 10), (5, 9)])
    assert d_off[:3].cpu().tolist() == eoff.tolist() and n.value == len(eblk)
    assert np.array_equal(d_blk.cpu().numpy()[:len(eblk)], eblk) and bool((d_blk[len(eblk):] == 77).all().item())
    assert lib.sccg_reader_lift(rd.ptr, ok, 2, hoff, ctypes.byref(buf)) == 0
    assert list(hoff)[:3] == eoff.tolist() and buf.len == 24 * len(eblk)
    lib.sccg_buf_free(ctypes.byref(buf))


# ---------------------------------------------------------------------------------------------
# 10. launches
# ---------------------------------------------------------------------------------------------
WORDS = {"one": 1, "two": 2, "three": 3, "four": 4, "five": 5, "six": 6}


def test_launch_count_is_the_constant_the_header_states(ctx, case):
    """The kernels are bracketed under the profiler's fetch family (its table is closed); a call queues the
    number of launches the header states, whatever n is, and a size query the number it states for one."""
    text = re.sub(r"\n \* ?", " ", open(sccg.HEADER).read())
    stated = re.search(r"Lift: .*?(\w+) kernel launches, one copy of the interval list and one host read .*?\((\w+) launches for a size query\)", text)
    assert stated, "the header states the launches of a lift call and of its size query"
    full, query = WORDS[stated.group(1).lower()], WORDS[stated.group(2).lower()]
    assert query < full <= 6
    lib, rd, co = ctx.lib, case.readers[1], case.cohort
    counts, queries = [], []
    m = ctypes.c_size_t()
    try:
        for n in (1, 3000):
            iv = liftlib.random_regions(case.nR, n, 200, 60 + n)
            ctx.profile(True, families=["fetch"])
            got = rd.lift(iv)
            prof = ctx.profile_get()
            assert set(prof) == {"fetch"}, prof
            counts.append(prof["fetch"][1])
            liftlib.check_oracle(got, liftlib.want(case.pos[1], iv), iv, "profiled")
            items = cohort_items(case, n, 200, 70 + n)
            ctx.profile(True, families=["fetch"])
            got = co.lift(items)
            counts.append(ctx.profile_get()["fetch"][1])
            liftlib.check_oracle(got, liftlib.want(case.pos, items), items, "profiled cohort")
            arr = (sccg.Region * n)(*iv)
            ctx.profile(True, families=["fetch"])
            assert lib.sccg_reader_lift_device(rd.ptr, arr, n, None, None, 0, ctypes.byref(m), None) == 0
            assert m.value == len(liftlib.want(case.pos[1], iv)[1])
            queries.append(ctx.profile_get()["fetch"][1])
    finally:
        ctx.profile(False)
    assert counts == [full] * 4, counts
    assert queries == [query] * 2, queries


# ---------------------------------------------------------------------------------------------
# 11. fetches and locate are what they were
# ---------------------------------------------------------------------------------------------
def test_fetches_and_locate_are_what_they_were(ctx, case):
    regions = [(0, 3000), (25_000, 26_111), (7, 8), (40_000, 41_500)]
    q = np.array([random.Random(5).randrange(case.nR) for _ in range(1000)], dtype=np.int64)
    with case.ref.open_reader(case.recs[2]) as rd:
        rd.enable_locate()

        def everything():
            pos, copies = rd.locate(q)
            return [rd.fetch(regions), rd.fetch_encoded(regions, "origin", "i32"), rd.fetch_encoded(regions, "onehot", "f16", revcomp=True),
                    rd.fetch_encoded(regions, "index", strand=[1, 0, 1, 0]), pos.tobytes(), copies.tobytes()]
        before, bytes_before = everything(), rd.device_bytes
        off, blk = rd.lift([(0, case.nR)] + liftlib.random_regions(case.nR, 500, 2000, 8))
        rd.lift_tensor([(0, case.nR)])
        assert len(blk) > 10
        assert everything() == before and rd.device_bytes == bytes_before
        assert b"".join(before[0]) == b"".join(case.truths[2][b:e] for b, e in regions)
        assert np.array_equal(np.frombuffer(before[4], dtype=np.int64), case.inv[2][0][q])


# ---------------------------------------------------------------------------------------------
# 12. command line
# ---------------------------------------------------------------------------------------------
def test_cli_lift_on_the_worked_example(tmp_path):
    rec, ref = tmp_path / "compressed_genome.txt", tmp_path / "ref.fa"
    rec.write_bytes(cohortlib.ERASED_REC)
    ref.write_bytes(RFA_N)
    pos, _ = locatelib.inverse(RFA_N, cohortlib.ERASED_REC)
    regions1 = [(1, 120), (3, 70), (5, 8), (6, 6), (47, 47), (1, 1), (45, 61)]
    p = subprocess.run([FETCH, "--lift", str(rec), str(ref)] + ["%d-%d" % r if r[0] != r[1] else str(r[0]) for r in regions1],
                       capture_output=True)
    assert p.returncode == 0, p.stderr
    want = liftlib.cli_lines(pos, regions1)
    assert p.stdout.decode().splitlines() == want
    assert want[:3] == [">1-120", "1\t4\t1\t4", "5\t8\tN"] and "47\t52\t-" in want and "61\t64\t39\t42" in want
    p = subprocess.run([FETCH, "--lift", str(rec), str(ref), "100-121"], capture_output=True)   # beyond the reference
    assert p.returncode == 1 and b"outside the reference" in p.stderr and p.stdout == b""
