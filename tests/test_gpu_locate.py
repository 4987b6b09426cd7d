"""Locate on the GPU (sccg_reader_enable_locate, sccg_*_locate): where a position of the reference
sequence lies in a sample -- the first sequence position a token copied it to and the number of copies.

The truth is never the code under test: locatelib inverts originlib's per-base origins (plain Python
from the record format and the reference FASTA) with numpy.  A second truth needs no inverse and is
asserted on the results: the origin fetch of a located position is the reference position asked for,
and the base there is the reference's."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import cohortlib
import fetchlib
import locatelib
import originlib
from cohortlib import HAND, RFA_N
from locatelib import fasta, random_body, record
from pkg import sccg

pytestmark = pytest.mark.gpu
E = sccg.ERR_CODES
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FETCH = os.path.join(REPO, "sccg-genome-compression_amd", "bin", "fetch")


@pytest.fixture(scope="module")
def ctx():
    c = sccg.Context(0)
    yield c
    c.close()


def check_record(ctx, rfa, rec, what, private=False):
    """Every reference position, in one call, against the oracle and the oracle-free truth; then the
    query-count edges, repeated and unordered."""
    want = locatelib.inverse(rfa, rec)
    nR = len(want[0])
    ref = None if private else ctx.open_reference(rfa, coords=True)
    rd = ctx.open_reader(rec, rfa) if private else ref.open_reader(rec)
    try:
        assert rd.has_coords and not rd.can_locate, what
        rd.enable_locate()
        assert rd.can_locate, what
        q = np.arange(nR, dtype=np.int64)
        got = rd.locate(q)
        locatelib.check(got, want, q, what)
        locatelib.check_independent(rd, rfa, q, got[0], what)
        rng = random.Random(nR)
        for n in (0, 1, 63, 64, 65):
            qs = np.array([rng.randrange(nR) for _ in range(n)], dtype=np.int64)
            if n > 2:
                qs[1], qs[2] = qs[0], nR - 1   # repeated; the last base of R
            locatelib.check(rd.locate(qs), want, qs, f"{what} n={n}")
        qs = q[::-1].copy()   # descending
        locatelib.check(rd.locate(qs), want, qs, f"{what} descending")
        return got
    finally:
        rd.close()
        if ref is not None:
            ref.close()


# ---------------------------------------------------------------------------------------------
# 1. hand-written records; the worked example
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND) + ["erased_rec"])
def test_hand_written_records(ctx, name):
    rfa, rec = (RFA_N, cohortlib.ERASED_REC) if name == "erased_rec" else HAND[name]
    pos, copies = check_record(ctx, rfa, rec, name)
    if name == "erased_rec":
        assert pos[:10].tolist() == [0, 1, 2, 3, -2, -2, -2, -2, 8, 9] and pos[60] == 38 and pos[73] == 47 and pos[74] == -1
        assert copies[:10].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 1, 1]
    if name == "literals_only":   # no token at all: every query finds no copy
        assert (pos == -1).all() and (copies == 0).all()


# ---------------------------------------------------------------------------------------------
# 2. index sizes
# ---------------------------------------------------------------------------------------------
def token_record(nR, k, seed, zero_every=0):
    """k tokens of nonzero length at seeded places of a reference of nR bases, literals between some,
    zero-length tokens mixed in."""
    rng = random.Random(seed)
    items = []
    for i in range(k):
        l = rng.randint(1, 40)
        items.append((rng.randrange(nR - l + 1), l))
        if i % 5 == 0:
            items.append(bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 3))))
        if zero_every and i % zero_every == 0:
            items.append((rng.randrange(nR), 0))
    return record(items)


@pytest.mark.parametrize("k,zero_every", [(1, 0), (2, 1), (64, 0), (65, 0), (65, 3), (3000, 0), (3000, 7)])
def test_token_counts(ctx, k, zero_every):
    nR = 1500 if k < 100 else 20_000   # (3,000 tokens of 20 bases on average cover each base three times: some not at all)
    rfa = fasta(random_body(nR, 40 + k))
    rec = token_record(nR, k, 7 * k + zero_every, zero_every)
    pos, copies = check_record(ctx, rfa, rec, f"{k} tokens, zero-length every {zero_every}")
    assert (pos >= 0).any()
    if k >= 3000:
        assert copies.max() >= 4 and (pos == -1).any()


# ---------------------------------------------------------------------------------------------
# 3. overlap
# ---------------------------------------------------------------------------------------------
def test_overlap_record_order_wins(ctx):
    rfa = fasta(random_body(600, 3))
    # 2 and 3 tokens over one base, later in p first in the record; nested; identical; touching
    items = [(120, 30), b"T", (100, 30), (110, 25), b"GG", (300, 50), (310, 10), (310, 10), (300, 50), (320, 1),
             (400, 10), (410, 10), (390, 10), (0, 5), (595, 5)]
    pos, copies = check_record(ctx, rfa, record(items), "overlap")
    # (120,30) sits at sequence 0..29, (100,30) at 31..60, (110,25) at 61..85, the first (300,50) at 88..137
    assert pos[125] == 5 and copies[125] == 3 and pos[115] == 31 + 15 and copies[115] == 2 and pos[105] == 36 and copies[105] == 1
    assert copies[320] == 3 and copies[315] == 4 and copies[305] == 2 and pos[305] == 88 + 5
    assert pos[599] >= 0 and pos[0] >= 0 and pos[399] >= 0 and pos[419] >= 0 and pos[420] == -1


def test_pile_up(ctx):
    """A stuck walk: 4,500 short tokens on one window of 64 bases.  pos is the first token's and copies
    is exact at every position of the window (the oracle's, at every position of the reference)."""
    rfa = fasta(random_body(2000, 9))
    rng = random.Random(4)
    toks = [(700 + rng.randrange(60), rng.randint(1, 4)) for _ in range(4500)]
    items = [(10, 50), b"AC"]
    for k, t in enumerate(toks):
        items.append(t)
        if k % 97 == 0:
            items.append(b"T")
    pos, copies = check_record(ctx, rfa, record(items + [(1500, 100)]), "pile-up")
    assert copies[705:755].min() >= 40 and copies.max() >= 150 and int(copies.sum()) == 150 + sum(l for _, l in toks)
    first, at = {}, 52
    for k, (p, l) in enumerate(toks):
        for r in range(p, p + l):
            first.setdefault(r, at + (r - p))
        at += l + (k % 97 == 0)
    assert all(pos[r] == j for r, j in first.items())


# ---------------------------------------------------------------------------------------------
# 4. coordinates: N runs of the reference and of the target
# ---------------------------------------------------------------------------------------------
def n_reference(seed=1):
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
    nline = b"(0,2)(30,4)(%d,3)" % (84 + 6 - 30)   # the last run behind the last decoded base
    rec = record(toks, lower=b"(3,9)", nline=nline)
    seq, _ = originlib.origins(rfa, rec)
    assert seq.startswith(b"NN") and seq.endswith(b"NNN") and len(seq) == 84 + 9
    pos, copies = check_record(ctx, rfa, rec, f"{rfa_kind} erased")
    R = originlib.ref_sequence(rfa)
    runs = [(m.start(), m.end()) for m in re.finditer(rb"N+", R)]
    assert len(runs) >= 5
    for a, e in runs:   # first and last base of each run, both neighbours
        assert pos[a] == -2 and pos[e - 1] == -2 and copies[a] == 0 and copies[e - 1] == 0
        assert (a == 0 or pos[a - 1] != -2) and (e == len(R) or pos[e] != -2)
    if variant:
        assert R[0:1] == b"N" and R[-1:] == b"N" and pos[0] == -2 and pos[len(R) - 1] == -2
        low = R.index(b"n")
        assert pos[low] >= 0 and seq[pos[low]:pos[low] + 1].upper() == b"N"   # a lowercase n is a base of R'
    assert pos[3 if variant else 0] == 2   # the first base of R' sits behind the target's first N run
    assert pos[len(R) - 3 if variant else len(R) - 1] == 2 + 30 + 4 + 2 + 39   # the last base of R'
    # the kept form over the same reference: shared and private, an N is locatable
    kept = record([(0, 30), b"AC", (len(R) - 40, 40), (2, 12)], nline=b",")
    for private in (False, True):
        kp, kc = check_record(ctx, rfa, kept, f"{rfa_kind} kept private={private}", private=private)
        assert (kp == -2).sum() == 0 and kp[len(R) - 1] == 32 + 39 and kp[runs[0][0]] >= 0 and kc[runs[0][0]] >= 1


# ---------------------------------------------------------------------------------------------
# 5. real records: eight samples over one shared reference
# ---------------------------------------------------------------------------------------------
class LocateCohort:
    def __init__(self, ctx):
        self.rfa, targets = cohortlib.make_cohort_inputs()
        body = fetchlib.split_fasta(self.rfa)[1]
        bodies = [targets[k][1] for k in cohortlib.KINDS]
        bodies += [cohortlib.make_target(body, kind, seed) for kind, seed in (("indel", 201), ("nruns", 202), ("block", 203))]
        self.truths = bodies
        self.recs = [ctx.compress(self.rfa, cohortlib.wrap60(b"s%d" % i, b)) for i, b in enumerate(bodies)]
        self.want = [locatelib.inverse(self.rfa, r) for r in self.recs]
        self.nR = len(self.want[0][0])
        self.ref = ctx.open_reference(self.rfa, coords=True)
        self.private = [i % 2 == 1 and cohortlib.n_line(r) == b"," for i, r in enumerate(self.recs)]
        self.readers = [ctx.open_reader(r, self.rfa) if pv else self.ref.open_reader(r) for pv, r in zip(self.private, self.recs)]
        self.bytes_before = [rd.device_bytes for rd in self.readers]
        self.late = self.ref.open_reader(self.recs[0])   # sample 8: joins both cohorts before it enables locating
        self.early_cohort = sccg.Cohort(self.readers + [self.late])
        for rd in self.readers:
            rd.enable_locate()
        self.cohort = sccg.Cohort(self.readers + [self.late])
        self.late.enable_locate()

    def close(self):
        self.cohort.close()
        self.early_cohort.close()
        self.late.close()
        for rd in self.readers:
            rd.close()
        self.ref.close()


@pytest.fixture(scope="module")
def case(ctx):
    c = LocateCohort(ctx)
    yield c
    c.close()


def cohort_items(case, n, seed):
    rng = random.Random(seed)
    return [(rng.randrange(8), rng.randrange(case.nR)) for _ in range(n)]


def check_items(case, items, got, what):
    gp, gc = got
    assert gp.shape == gc.shape == (len(items),), what
    for s in range(8):
        idx = np.array([k for k, it in enumerate(items) if it[0] == s], dtype=np.int64)
        if idx.size:
            q = np.array([items[k][1] for k in idx], dtype=np.int64)
            locatelib.check((gp[idx], gc[idx]), case.want[s], q, f"{what} sample {s}")
            locatelib.check_independent(case.readers[s], case.rfa, q, gp[idx], f"{what} sample {s}")


def test_cohort_locate(ctx, case):
    assert any(case.private) and not all(case.private), case.private   # private kept-form and shared readers mixed
    assert any(cohortlib.n_line(r) != b"," for r in case.recs)
    items = cohort_items(case, 5000, 1)
    got = case.cohort.locate(items)
    check_items(case, items, got, "cohort")
    assert (got[0] >= 0).any() and (got[0] == -1).any() and (got[1] >= 1).any()
    # the readers' own answers are the cohort's
    for s in range(8):
        sel = np.array([k for k, it in enumerate(items) if it[0] == s])
        rp, rc = case.readers[s].locate(np.array([items[k][1] for k in sel], dtype=np.int64))
        assert np.array_equal(rp, got[0][sel]) and np.array_equal(rc, got[1][sel]), s
    for n in (0, 1, 63, 64, 65):
        it = cohort_items(case, n, 10 + n)
        check_items(case, it, case.cohort.locate(it), f"cohort n={n}")
    # every position of one erased-form and one kept-form sample
    for s in (2, case.private.index(True)):
        q = np.arange(case.nR, dtype=np.int64)
        locatelib.check(case.readers[s].locate(q), case.want[s], q, f"sample {s}, every position")


def test_locate_tensor(ctx, case):
    import torch
    items = cohort_items(case, 300, 3)
    pos, copies = case.cohort.locate_tensor(items)
    torch.cuda.synchronize()
    assert pos.dtype == torch.int64 and copies.dtype == torch.int32 and pos.device == torch.device("cuda", 0)
    check_items(case, items, (pos.cpu().numpy(), copies.cpu().numpy()), "cohort tensor")
    q = np.array([r for _, r in items], dtype=np.int64)
    pos, copies = case.readers[4].locate_tensor(q)
    torch.cuda.synchronize()
    locatelib.check((pos.cpu().numpy(), copies.cpu().numpy()), case.want[4], q, "reader tensor")
    # copies may be NULL in both forms
    d_pos = torch.full((len(q),), 77, dtype=torch.int64, device=pos.device)
    qa = (ctypes.c_int64 * len(q))(*q.tolist())
    assert ctx.lib.sccg_reader_locate_device(case.readers[4].ptr, qa, len(q), d_pos.data_ptr(), None, None) == 0
    assert np.array_equal(d_pos.cpu().numpy(), case.want[4][0][q])
    hp = (ctypes.c_int64 * len(q))()
    assert ctx.lib.sccg_reader_locate(case.readers[4].ptr, qa, len(q), hp, None) == 0
    assert list(hp) == case.want[4][0][q].tolist()


def test_fetch_tensor_at(ctx, case):
    import torch
    rng = random.Random(8)
    L = 129
    items = []
    for s in range(8):
        wp = case.want[s][0]
        hits, miss = np.nonzero(wp >= 0)[0], np.nonzero(wp < 0)[0]
        items += [(s, int(hits[rng.randrange(hits.size)])) for _ in range(12)]
        items += [(s, int(miss[rng.randrange(miss.size)])) for _ in range(2) if miss.size]
        late = hits[wp[hits] + L > len(case.truths[s])]   # a window that would pass the sample's end
        items += [(s, int(late[-1]))] if late.size else []
    found_want = [bool(case.want[s][0][r] >= 0 and case.want[s][0][r] + L <= len(case.truths[s])) for s, r in items]
    assert not all(found_want) and sum(found_want) >= 80
    assert any(case.want[s][0][r] >= 0 and not f for (s, r), f in zip(items, found_want))   # located, but out of the sample
    windows = [(s, int(case.want[s][0][r]), int(case.want[s][0][r]) + L) for (s, r), f in zip(items, found_want) if f]
    for enc, dt in (("onehot", None), ("index", None), ("onehot", torch.float32)):
        t, found = case.cohort.fetch_tensor_at(items, L, enc, dt)
        torch.cuda.synchronize()
        assert found.dtype == torch.bool and found.cpu().tolist() == found_want
        ref = case.cohort.fetch_tensor(windows, enc, dt)
        assert t.dtype == ref.dtype and tuple(t.shape) == (len(items), L) + tuple(ref.shape[2:])
        assert torch.equal(t[found], ref)
        assert not bool(t[~found].any().item())
    good = [it for it, f in zip(items, found_want) if f][:12]   # all found: the fetch's own tensor
    t, found = case.cohort.fetch_tensor_at(good, L, "ascii", revcomp=True)
    assert bool(found.all().item()) and torch.equal(t, case.cohort.fetch_tensor(windows[:12], "ascii", revcomp=True))
    t, found = case.cohort.fetch_tensor_at([], L)
    assert tuple(t.shape) == (0, L, 4) and tuple(found.shape) == (0,)
    try:   # two launches in all: the locate kernel is bracketed under the fetch family
        ctx.profile(True, families=["fetch"])
        case.cohort.fetch_tensor_at(items, L)
        assert ctx.profile_get()["fetch"][1] == 2
    finally:
        ctx.profile(False)


# ---------------------------------------------------------------------------------------------
# 6. contract
# ---------------------------------------------------------------------------------------------
def test_enable_is_idempotent_and_counted(ctx, case):
    for rd, before in zip(case.readers, case.bytes_before):
        after = rd.device_bytes
        assert after > before
        rd.enable_locate()
        assert rd.device_bytes == after and rd.can_locate
    with case.ref.open_reader(case.recs[2]) as rd:
        b0 = rd.device_bytes
        assert b0 == case.bytes_before[2] and not rd.can_locate   # not before
        # the index by its documented layout: nt tokens of nonzero length, ne distinct starts and ends; five
        # arrays (4 nt, 8 nt, 4 ne, 4 ne, 8 ne bytes), each padded to 256 bytes, and 256 behind them
        p, ends, nt = 0, set(), 0
        for m in re.finditer(rb"\((-?\d+),(\d+)\)", case.recs[2].rstrip(b"\n").rpartition(b"\n")[2]):
            p += int(m.group(1))
            if int(m.group(2)):
                nt += 1
                ends |= {p, p + int(m.group(2))}
        ne = len(ends)
        rd.enable_locate()
        grown = rd.device_bytes - b0
        assert nt >= 10 and ne >= nt and grown == sum((x + 255) // 256 * 256 for x in (4 * nt, 8 * nt, 4 * ne, 4 * ne, 8 * ne)) + 256, (grown, nt, ne)
        assert grown <= 44 * nt + 6 * 256


def test_fetches_are_what_they_were(ctx, case):
    regions = [(0, 3000), (25_000, 26_111), (7, 8), (40_000, 41_500)]
    with case.ref.open_reader(case.recs[2]) as rd:
        def all_fetches():
            return [rd.fetch(regions), rd.fetch_encoded(regions, "origin", "i32"), rd.fetch_encoded(regions, "onehot", "f16", revcomp=True),
                    rd.fetch_encoded(regions, "index", strand=[1, 0, 1, 0])]
        before = all_fetches()
        rd.enable_locate()
        assert all_fetches() == before
        assert b"".join(before[0]) == b"".join(case.truths[2][b:e] for b, e in regions)


def expect(rc_name, text, call):
    with pytest.raises(sccg.SccgError) as ei:
        call()
    assert ei.value.rc == E[rc_name] and text in str(ei.value), str(ei.value)


def test_errors_write_nothing(ctx, case):
    import torch
    dev = torch.device("cuda", 0)
    rd, co, nR = case.readers[0], case.cohort, case.nR
    # a reader that has not enabled locating; readers without coordinates
    with case.ref.open_reader(case.recs[0]) as fresh:
        expect("SCCG_E_UNSUPPORTED", "enable", lambda: fresh.locate([5]))
        expect("SCCG_E_UNSUPPORTED", "enable", lambda: fresh.locate([]))
        expect("SCCG_E_UNSUPPORTED", "enable", lambda: fresh.locate_tensor([5]))
    with ctx.open_reader(case.recs[2], case.rfa) as nocoords:
        assert not nocoords.has_coords
        expect("SCCG_E_UNSUPPORTED", "coordinates", nocoords.enable_locate)
        assert not nocoords.can_locate
    with ctx.open_reference(case.rfa) as plain, plain.open_reader(case.recs[2]) as shared:
        expect("SCCG_E_UNSUPPORTED", "SCCG_REF_COORDS", shared.enable_locate)
    # positions outside [0, |R|), samples outside the cohort: the first offender is named
    expect("SCCG_E_INVALID", "query 2", lambda: rd.locate([0, nR - 1, nR, -1]))
    expect("SCCG_E_INVALID", "query 0", lambda: rd.locate([-1]))
    expect("SCCG_E_INVALID", "locus 1", lambda: co.locate([(0, 5), (3, nR), (9, 0)]))
    expect("SCCG_E_INVALID", "sample 9", lambda: co.locate([(0, 5), (9, 0), (3, nR)]))
    expect("SCCG_E_INVALID", "sample -1", lambda: co.locate([(-1, 0)]))
    # sample 8 had not enabled locating when either cohort was created; the early cohort knows of none
    expect("SCCG_E_UNSUPPORTED", "locus 1", lambda: co.locate([(0, 5), (8, 5), (0, nR)]))
    expect("SCCG_E_INVALID", "locus 0", lambda: co.locate([(0, nR), (8, 5)]))
    expect("SCCG_E_UNSUPPORTED", "locus 0", lambda: case.early_cohort.locate([(0, 5)]))
    assert case.late.can_locate and case.late.locate([5])[0][0] == case.want[0][0][5]
    # raw calls: sentinel-filled outputs stay as they were
    lib = ctx.lib
    hp, hc = (ctypes.c_int64 * 4)(*[77] * 4), (ctypes.c_int32 * 4)(*[77] * 4)
    d_pos = torch.full((8,), 77, dtype=torch.int64, device=dev)
    d_cp = torch.full((8,), 77, dtype=torch.int32, device=dev)
    q_bad, q_ok = (ctypes.c_int64 * 4)(1, 2, nR, 3), (ctypes.c_int64 * 4)(1, 2, 3, 4)
    flagged = (sccg.CohortLocus * 2)((5, 0, 0), (6, 1, 1))
    badsample = (sccg.CohortLocus * 2)((5, 0, 0), (6, 9, 0))
    badpos = (sccg.CohortLocus * 2)((5, 0, 0), (nR, 1, 0))
    late = (sccg.CohortLocus * 2)((5, 0, 0), (6, 8, 0))
    I, U = E["SCCG_E_INVALID"], E["SCCG_E_UNSUPPORTED"]
    assert lib.sccg_reader_locate(rd.ptr, q_bad, 4, hp, hc) == I
    assert lib.sccg_reader_locate(rd.ptr, None, 4, hp, hc) == I
    assert lib.sccg_reader_locate(rd.ptr, q_ok, 4, None, hc) == I
    assert lib.sccg_reader_locate_device(rd.ptr, q_bad, 4, d_pos.data_ptr(), d_cp.data_ptr(), None) == I
    assert lib.sccg_reader_locate_device(rd.ptr, q_ok, 4, None, d_cp.data_ptr(), None) == I
    assert lib.sccg_reader_locate_device(rd.ptr, q_ok, 4, d_pos.data_ptr() + 4, d_cp.data_ptr(), None) == I
    assert "d_pos" in lib.sccg_last_error(ctx.ptr).decode()
    assert lib.sccg_reader_locate_device(rd.ptr, q_ok, 4, d_pos.data_ptr(), d_cp.data_ptr() + 2, None) == I
    assert "d_copies" in lib.sccg_last_error(ctx.ptr).decode()
    for loci, rc, word in ((flagged, I, "flag"), (badsample, I, "sample 9"), (badpos, I, "outside"), (late, U, "sample 8")):
        assert lib.sccg_cohort_locate(co.ptr, loci, 2, hp, hc) == rc, word
        assert word in lib.sccg_last_error(ctx.ptr).decode() and "locus 1" in lib.sccg_last_error(ctx.ptr).decode()
        assert lib.sccg_cohort_locate_device(co.ptr, loci, 2, d_pos.data_ptr(), d_cp.data_ptr(), None) == rc, word
    assert lib.sccg_cohort_locate(co.ptr, None, 2, hp, hc) == I
    assert lib.sccg_cohort_locate_device(co.ptr, late, 1, d_pos.data_ptr() + 4, None, None) == I
    # n == 0 is OK and writes nothing
    assert lib.sccg_reader_locate(rd.ptr, None, 0, None, None) == 0
    assert lib.sccg_reader_locate_device(rd.ptr, None, 0, None, None, None) == 0
    assert lib.sccg_cohort_locate(co.ptr, None, 0, hp, hc) == 0
    assert lib.sccg_cohort_locate_device(co.ptr, None, 0, d_pos.data_ptr(), d_cp.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert list(hp) == [77] * 4 and list(hc) == [77] * 4
    assert bool((d_pos == 77).all().item()) and bool((d_cp == 77).all().item())
    # and the good call over the same buffers works
    assert lib.sccg_reader_locate_device(rd.ptr, q_ok, 4, d_pos.data_ptr(), d_cp.data_ptr(), None) == 0
    assert d_pos[:4].cpu().tolist() == case.want[0][0][1:5].tolist() and d_pos[4:].cpu().tolist() == [77] * 4


def test_one_launch_whatever_n_is(ctx, case):
    """The locate kernel is bracketed under the profiler's fetch family (its table is closed), and a
    locate call launches nothing else of that family."""
    counts = []
    try:
        for n in (1, 5000):
            q = np.array([r for _, r in cohort_items(case, n, 20 + n)], dtype=np.int64)
            ctx.profile(True, families=["fetch"])
            got = case.readers[2].locate(q)
            prof = ctx.profile_get()
            assert set(prof) == {"fetch"}, prof
            counts.append(prof["fetch"][1])
            locatelib.check(got, case.want[2], q, "profiled")
            items = cohort_items(case, n, 30 + n)
            ctx.profile(True, families=["fetch"])
            got = case.cohort.locate(items)
            counts.append(ctx.profile_get()["fetch"][1])
            check_items(case, items, got, "profiled cohort")
    finally:
        ctx.profile(False)
    assert counts == [1, 1, 1, 1], counts


# ---------------------------------------------------------------------------------------------
# 7. command line
# ---------------------------------------------------------------------------------------------
def test_cli_locate_on_the_worked_example(tmp_path):
    rec, ref = tmp_path / "compressed_genome.txt", tmp_path / "ref.fa"
    rec.write_bytes(cohortlib.ERASED_REC)
    ref.write_bytes(RFA_N)
    wp, wc = locatelib.inverse(RFA_N, cohortlib.ERASED_REC)
    qs = [1, 4, 5, 8, 9, 21, 47, 49, 61, 74, 75, 120, 9]
    p = subprocess.run([FETCH, "--locate", str(rec), str(ref)] + [str(q) for q in qs], capture_output=True)
    assert p.returncode == 0, p.stderr
    want = ["%d\t%s\t%d" % (q, "N" if wp[q - 1] == -2 else "-" if wp[q - 1] == -1 else str(wp[q - 1] + 1), wc[q - 1]) for q in qs]
    assert p.stdout.decode().splitlines() == want
    assert want[0] == "1\t1\t1" and want[2] == "5\tN\t0" and want[6] == "47\t-\t0" and want[8] == "61\t39\t1"
    p = subprocess.run([FETCH, "--locate", str(rec), str(ref), "121"], capture_output=True)   # beyond the reference
    assert p.returncode == 1 and b"outside the reference" in p.stderr and p.stdout == b""
