"""Find with mismatches on the GPU (sccg_reader_find_approx*, sccg_cohort_find_approx*): where an IUPAC pattern
occurs within K substitutions in regions of a sample, on either strand, each hit with its mismatch count.

The truth is never the code under test (findapproxlib): a per-start mismatch count over the sequence's bytes,
which are cohortlib.hand_sequence's for the hand-built records and the target's body for compressed ones.  One
more truth needs no oracle and is asserted on the GPU's own outputs: the index fetch of every reported window
gives the reported number of mismatches."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import cohortlib
import findapproxlib as fa
import findlib
from cohortlib import HAND, RFA_N
from locatelib import fasta, random_body, record
from pkg import sccg

pytestmark = pytest.mark.gpu
E = sccg.ERR_CODES
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRANDS = ("both", "+", "-")


@pytest.fixture(scope="module")
def ctx():
    c = sccg.Context(0)
    yield c
    c.close()


class Readers:
    """The readers a record can be searched through: private, shared, shared with reference coordinates."""

    def __init__(self, ctx, rfa, rec, only=None):
        self.refs = [ctx.open_reference(rfa), ctx.open_reference(rfa, coords=True)]
        self.all = {"private": ctx.open_reader(rec, rfa), "shared": self.refs[0].open_reader(rec), "coords": self.refs[1].open_reader(rec)}
        self.use = {k: v for k, v in self.all.items() if only is None or k in only}
        self.seq = cohortlib.hand_sequence(rfa, rec)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for rd in self.all.values():
            rd.close()
        for ref in self.refs:
            ref.close()

    def check(self, pattern, regions, K, strands="both", what=""):
        """Every reader against the oracle (computed once); returns the pair."""
        regions = list(regions)
        expected = fa.want(self.seq, pattern, regions, K, strands)
        for name, rd in self.use.items():
            assert rd.length == len(self.seq)
            fa.check(rd.find_approx(pattern, regions, K, strands), expected, regions, f"{what} {name} {fa.text(pattern)} K={K} {strands}")
        return expected


def rows(hits):
    return [tuple(r) for r in np.asarray(hits).tolist()]


def cut_places(seq: bytes, m: int):
    return [j for j in range(len(seq) - m + 1) if all(c in b"ACGTacgt" for c in seq[j:j + m])]


def altered(pat: str, letters) -> str:
    """The pattern with the given letters changed to another of A, C, G, T."""
    p = list(pat)
    for t in letters:
        p[t] = "ACGT"[("ACGT".index(p[t]) + 1 + t % 3) % 4]
    return "".join(p)


# ---------------------------------------------------------------------------------------------
# 1. hand-written records
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND) + ["erased_rec"])
def test_hand_written_records(ctx, name):
    rfa, rec = (RFA_N, cohortlib.ERASED_REC) if name == "erased_rec" else HAND[name]
    with Readers(ctx, rfa, rec) as p:
        if name == "erased_rec":
            assert p.seq == cohortlib.ERASED_SEQ
        L = len(p.seq)
        pairs = fa.every_pair(min(L, 120))
        rng = random.Random(3)
        patterns = []
        for m in (2, 4, 8):
            places = cut_places(p.seq, m)
            if places:
                cut = p.seq[rng.choice(places):][:m].decode().upper()
                patterns += [altered(cut, [m - 1]), altered(cut, [0, m // 2])]
        assert len(patterns) >= 4, patterns
        inexact = 0
        for pat in patterns:
            for K in (0, 1, 2):
                if K >= len(pat):
                    continue
                for strands in STRANDS:
                    p.check(pat, pairs, K, strands, name)
                    inexact += int((p.check(pat, [(0, L)], K, strands, name + " whole")[1][:, 2] > 0).sum())
        assert inexact > 0


# ---------------------------------------------------------------------------------------------
# 2. word and tile edges
# ---------------------------------------------------------------------------------------------
def split_record(body: bytes, tok: int) -> bytes:
    """body over a reference that is body: tokens of `tok` bases with one literal between two of them."""
    items, at = [], 0
    while at < len(body):
        l = min(tok, len(body) - at)
        items.append((at, l))
        at += l
        if at < len(body):
            items.append(body[at:at + 1])
            at += 1
    return record(items)


def planted(n: int, k: int, seed: int) -> bytes:
    rng = random.Random(seed)
    a = bytearray(b"A" * n)
    for at in rng.sample(range(n), k):
        a[at] = ord("C")
    return bytes(a)


def edge_pattern(m: int):
    """"A" * m with C at letter 0, letter m - 1 and both ends of every 16-letter word: (pattern, letters altered)."""
    at = sorted({t for t in (0, m - 1, 15, 16, 31, 32, 47, 48) if t < m})
    p = ["A"] * m
    for t in at:
        p[t] = "C"
    return "".join(p), len(at)


@pytest.mark.parametrize("layout", ["one_token", "tokens_of_700"])
@pytest.mark.parametrize("body_kind", ["poly_a", "planted_c"])
def test_word_and_tile_edges(ctx, layout, body_kind):
    n = 3300
    body = b"A" * n if body_kind == "poly_a" else planted(n, 40, 8)
    rec = record([(0, n)]) if layout == "one_token" else split_record(body, 700)
    rng = random.Random(5)
    with Readers(ctx, fasta(body), rec, only=("private", "coords")) as p:
        assert p.seq == body
        regions = [(0, n), (1, n - 1), (17, 3000)] + [tuple(sorted((rng.randrange(n + 1), rng.randrange(n + 1)))) for _ in range(40)]
        for m in (1, 15, 16, 17, 32, 33, 48, 49, 64):
            pat, na = edge_pattern(m)
            assert na == {1: 1, 15: 2, 16: 2, 17: 3, 32: 4, 33: 5, 48: 6, 49: 7, 64: 8}[m]
            for K in sorted({k for k in (na - 1, na, min(m - 1, 15)) if 0 <= k < m}):
                strands = STRANDS[(m + K) % 3]
                off, hits = p.check(pat, regions, K, strands, f"{layout} {body_kind} m={m}")
                if body_kind == "poly_a" and strands != "-":
                    fwd = hits[:off[1]][hits[:off[1], 1] == 0]
                    if K >= na:   # every candidate is a forward hit with exactly na mismatches, at consecutive positions
                        assert fwd[:, 0].tolist() == list(range(n - m + 1)) and set(fwd[:, 2].tolist()) == {na}
                    else:         # one less gives none
                        assert len(fwd) == 0
            if m <= 16:
                off, hits = p.check("C" * m, regions, m - 1, "+", f"{layout} {body_kind} poly-C")
                assert body_kind != "poly_a" or len(hits) == 0


# ---------------------------------------------------------------------------------------------
# 3. N bases are mismatches
# ---------------------------------------------------------------------------------------------
MOTIF = b"GATTACAGGCTC"   # 12 letters, no palindrome


def boundary_case():
    """(rfa, rec, the motif's places in the sequence before the N runs go in, the runs by decoded offset)."""
    m = len(MOTIF)
    base = bytearray(random_body(700, 31))
    for at in (120, 300, 420, 520, 560, 600):
        base[at:at + m] = MOTIF
    # R: an N run inside the motif at 420 (R' has it whole); the record indexes the erased form
    R = bytes(base[:426]) + b"NNNN" + bytes(base[426:])
    items = [
        (100, 26), MOTIF[6:] + b"T",            # token | literal: the token ends with the motif's first half (R' 120..125)
        b"C" + MOTIF[:5], (125, 20),            # literal | token: the token starts at the motif's sixth letter
        (110, 16), (306, 20),                   # two tokens that are not neighbours on the reference
        (400, 50),                              # a token over the erased reference run: R' 420..431 is the motif
        (510, 22), (532, 20),                   # 520: the motif ends the first token; a target N run goes in behind it
        (560, 30),                              # 560: a target N run goes in before it
        (600, 12),                              # the motif at 600 is cut by a run in the middle
    ]
    seq0 = b"".join(it if isinstance(it, bytes) else bytes(base[it[0]:it[0] + it[1]]) for it in items)
    hits0 = [mm.start() for mm in re.finditer(MOTIF, seq0)]
    assert len(hits0) == 7, hits0
    # N runs by decoded offset: right behind hit 4 (the 520 motif), right before hit 5 (560), inside hit 6 (600)
    d_behind, d_before, d_inside = hits0[4] + m, hits0[5], hits0[6] + 5
    runs = [(d_behind, 3), (d_before, 14), (d_inside, 2)]
    nline, prev, shift = b"", 0, 0
    for d, l in runs:   # the N line lists sequence positions: each run shifts the ones behind it
        nline += b"(%d,%d)" % (d + shift - prev, l)
        prev = d + shift
        shift += l
    return fasta(R), record(items, nline=nline), hits0, runs


def test_n_bases_are_mismatches(ctx):
    rfa, rec, hits0, runs = boundary_case()
    m, pat = len(MOTIF), MOTIF.decode()
    with Readers(ctx, rfa, rec, only=("shared", "coords")) as p:
        seq = p.seq
        L = len(seq)
        assert seq.count(b"N") == sum(l for _, l in runs)
        found = [mm.start() for mm in re.finditer(MOTIF, seq)]
        n_at = [mm.span() for mm in re.finditer(rb"N+", seq)]
        assert len(found) == 6 and [e - s for s, e in n_at] == [3, 14, 2]
        # the seventh motif holds the 2-base run: MOTIF[:5] NN MOTIF[5:], 14 bases; a window of 12 from its start sees
        # MOTIF[:5] + NN + MOTIF[5:10] = 5 matches, 2 N, then MOTIF[5:10] against MOTIF[7:12]
        cut = n_at[2][0] - 5
        assert seq[cut:cut + 14] == MOTIF[:5] + b"NN" + MOTIF[5:]
        d_cut = 2 + sum(1 for a, b in zip(MOTIF[5:10], MOTIF[7:12]) if a != b)
        assert d_cut > 2   # the run shifts the motif's tail: more than the two N mismatch
        for K in (0, 1, 2):   # the plain motif is not there: not at 0, not at 1, not at 2
            off, hits = p.check(pat, [(0, L)], K, "both", "boundaries")
            assert [r for r in rows(hits) if r[2] == 0] == [(j, 0, 0) for j in found]
            assert not any(cut <= r[0] <= cut + 2 and r[1] == 0 for r in rows(hits))
        # the motif as the run cuts it, 14 letters with N N where the run lies: the sequence's two N are mismatches
        # even against the pattern's N -- absent at K = 0, still absent at K = 1, present at K = 2 with mismatches == 2
        gap = pat[:5] + "NN" + pat[5:]
        for K, there in ((0, False), (1, False), (2, True)):
            got = rows(p.check(gap, [(0, L)], K, "both", "the cut motif")[1])
            assert ((cut, 0, 2) in got) == there and not any(r[:2] == (cut, 0) and r[2] != 2 for r in got)
        for j, q in [(j, pat) for j in found] + [(cut, pat), (cut, gap)]:   # every begin and end around each placement
            regs = [(b, e) for b in range(max(j - 3, 0), j + 4) for e in range(j + len(q) - 3, min(j + len(q) + 4, L + 1))]
            for K in (0, 1, 2):
                p.check(q, regs, K, "both", f"around {j}")
        # "N" * 5 at K = 1 over the 14-base run and its flanks: exactly one N is a hit with d = 1, two are not
        s, e = n_at[1]
        flank = (s - 6, e + 6)
        assert all(c in b"ACGTacgt" for c in seq[s - 6:s] + seq[e:e + 6])
        off, hits = p.check("N" * 5, [flank, (s, e), (s - 4, e), (s, e + 4), (s - 5, s), (e, e + 5), (s - 4, s + 1), (s - 3, s + 2)], 1, "+",
                            "N run")
        assert rows(hits[:off[1]]) == [(s - 6, 0, 0), (s - 5, 0, 0), (s - 4, 0, 1), (e - 1, 0, 1), (e, 0, 0), (e + 1, 0, 0)]
        assert np.diff(off).tolist() == [6, 0, 1, 1, 1, 1, 1, 0]
        p.check("N" * 12, fa.every_pair(L)[::53], 3, "both", "N pattern")
        p.check("NNNNNNNNNNNNNNNNNNNNNGG", [(0, L)], 2, "both", "guide + PAM")


# ---------------------------------------------------------------------------------------------
# 4. region rules
# ---------------------------------------------------------------------------------------------
def motif_sample(n=5000, every=97, seed=12):
    body = bytearray(random_body(n, seed))
    sites = list(range(40, n - 40, every))
    for at in sites:
        body[at:at + len(MOTIF)] = MOTIF
    return bytes(body), sites


def test_region_rules(ctx):
    body, sites = motif_sample()
    m = len(MOTIF)
    pat = altered(MOTIF.decode(), [3, 9])   # two letters off every planted site
    with Readers(ctx, fasta(body), split_record(body, 333), only=("private", "coords")) as p:
        assert p.seq == body
        j = sites[3]
        ends = [(j, j + m), (j, j + m - 1), (j + 1, j + m), (j - 1, j + m), (j, j + m + 1), (j, j), (j + m, j + m)]
        off, hits = p.check(pat, ends, 2, "both", "ends")   # a window within K that crosses `end` is no hit
        assert np.diff(off).tolist() == [1, 0, 0, 1, 1, 0, 0] and rows(hits) == [(j, 0, 2)] * 3
        assert len(p.check(pat, ends, 1, "both", "ends, K too small")[1]) == 0
        # repeated, overlapping, unordered
        regs = [(sites[9], sites[12] + m), (sites[2], sites[5] + m), (sites[9], sites[12] + m), (sites[10] + 1, sites[12] + m), (0, 5000),
                (sites[2], sites[5] + m)]
        off, hits = p.check(pat, regs, 2, "both", "repeated overlapping unordered")
        assert np.diff(off).tolist() == [4, 4, 4, 2, len(sites), 4]
        # 2,000 one-motif regions in one call, in a shuffled order, every third one a base too short
        rng = random.Random(2)
        many = [(s, s + m - (k % 3 == 2)) for k, s in enumerate(rng.choices(sites, k=2000))]
        off, hits = p.check(pat, many, 2, "both", "2,000 regions")
        assert off[-1] == len(hits) == sum(1 for b, e in many if e - b == m) and set(hits[:, 2].tolist()) == {2}
        # n == 0
        off, hits = p.check(pat, [], 2, "both", "no region")
        assert off.tolist() == [0] and hits.shape == (0, 3)
        # regions that own no candidate at the front, in the middle and at the end of the list
        empties = [(5, 5), (0, m - 1), (sites[0], sites[1] + m), (7, 7), (9, 9 + m - 1), (5000, 5000), (sites[4], sites[4] + m), (3, 3),
                   (5000 - m + 1, 5000)]
        off, hits = p.check(pat, empties, 2, "both", "empty regions")
        assert off.tolist() == [0, 0, 0, 2, 2, 2, 2, 3, 3, 3]
        off, hits = p.check(pat, [(4, 4), (0, 3), (5000, 5000)], 2, "both", "only empty regions")
        assert off.tolist() == [0, 0, 0, 0] and len(hits) == 0
        p.check(pat, [(0, 5000)] * 3 + [(0, 0)] + [(0, 5000)], 3, "-", "the other strand")


# ---------------------------------------------------------------------------------------------
# 5. both strands
# ---------------------------------------------------------------------------------------------
def test_both_strands(ctx):
    body = bytearray(random_body(4000, 77))
    pal = list(range(100, 3900, 313))
    for at in pal:
        body[at:at + 6] = b"GAATTA"   # the palindrome GAATTC with one letter altered in the sample
    asym, rc = MOTIF, findlib.revcomp_pattern(MOTIF).encode()
    for k, at in enumerate(range(50, 3900, 411)):
        body[at:at + 12] = asym if k % 2 == 0 else rc
    body = bytes(body)
    sites_r = [mm.start() for mm in re.finditer(rc, body)]
    assert len(sites_r) >= 4
    with Readers(ctx, fasta(body), split_record(body, 450), only=("shared",)) as p:
        whole = [(0, len(body))]
        off, hits = p.check("GAATTC", whole + [(a, a + 6) for a in pal], 1, "both", "palindrome")
        assert rows(hits[off[1]:]) == [(a, s, 1) for a in pal for s in (0, 1)]   # two rows a site, forward first, both d = 1
        for a in pal:
            assert (a, 0, 1) in rows(hits[:off[1]]) and (a, 1, 1) in rows(hits[:off[1]])
        # a site where the two strands' d differ: GAATTA itself is there on the forward strand, two letters off on the reverse
        off, hits = p.check("GAATTA", [(a, a + 6) for a in pal], 2, "both", "strands differ")
        assert rows(hits) == [(a, s, 2 * s) for a in pal for s in (0, 1)]
        p.check("GAATTA", whole, 2, "both", "strands differ, whole")
        # "-" alone is the reverse-complemented pattern on "+", relabelled, mismatches included
        rd = p.use["shared"]
        regs = whole + [(s - 2, s + 20) for s in sites_r]
        for pat, K in ((altered(asym.decode(), [4]), 1), (altered(asym.decode(), [0, 11]), 3), ("GAATTC", 1), ("RYN", 1), ("GGNCC", 2)):
            moff, mhit = rd.find_approx(pat, regs, K, "-")
            poff, phit = rd.find_approx(findlib.revcomp_pattern(pat), regs, K, "+")
            assert moff.tolist() == poff.tolist() and np.array_equal(mhit[:, [0, 2]], phit[:, [0, 2]]), pat
            assert set(mhit[:, 1].tolist()) <= {1} and set(phit[:, 1].tolist()) <= {0} and len(mhit) > 0, pat
            assert (mhit[:, 2] > 0).any(), pat
            p.check(pat, regs, K, "both", "relabelled")


# ---------------------------------------------------------------------------------------------
# 6. IUPAC, case
# ---------------------------------------------------------------------------------------------
def test_iupac_letters_and_case(ctx):
    body = b"ACGT" * 6 + random_body(1200, 5) + b"AACCGGTT" * 4
    lower = b"(3,9)(20,700)(800,3)"
    rec = record([(0, 600), body[600:607], (607, len(body) - 607)], lower=lower)
    with Readers(ctx, fasta(body), rec, only=("private", "coords")) as p:
        assert p.seq.upper() == body and p.seq != body and p.seq[3:12].islower()
        whole = [(0, len(body)), (0, 24), (2, 17), (590, 640)]
        for pat in ("rYn", "BDHV", "ACGTACGTACGTACGTACGTACG"):
            for K in (0, 1, 3):
                if K >= len(pat):
                    continue
                for strands in STRANDS:
                    off, hits = p.check(pat, whole, K, strands, "case")
                assert len(hits) > 0
                one = p.use["private"]
                assert rows(one.find_approx(pat.lower(), whole, K)[1]) == rows(one.find_approx(pat.upper(), whole, K)[1])
        # ACGT six times under the 23-mer: the lowercase run 3..11 is searched like any other base
        assert rows(p.check("ACGTACGTACGTACGTACGTACG", [(0, 24)], 3, "+")[1]) == [(0, 0, 0)]


# ---------------------------------------------------------------------------------------------
# 7. cohort
# ---------------------------------------------------------------------------------------------
class FindCohort:
    """The 5-kind cohort of cohortlib.make_cohort_inputs, shared and private readers mixed, sample 5 = sample 1's reader again."""

    def __init__(self, ctx):
        self.rfa, targets = cohortlib.make_cohort_inputs()
        self.truths = [targets[k][1] for k in cohortlib.KINDS]
        self.recs = [ctx.compress(self.rfa, targets[k][0]) for k in cohortlib.KINDS]
        self.ref = ctx.open_reference(self.rfa)
        self.private = [i % 2 == 1 for i in range(5)]
        self.readers = [ctx.open_reader(r, self.rfa) if pv else self.ref.open_reader(r) for pv, r in zip(self.private, self.recs)]
        self.cohort = sccg.Cohort(self.readers + [self.readers[1]])
        self.truths6 = self.truths + [self.truths[1]]
        self.length = [len(t) for t in self.truths6]

    def close(self):
        self.cohort.close()
        for rd in self.readers:
            rd.close()
        self.ref.close()

    def regions(self, s, n, hi, seed):
        return [(b, e) for _, b, e in self.items(n, hi, seed, sample=s)]

    def items(self, n, hi, seed, sample=None):
        rng = random.Random(seed)
        out = []
        for _ in range(n):
            s = rng.randrange(6) if sample is None else sample
            ln = rng.randint(0, hi)
            b = rng.randrange(self.length[s] - ln + 1)
            out.append((s, b, b + ln))
        return out


@pytest.fixture(scope="module")
def case(ctx):
    c = FindCohort(ctx)
    yield c
    c.close()


def cut_8mer(case):
    seq = case.truths[0]
    return seq[cut_places(seq[30_000:30_400], 8)[5] + 30_000:][:8].decode().upper()


def test_cohort_find_approx(ctx, case):
    assert any(case.private) and not all(case.private)
    assert any(cohortlib.n_line(r) != b"," for r in case.recs)
    items = case.items(1500, 400, 1) + [(2, 9_990, 10_020), (2, 24_990, 25_080), (2, 39_000, 42_000)]   # the N-run sample's runs
    for pat, K, strands in (("GAATTC", 1, "both"), (cut_8mer(case), 2, "both"), ("NNNNNGG", 1, "both"), ("GAATTC", 1, "-"),
                            ("TATAWAWR", 2, "+")):
        off, hits = fa.check_cohort(case.cohort, case.truths6, pat, items, K, strands, "cohort")
        assert len(hits) > 0 and (hits[:, 2] > 0).any(), pat
        for s in range(6):   # the readers' own answers are the cohort's
            idx = [k for k, it in enumerate(items) if it[0] == s]
            roff, rhit = case.cohort.readers[s].find_approx(pat, [items[k][1:] for k in idx], K, strands)
            assert np.array_equal(rhit, np.concatenate([hits[off[k]:off[k + 1]] for k in idx])), (pat, s)
            assert np.array_equal(np.diff(roff), np.array([off[k + 1] - off[k] for k in idx])), (pat, s)
    for n in (0, 1, 63, 64, 65):
        fa.check_cohort(case.cohort, case.truths6, "GGNCC", case.items(n, 400, 10 + n), 1, "both", f"cohort n={n}")


# ---------------------------------------------------------------------------------------------
# 8. the reported mismatches on the GPU's own bases
# ---------------------------------------------------------------------------------------------
def test_every_row_counts_its_mismatches_on_the_gpus_own_bases(case):
    rd = case.readers[2]   # the N-run sample
    L = case.length[2]
    sparse, dense = [(0, L), (9_000, 26_000)], [(9_900, 10_400), (24_900, 25_400)]   # (both over the sample's N runs)
    for pat, regs in (("GAATTCGA", sparse), ("NNNNNGG", dense), ("RYRYSW", dense), ("AC" + "N" * 16 + "GT", dense)):
        for K in (1, 2):
            off, hits = rd.find_approx(pat, regs, K)
            assert len(hits) > 0 and (hits[:, 2] == K).any()
            fa.check_independent(lambda regs: rd.fetch_encoded(regs, "index"), pat, hits, K, pat)
    items = case.items(300, 2000, 6)
    off, hits = case.cohort.find_approx("CCWGG", items, 1)
    samp = np.repeat(np.array([it[0] for it in items]), np.diff(off))
    assert len(hits) > 10
    fa.check_independent(lambda regs: case.cohort.fetch_encoded([(int(s), b, e) for s, (b, e) in zip(samp, regs)], "index"), "CCWGG", hits, 1,
                         "cohort")


# ---------------------------------------------------------------------------------------------
# 9. K = 0 is find
# ---------------------------------------------------------------------------------------------
def test_k0_is_find(case):
    rd = case.readers[0]
    seq = case.truths[0]
    at = cut_places(seq[20_000:21_000], 64)[0] + 20_000
    mer64 = seq[at:at + 64].decode().upper()
    g = next(j for j in range(at + 100, at + 5000) if seq[j + 21:j + 23].upper() == b"GG" and cut_places(seq[j:j + 23], 23))
    guide = seq[g:g + 20].decode().upper() + "NGG"   # a guide + PAM that is there
    regs = [(0, case.length[0]), (at, at + 64), (at + 1, at + 64), (5, 5)] + case.regions(0, 200, 3000, 9)
    for pat in ("GAATTC", "N", mer64, guide, "rYn", "CCWGG"):
        for strands in ("both", "-"):
            off, hits = rd.find_approx(pat, regs, 0, strands)
            foff, fhit = rd.find(pat, regs, strands)
            assert np.array_equal(off, foff) and np.array_equal(hits[:, :2], fhit) and not hits[:, 2].any(), pat
            assert len(hits) > 0 or strands == "-", pat
    items = case.items(200, 3000, 12)
    off, hits = case.cohort.find_approx("GAATTC", items, 0)
    foff, fhit = case.cohort.find("GAATTC", items)
    assert np.array_equal(off, foff) and np.array_equal(hits[:, :2], fhit) and not hits[:, 2].any() and len(hits) > 0


# ---------------------------------------------------------------------------------------------
# 10. tensor forms
# ---------------------------------------------------------------------------------------------
def test_find_approx_tensor(case):
    import torch
    rd = case.readers[2]
    regs = case.regions(2, 100, 3000, 3) + [(7, 7), (0, case.length[2])]
    eoff, ehit = fa.want(case.truths[2], "GGNCCA", regs, 1)
    off, hits = rd.find_approx_tensor("GGNCCA", regs, 1)
    assert off.dtype == torch.int64 and hits.dtype == torch.int64 and off.device == torch.device("cuda", 0) and hits.is_cuda
    assert tuple(hits.shape) == (len(ehit), 3)
    assert off.cpu().tolist() == eoff.tolist() and np.array_equal(hits.cpu().numpy(), ehit) and len(ehit) > 20
    noff, nhit = rd.find_approx("GGNCCA", regs, 1)
    assert np.array_equal(noff, off.cpu().numpy()) and np.array_equal(nhit, hits.cpu().numpy())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        off2, hits2 = rd.find_approx_tensor("GGNCCA", regs, 1, stream=s)
    assert torch.equal(off2, off) and torch.equal(hits2, hits)   # a second identical call: the same bytes
    assert rd.find_approx("GGNCCA", regs, 1)[1].tobytes() == nhit.tobytes()
    items = case.items(100, 3000, 4)
    eoff, ehit = fa.want(case.truths6, "GAATTC", items, 1, "-")
    off, hits = case.cohort.find_approx_tensor("GAATTC", items, 1, "-")
    assert off.cpu().tolist() == eoff.tolist() and np.array_equal(hits.cpu().numpy(), ehit)
    off, hits = rd.find_approx_tensor("GAATTC", [], 1)
    assert off.cpu().tolist() == [0] and tuple(hits.shape) == (0, 3)
    off, hits = rd.find_approx_tensor("GAGAGAGAGAGAGAGAGAGAGAGA", [(0, 5000), (3, 4)], 1)   # no hit at all
    assert off.cpu().tolist() == [0, 0, 0] and tuple(hits.shape) == (0, 3)
    with pytest.raises(ValueError):
        rd.find_approx("ACG", [(0, 5)], 1, strands="x")


# ---------------------------------------------------------------------------------------------
# 11. size query, capacity, alignment
# ---------------------------------------------------------------------------------------------
def test_size_query_capacity_alignment(case):
    import torch
    dev = torch.device("cuda", 0)
    lib, rd, co = case.readers[0].lib, case.readers[0], case.cohort
    regs = [(5, 5), (100, 9000), (3, 4), (50_000, case.length[0])]
    pat, K = b"GGNCCA", 1
    eoff, ehit = fa.want(case.truths[0], pat, regs, K)
    need = len(ehit)
    assert need >= 8 and (ehit[:, 2] > 0).any()
    arr = (sccg.Region * len(regs))(*regs)
    items = (sccg.CohortRegion * len(regs))(*[(b, e, 0, 0) for b, e in regs])
    n = ctypes.c_size_t(0)
    for call, ptr, a in ((lib.sccg_reader_find_approx_device, rd.ptr, arr), (lib.sccg_cohort_find_approx_device, co.ptr, items)):
        def run(d_off, d_hit, cap, flags=3):
            return call(ptr, pat, len(pat), a, len(regs), flags, K, d_off, d_hit, cap, ctypes.byref(n), None)
        d_off = torch.full((len(regs) + 1 + 4,), 77, dtype=torch.int64, device=dev)
        d_hit = torch.full((need + 4, 3), 77, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        n.value = 0
        assert run(None, None, 0) == 0 and n.value == need   # size query
        assert run(d_off.data_ptr(), None, 0) == 0 and n.value == need
        torch.cuda.synchronize()
        assert bool((d_off == 77).all().item())   # a size query writes nothing
        n.value = 0
        assert run(d_off.data_ptr(), d_hit.data_ptr(), need - 1) == E["SCCG_E_NOMEM"]
        assert n.value == need and str(need) in lib.sccg_last_error(rd.ctx.ptr).decode()
        torch.cuda.synchronize()
        assert bool((d_hit[need - 1:] == 77).all().item())   # nothing past cap
        assert run(d_off.data_ptr() + 4, d_hit.data_ptr(), need) == E["SCCG_E_INVALID"]
        assert "d_off" in lib.sccg_last_error(rd.ctx.ptr).decode()
        assert run(d_off.data_ptr(), d_hit.data_ptr() + 4, need) == E["SCCG_E_INVALID"]
        assert "d_hit" in lib.sccg_last_error(rd.ctx.ptr).decode()
        d_off.fill_(77)
        d_hit.fill_(77)
        torch.cuda.synchronize()   # (the fills run on torch's stream, the call on the context's own, which does not wait for it)
        assert run(d_off.data_ptr(), d_hit.data_ptr(), need) == 0 and n.value == need   # exact
        assert d_off.cpu().tolist() == eoff.tolist() + [77] * 4
        assert np.array_equal(d_hit.cpu().numpy()[:need], ehit) and bool((d_hit[need:] == 77).all().item())   # the guard rows
        first = d_hit.cpu().numpy().tobytes()
        assert run(d_off.data_ptr(), d_hit.data_ptr(), need) == 0 and d_hit.cpu().numpy().tobytes() == first   # byte-identical
        d_hit.fill_(77)   # without offsets; flags 0 is the forward strand
        torch.cuda.synchronize()
        assert run(None, d_hit.data_ptr(), need + 4, flags=0) == 0
        fwd = ehit[ehit[:, 1] == 0]
        assert n.value == len(fwd) and np.array_equal(d_hit.cpu().numpy()[:len(fwd)], fwd) and bool((d_hit[len(fwd):] == 77).all().item())


# ---------------------------------------------------------------------------------------------
# 12. errors: their order, status and named offender; nothing is written
# ---------------------------------------------------------------------------------------------
def expect(rc_name, text, call):
    with pytest.raises(sccg.SccgError) as ei:
        call()
    assert ei.value.rc == E[rc_name] and text in str(ei.value), str(ei.value)


def test_errors_write_nothing(ctx, case):
    import torch
    dev = torch.device("cuda", 0)
    rd, co, L = case.readers[0], case.cohort, case.length[0]
    lib = rd.lib
    I = E["SCCG_E_INVALID"]
    expect("SCCG_E_INVALID", "pattern byte 2", lambda: rd.find_approx("ACXG", [(0, 10)], 1))
    expect("SCCG_E_INVALID", "0 letters", lambda: rd.find_approx("", [(0, 10)], 0))
    expect("SCCG_E_INVALID", "65 letters", lambda: co.find_approx_tensor("A" * 65, [(0, 0, 10)], 1))
    for K, pat in ((16, "A" * 20), (4, "ACGT"), (1, "A"), (64, "A" * 64), (1 << 31, "ACGTACGT"), (0xFFFFFFFF, "ACGTACGT")):
        for call in (lambda: rd.find_approx(pat, [(0, 10)], K), lambda: co.find_approx(pat, [(0, 0, 10)], K),
                     lambda: rd.find_approx_tensor(pat, [(0, 10)], K), lambda: co.find_approx_tensor(pat, [(0, 0, 10)], K)):
            expect("SCCG_E_INVALID", "mismatches", call)
            expect("SCCG_E_INVALID", str(K), call)
    expect("SCCG_E_INVALID", "region 1", lambda: rd.find_approx("ACG", [(0, 5), (5, L + 1), (-1, 3)], 1))
    expect("SCCG_E_INVALID", "region 1", lambda: co.find_approx("ACG", [(0, 0, 5), (1, 0, 5, True)], 1))   # flag bit 0
    expect("SCCG_E_INVALID", "sample 9", lambda: co.find_approx("ACG", [(0, 0, 5), (9, 0, 5)], 1))
    # raw calls over sentinel-filled outputs
    hoff = (ctypes.c_int64 * 4)(*[77] * 4)
    buf = sccg.Buf()
    n = ctypes.c_size_t(77)
    d_off = torch.full((8,), 77, dtype=torch.int64, device=dev)
    d_hit = torch.full((64, 3), 77, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ok = (sccg.Region * 2)((20_000, 20_010), (20_005, 20_009))
    bad_r = (sccg.Region * 2)((0, 10), (5, L + 1))
    okc = (sccg.CohortRegion * 2)((0, 5, 0, 0), (0, 5, 1, 0))
    flag1 = (sccg.CohortRegion * 2)((0, 5, 0, 0), (0, 5, 1, 1))
    badsample = (sccg.CohortRegion * 2)((0, 5, 0, 0), (0, 5, 9, 0))
    msg = lambda: lib.sccg_last_error(ctx.ptr).decode()
    dev_args = (d_off.data_ptr(), d_hit.data_ptr(), 64, ctypes.byref(n), None)
    odd_args = (d_off.data_ptr() + 4, d_hit.data_ptr(), 64, ctypes.byref(n), None)
    R, RD, C, CD = lib.sccg_reader_find_approx, lib.sccg_reader_find_approx_device, lib.sccg_cohort_find_approx, lib.sccg_cohort_find_approx_device
    # the pattern before the flags, the flags before K, K before the alignment and the regions
    assert R(rd.ptr, b"AXG", 3, bad_r, 2, 4, 9, hoff, ctypes.byref(buf)) == I and "pattern byte 1" in msg()
    assert R(rd.ptr, b"ACG", 3, bad_r, 2, 4, 9, hoff, ctypes.byref(buf)) == I and "flag" in msg() and "mismatches" not in msg()
    assert R(rd.ptr, b"ACG", 3, bad_r, 2, 3, 9, hoff, ctypes.byref(buf)) == I and "9 mismatches" in msg()
    assert R(rd.ptr, b"ACG", 3, bad_r, 2, 3, 3, hoff, ctypes.byref(buf)) == I and "3 mismatches" in msg()   # K == m
    assert R(rd.ptr, b"ACG", 3, bad_r, 2, 3, 2, hoff, ctypes.byref(buf)) == I and "region 1" in msg()
    assert RD(rd.ptr, b"A" * 20, 20, bad_r, 2, 3, 16, *odd_args) == I and "16 mismatches" in msg()
    assert RD(rd.ptr, b"A" * 20, 20, bad_r, 2, 3, 1 << 31, *odd_args) == I and "2147483648 mismatches" in msg()
    assert RD(rd.ptr, b"A" * 20, 20, bad_r, 2, 3, 15, *odd_args) == I and "d_off" in msg()
    assert RD(rd.ptr, b"A" * 20, 20, bad_r, 2, 3, 15, *dev_args) == I and "region 1" in msg()
    assert RD(rd.ptr, b"A" * 20, 20, bad_r, 2, 3, 15, None, None, 0, ctypes.byref(n), None) == I   # size query
    assert RD(rd.ptr, b"ACG", 3, ok, 2, 3, 1, d_off.data_ptr(), d_hit.data_ptr(), 64, None, None) == I
    assert R(rd.ptr, None, 3, ok, 2, 3, 1, hoff, ctypes.byref(buf)) == I and "pattern" in msg()
    assert R(rd.ptr, b"ACG", 3, ok, 2, 3, 1, hoff, None) == I
    assert R(rd.ptr, b"ACG", 3, None, 2, 3, 1, hoff, ctypes.byref(buf)) == I
    for regs, word in ((flag1, "flag"), (badsample, "sample 9")):
        assert C(co.ptr, b"ACG", 3, regs, 2, 3, 1, hoff, ctypes.byref(buf)) == I and word in msg() and "region 1" in msg(), msg()
        assert C(co.ptr, b"ACG", 3, regs, 2, 3, 3, hoff, ctypes.byref(buf)) == I and "mismatches" in msg()   # K first
        assert CD(co.ptr, b"ACG", 3, regs, 2, 3, 1, *dev_args) == I and word in msg()
        assert CD(co.ptr, b"ACG", 3, regs, 2, 3, 1, *odd_args) == I and "d_off" in msg()
        assert CD(co.ptr, b"ACG", 3, regs, 2, 8, 7, *odd_args) == I and "find flag" in msg()
        assert CD(co.ptr, b"ACG", 3, regs, 2, 3, 1, None, None, 0, ctypes.byref(n), None) == I
    assert C(co.ptr, b"ACG", 3, okc, 2, 3, 1, hoff, None) == I
    torch.cuda.synchronize()
    assert list(hoff) == [77] * 4 and not buf.data and buf.len == 0 and n.value == 77
    assert bool((d_off == 77).all().item()) and bool((d_hit == 77).all().item())
    # and the good calls over the same buffers work
    eoff, ehit = fa.want(case.truths[0], "ACG", [(20_000, 20_010), (20_005, 20_009)], 2)
    k = len(ehit)
    assert RD(rd.ptr, b"ACG", 3, ok, 2, 3, 2, *dev_args) == 0 and n.value == k and 0 < k <= 40
    assert d_off[:3].cpu().tolist() == eoff.tolist()
    assert np.array_equal(d_hit.cpu().numpy()[:k], ehit) and bool((d_hit[k:] == 77).all().item())
    assert R(rd.ptr, b"ACG", 3, ok, 2, 3, 2, hoff, ctypes.byref(buf)) == 0
    assert list(hoff)[:3] == eoff.tolist() and buf.len == 24 * k
    lib.sccg_buf_free(ctypes.byref(buf))


# ---------------------------------------------------------------------------------------------
# 13. launches
# ---------------------------------------------------------------------------------------------
def test_launch_count_is_the_constant_design_states(ctx, case):
    """The kernels are bracketed under the profiler's fetch family; a call queues the number of launches DESIGN and
    the header state, whatever n is, for a reader and for a cohort."""
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    stated = re.search(r"a find-approx call queues \*\*(\d+) launches\*\*", text)
    assert stated, 'DESIGN states "a find-approx call queues **N launches**"'
    full = int(stated.group(1))
    header = re.sub(r"\n \* ?", " ", open(sccg.HEADER).read())
    words = {"one": 1, "two": 2, "three": 3, "four": 4, "five": 5, "six": 6}
    said = re.search(r"Find with mismatches: .*?Costs: (\w+) kernel launches \((\w+) for a size query\)", header)
    assert said and words[said.group(1)] == full, "the header states the same number"
    query = words[said.group(2)]
    assert (full, query) == (3, 2)
    lib, rd, co = ctx.lib, case.readers[1], case.cohort
    counts, queries = [], []
    m = ctypes.c_size_t()
    try:
        for n in (1, 2000):
            regs = case.regions(1, n, 300, 60 + n)
            ctx.profile(True, families=["fetch"])
            mine = got = rd.find_approx("CCWGG", regs, 1)
            prof = ctx.profile_get()
            assert set(prof) == {"fetch"}, prof
            counts.append(prof["fetch"][1])
            fa.check(got, fa.want(case.truths[1], "CCWGG", regs, 1), regs, "profiled")
            items = case.items(n, 300, 70 + n)
            ctx.profile(True, families=["fetch"])
            got = co.find_approx("CCWGG", items, 1)
            counts.append(ctx.profile_get()["fetch"][1])
            fa.check(got, fa.want(case.truths6, "CCWGG", items, 1), items, "profiled cohort")
            arr = (sccg.Region * n)(*regs)
            carr = (sccg.CohortRegion * n)(*[(b, e, s, 0) for s, b, e in items])
            for call, ptr, a, total in ((lib.sccg_reader_find_approx_device, rd.ptr, arr, len(mine[1])),
                                        (lib.sccg_cohort_find_approx_device, co.ptr, carr, len(got[1]))):
                ctx.profile(True, families=["fetch"])
                assert call(ptr, b"CCWGG", 5, a, n, 3, 1, None, None, 0, ctypes.byref(m), None) == 0
                queries.append(ctx.profile_get()["fetch"][1])
                assert m.value == total
    finally:
        ctx.profile(False)
    assert counts == [full] * 4, counts
    assert queries == [query] * 4, queries


# ---------------------------------------------------------------------------------------------
# 14. nothing else moved
# ---------------------------------------------------------------------------------------------
def test_nothing_else_moved(case):
    regions = [(0, 3000), (25_000, 26_111), (7, 8), (40_000, 41_500)]
    rd = case.readers[2]
    L = case.length[2]

    def everything():
        return [rd.fetch(regions), rd.fetch_encoded(regions, "onehot", "f16", revcomp=True), rd.fetch_encoded(regions, "index", strand=[1, 0, 1, 0]),
                [a.tobytes() for a in rd.find("GAATTC", [(0, L)] + regions)]]
    before, bytes_before = everything(), rd.device_bytes
    off, hits = rd.find_approx("GAATTC", [(0, L)] + case.regions(2, 500, 2000, 8), 1)
    rd.find_approx_tensor("NNNNNNNNNNNNNNNNNNNNNGG", [(0, L)], 4)
    case.cohort.find_approx("GAATTC", case.items(200, 2000, 5), 2)
    assert len(hits) > 10
    assert everything() == before and rd.device_bytes == bytes_before
    assert b"".join(before[0]) == b"".join(case.truths[2][b:e] for b, e in regions)
