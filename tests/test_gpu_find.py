"""Find on the GPU (sccg_reader_find*, sccg_cohort_find*): where an IUPAC pattern occurs in regions of a
sample, on either strand.

The truth is never the code under test (findlib): a regex with a lookahead over the sequence's bytes, which
are cohortlib.hand_sequence's for the hand-built records and the target's body for compressed ones.  One more
truth needs no oracle and is asserted on the GPU's own outputs: the index fetch of every reported window, on
the strand of its hit, satisfies the pattern's masks."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import cohortlib
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

    def check(self, pattern, regions, strands="both", what=""):
        """Every reader against the oracle (computed once); returns the pair."""
        regions = list(regions)
        expected = findlib.want(self.seq, pattern, regions, strands)
        for name, rd in self.use.items():
            assert rd.length == len(self.seq)
            findlib.check(rd.find(pattern, regions, strands), expected, regions, f"{what} {name} {findlib.text(pattern)} {strands}")
        return expected


def rows(hits):
    return [tuple(r) for r in np.asarray(hits).tolist()]


def cut_patterns(seq: bytes, lengths, seed):
    """A pattern of each length cut from the sequence where it holds A, C, G, T only (none: that length is left out)."""
    rng = random.Random(seed)
    out = []
    for m in lengths:
        places = [j for j in range(len(seq) - m + 1) if all(c in b"ACGTacgt" for c in seq[j:j + m])]
        if places:
            j = rng.choice(places)
            out.append(seq[j:j + m].decode().upper())
    return out


def absent_pattern(seq: bytes) -> str:
    for pat in ("CCCCCCCC", "GAGAGAGAGAGA", "TTTTCCCCAAAA", "CATCATCATCATCAT"):
        if not len(findlib.want(seq, pat, [(0, len(seq))])[1]):
            return pat
    raise AssertionError("every candidate occurs")


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
        pairs = findlib.every_pair(min(L, 120))
        patterns = cut_patterns(p.seq, (1, 2, 4, 8), 3) + [absent_pattern(p.seq)]
        assert len(patterns) >= 4, patterns
        for pat in patterns:
            for strands in STRANDS:
                off, hits = p.check(pat, pairs, strands, name)
                p.check(pat, [(0, L)], strands, name + " whole")
                if pat == patterns[-1]:
                    assert len(hits) == 0 and not off.any()
        assert len(p.check(patterns[0], pairs, "+", name)[1]) > 0
        if L > 120:
            p.check(patterns[2], [(L - 120 + b, L - e) for b in range(0, 120, 7) for e in range(0, 120 - b, 5)], "both", name + " tail pairs")


# ---------------------------------------------------------------------------------------------
# 2. tile edges without knowing the tile
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


@pytest.mark.parametrize("layout", ["one_token", "tokens_of_700"])
@pytest.mark.parametrize("body_kind", ["poly_a", "planted_c"])
def test_tile_edges(ctx, layout, body_kind):
    n = 3300
    body = b"A" * n if body_kind == "poly_a" else planted(n, 40, 8)
    rec = record([(0, n)]) if layout == "one_token" else split_record(body, 700)
    rng = random.Random(5)
    with Readers(ctx, fasta(body), rec, only=("private", "coords")) as p:
        assert p.seq == body
        regions = [(0, n), (1, n - 1), (17, 3000)] + [tuple(sorted((rng.randrange(n + 1), rng.randrange(n + 1)))) for _ in range(40)]
        for pat in ("AAAA", "A" * 64, "W" * 17):
            m = len(pat)
            for strands in (("both", "+") if pat[0] == "W" else ("+", "-")):
                off, hits = p.check(pat, regions, strands, f"{layout} {body_kind}")
                whole = hits[:off[1]]
                if body_kind == "poly_a":   # every start is a hit: len - m + 1 a strand, consecutive positions
                    per = n - m + 1
                    if pat[0] == "W":
                        k = 2 if strands == "both" else 1
                        assert len(whole) == k * per and whole[::k, 0].tolist() == list(range(per))
                        assert set(whole[:, 1].tolist()) == ({0, 1} if k == 2 else {0})
                    else:
                        assert len(whole) == (per if strands == "+" else 0)   # poly-A on the reverse strand is poly-T
                        assert strands == "-" or whole[:, 0].tolist() == list(range(per))
                elif strands != "-" or pat[0] == "W":   # hits stop at every planted C and resume behind it
                    assert len(whole) < (2 if strands == "both" else 1) * (n - m + 1)
                    assert len(whole) > 0 or m == 64
        off, hits = p.check("T" * 9, regions, "-", f"{layout} {body_kind} poly-T")   # the reverse strand's poly-A
        if body_kind == "poly_a":
            assert off[1] == n - 8 and set(hits[:, 1].tolist()) == {1}


# ---------------------------------------------------------------------------------------------
# 3. a window across boundaries
# ---------------------------------------------------------------------------------------------
MOTIF = b"GATTACAGGCTC"   # 12 letters, no palindrome, absent from the random bodies below (asserted)


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
        (560, 30),                              # 560: a target N run goes in before it; 566: another one splits ...
        (600, 12),                              # ... nothing: the motif at 600 is cut by a run in the middle
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


def test_window_across_boundaries(ctx):
    rfa, rec, hits0, runs = boundary_case()
    m = len(MOTIF)
    with Readers(ctx, rfa, rec, only=("shared", "coords")) as p:   # (a private reader takes the erased form too: checked in 1.)
        seq = p.seq
        assert seq.count(b"N") == sum(l for _, l in runs)
        found = [mm.start() for mm in re.finditer(MOTIF, seq)]
        assert len(found) == 6, found   # the seventh is cut by the N run inside it
        n_at = [mm.span() for mm in re.finditer(rb"N+", seq)]
        assert found[4] + m == n_at[0][0] and found[5] == n_at[1][1]   # directly before a run, directly behind one
        pat = MOTIF.decode()
        off, hits = p.check(pat, [(0, len(seq))], "both", "boundaries")
        assert rows(hits) == [(j, 0) for j in found]
        off, hits = p.check(findlib.revcomp_pattern(pat), [(0, len(seq))], "both", "boundaries rc")
        assert rows(hits) == [(j, 1) for j in found]
        for j in found + [n_at[2][0] - 5]:   # every begin and end around each placement
            p.check(pat, [(b, e) for b in range(max(j - 3, 0), j + 4) for e in range(j + m - 3, min(j + m + 4, len(seq) + 1))], "both",
                    f"around {j}")
        # N bases match nothing, not even N: no window inside or across a run
        s, e = n_at[1]
        assert e - s == 14
        off, hits = p.check("N" * 5, [(s, e), (s - 4, e), (s, e + 4), (s - 5, e + 5), (s - 5, s), (e, e + 5)], "+", "N run")
        assert np.diff(off).tolist() == [0, 0, 0, 2, 1, 1]
        p.check("N" * 12, findlib.every_pair(len(seq))[::53], "both", "N pattern")
        p.check("NNNNNNNNNNNNNNNNNNNNNGG", [(0, len(seq))], "both", "guide + PAM")


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
    m, pat = len(MOTIF), MOTIF.decode()
    with Readers(ctx, fasta(body), split_record(body, 333), only=("private", "coords")) as p:
        assert p.seq == body
        j = sites[3]
        off, hits = p.check(pat, [(j, j + m), (j, j + m - 1), (j + 1, j + m), (j - 1, j + m), (j, j + m + 1), (j, j), (j + m, j + m)], "both",
                            "ends")
        assert np.diff(off).tolist() == [1, 0, 0, 1, 1, 0, 0] and rows(hits) == [(j, 0)] * 3
        # repeated, overlapping, unordered
        regs = [(sites[9], sites[12] + m), (sites[2], sites[5] + m), (sites[9], sites[12] + m), (sites[10] + 1, sites[12] + m), (0, 5000),
                (sites[2], sites[5] + m)]
        off, hits = p.check(pat, regs, "both", "repeated overlapping unordered")
        assert np.diff(off).tolist() == [4, 4, 4, 2, len(sites), 4]
        # 2,000 one-motif regions in one call, in a shuffled order, every third one a base too short
        rng = random.Random(2)
        many = [(s, s + m - (k % 3 == 2)) for k, s in enumerate(rng.choices(sites, k=2000))]
        off, hits = p.check(pat, many, "both", "2,000 regions")
        assert off[-1] == len(hits) == sum(1 for b, e in many if e - b == m)
        # n == 0
        off, hits = p.check(pat, [], "both", "no region")
        assert off.tolist() == [0] and hits.shape == (0, 2)
        # regions that own no candidate at the front, in the middle and at the end of the list
        empties = [(5, 5), (0, m - 1), (sites[0], sites[1] + m), (7, 7), (9, 9 + m - 1), (5000, 5000), (sites[4], sites[4] + m), (3, 3),
                   (5000 - m + 1, 5000)]
        off, hits = p.check(pat, empties, "both", "empty regions")
        assert off.tolist() == [0, 0, 0, 2, 2, 2, 2, 3, 3, 3]
        off, hits = p.check(pat, [(4, 4), (0, 3), (5000, 5000)], "both", "only empty regions")
        assert off.tolist() == [0, 0, 0, 0] and len(hits) == 0
        p.check(pat, [(0, 5000)] * 3 + [(0, 0)] + [(0, 5000)], "-", "nothing on this strand")


# ---------------------------------------------------------------------------------------------
# 5. both strands
# ---------------------------------------------------------------------------------------------
def test_both_strands(ctx):
    body = bytearray(random_body(4000, 77).replace(b"GAATTC", b"GAATTA"))
    pal = list(range(100, 3900, 313))
    for at in pal:
        body[at:at + 6] = b"GAATTC"
    asym, rc = MOTIF, findlib.revcomp_pattern(MOTIF).encode()
    for k, at in enumerate(range(50, 3900, 411)):
        body[at:at + 12] = asym if k % 2 == 0 else rc
    body = bytes(body)
    sites_f = [mm.start() for mm in re.finditer(asym, body)]
    sites_r = [mm.start() for mm in re.finditer(rc, body)]
    assert len(sites_f) >= 4 and len(sites_r) >= 4
    with Readers(ctx, fasta(body), split_record(body, 450), only=("shared",)) as p:
        whole = [(0, len(body))]
        off, hits = p.check("GAATTC", whole + [(a, a + 6) for a in pal], "both", "palindrome")
        found = [mm.start() for mm in re.finditer(b"GAATTC", body)]
        assert rows(hits[:off[1]]) == [(j, s) for j in found for s in (0, 1)]   # two rows a site, forward first
        assert rows(hits[off[1]:]) == [(a, s) for a in pal for s in (0, 1)]
        assert rows(p.check("GAATTC", whole, "+", "palindrome")[1]) == [(j, 0) for j in found]
        assert rows(p.check("GAATTC", whole, "-", "palindrome")[1]) == [(j, 1) for j in found]
        off, hits = p.check(asym.decode(), whole, "both", "asymmetric")
        assert rows(hits) == sorted([(j, 0) for j in sites_f] + [(j, 1) for j in sites_r])
        # "-" alone is the reverse-complemented pattern on "+", relabelled
        rd = p.use["shared"]
        regs = whole + [(s - 2, s + 20) for s in sites_r]
        for pat in (asym.decode(), "GAATTC", "RYN", "GGNCC", "W" * 5 + "S"):
            moff, mhit = rd.find(pat, regs, "-")
            poff, phit = rd.find(findlib.revcomp_pattern(pat), regs, "+")
            assert moff.tolist() == poff.tolist() and mhit[:, 0].tolist() == phit[:, 0].tolist(), pat
            assert set(mhit[:, 1].tolist()) <= {1} and set(phit[:, 1].tolist()) <= {0} and len(mhit) > 0, pat
            p.check(pat, regs, "both", "relabelled")


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
        for letter in "ACGTURYSWKMBDHVN":
            off, hits = p.check(letter, whole, "both", "one letter")
            assert np.diff(off)[1] == 2 * 6 * len(findlib.IUPAC[letter])   # ACGT six times: a letter's set, and its complement's
            p.check(letter.lower() + "N" + letter, whole, "both", "three letters")
        for pat in ("acgt", "AcGt", "rYn", "ACGTACGTACGTACGTACGTACG", "aaccggtt", "SSWW", "BDHV", "KM"):
            for strands in STRANDS:
                off, hits = p.check(pat, whole, strands, "case")
            assert rows(p.use["private"].find(pat, whole)[1]) == rows(p.use["private"].find(pat.upper(), whole)[1])
        assert len(p.check("acgtacgt", [(0, 24)], "+")[1]) == 5   # the lowercase run 3..11 is searched like any other base


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


def test_cohort_find(ctx, case):
    assert any(case.private) and not all(case.private)
    assert any(cohortlib.n_line(r) != b"," for r in case.recs)
    items = case.items(1500, 400, 1) + [(2, 9_990, 10_020), (2, 24_990, 25_080), (2, 39_000, 42_000)]   # the N-run sample's runs
    cut = cut_patterns(case.truths[0][30_000:30_400], (8,), 4)[0]
    for pat, strands in (("GAATTC", "both"), (cut, "both"), ("NNNNNGG", "both"), ("CAG", "-"), ("TATAWAWR", "+")):
        off, hits = findlib.check_cohort(case.cohort, case.truths6, pat, items, strands, "cohort")
        assert len(hits) > 0, pat
        for s in range(6):   # the readers' own answers are the cohort's
            idx = [k for k, it in enumerate(items) if it[0] == s]
            roff, rhit = case.cohort.readers[s].find(pat, [items[k][1:] for k in idx], strands)
            assert np.array_equal(rhit, np.concatenate([hits[off[k]:off[k + 1]] for k in idx])), (pat, s)
            assert np.array_equal(np.diff(roff), np.array([off[k + 1] - off[k] for k in idx])), (pat, s)
    for n in (0, 1, 63, 64, 65):
        findlib.check_cohort(case.cohort, case.truths6, "GGNCC", case.items(n, 400, 10 + n), "both", f"cohort n={n}")
    whole = [(s, 0, case.length[s]) for s in (5, 2, 0, 3)]
    off, hits = findlib.check_cohort(case.cohort, case.truths6, "GAATTC", whole, "both", "cohort whole samples")
    assert len(hits) > 8 and np.array_equal(hits[off[0]:off[1]], case.readers[1].find("GAATTC", [(0, case.length[1])])[1])


def test_every_hit_satisfies_the_masks_on_the_gpus_own_bases(case):
    rd = case.readers[2]   # the N-run sample
    L = case.length[2]
    for pat in ("GAATTC", "NNNNNGG", "RYRYSW", "AC" + "N" * 16 + "GT"):
        off, hits = rd.find(pat, [(0, L), (9_000, 26_000)])
        assert len(hits) > 0
        findlib.check_independent(lambda regs, strand: rd.fetch_encoded(regs, "index", strand=strand), pat, hits, pat)
    items = case.items(300, 2000, 6)
    off, hits = case.cohort.find("CCWGG", items)
    samp = np.repeat(np.array([it[0] for it in items]), np.diff(off))
    assert len(hits) > 10
    findlib.check_independent(
        lambda regs, strand: case.cohort.fetch_encoded([(int(s), b, e, st) for s, (b, e), st in zip(samp, regs, strand)], "index"), "CCWGG",
        hits, "cohort")


# ---------------------------------------------------------------------------------------------
# 8. tensor and device forms
# ---------------------------------------------------------------------------------------------
def test_find_tensor(case):
    import torch
    rd = case.readers[2]
    regs = case.regions(2, 100, 3000, 3) + [(7, 7), (0, case.length[2])]
    eoff, ehit = findlib.want(case.truths[2], "GGNCC", regs)
    off, hits = rd.find_tensor("GGNCC", regs)
    assert off.dtype == torch.int64 and hits.dtype == torch.int64 and off.device == torch.device("cuda", 0) and hits.is_cuda
    assert off.cpu().tolist() == eoff.tolist() and np.array_equal(hits.cpu().numpy(), ehit) and len(ehit) > 20
    noff, nhit = rd.find("GGNCC", regs)
    assert np.array_equal(noff, off.cpu().numpy()) and np.array_equal(nhit, hits.cpu().numpy())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        off2, hits2 = rd.find_tensor("GGNCC", regs, stream=s)
    assert torch.equal(off2, off) and torch.equal(hits2, hits)   # a second identical call: the same bytes
    assert rd.find("GGNCC", regs)[1].tobytes() == nhit.tobytes()
    items = case.items(100, 3000, 4)
    eoff, ehit = findlib.want(case.truths6, "GAATTC", items, "-")
    off, hits = case.cohort.find_tensor("GAATTC", items, "-")
    assert off.cpu().tolist() == eoff.tolist() and np.array_equal(hits.cpu().numpy(), ehit)
    off, hits = rd.find_tensor("GAATTC", [])
    assert off.cpu().tolist() == [0] and tuple(hits.shape) == (0, 2)
    off, hits = rd.find_tensor("GAGAGAGAGAGAGAGAGAGAGAGA", [(0, 5000), (3, 4)])   # no hit at all
    assert off.cpu().tolist() == [0, 0, 0] and tuple(hits.shape) == (0, 2)


def test_size_query_capacity_alignment(case):
    import torch
    dev = torch.device("cuda", 0)
    lib, rd, co = case.readers[0].lib, case.readers[0], case.cohort
    regs = [(5, 5), (100, 9000), (3, 4), (50_000, case.length[0])]
    pat = b"GGNCC"
    eoff, ehit = findlib.want(case.truths[0], pat, regs)
    need = len(ehit)
    assert need >= 8
    arr = (sccg.Region * len(regs))(*regs)
    items = (sccg.CohortRegion * len(regs))(*[(b, e, 0, 0) for b, e in regs])
    n = ctypes.c_size_t(0)
    for call, ptr, a in ((lib.sccg_reader_find_device, rd.ptr, arr), (lib.sccg_cohort_find_device, co.ptr, items)):
        def run(d_off, d_hit, cap, flags=3):
            return call(ptr, pat, len(pat), a, len(regs), flags, d_off, d_hit, cap, ctypes.byref(n), None)
        d_off = torch.full((len(regs) + 1 + 4,), 77, dtype=torch.int64, device=dev)
        d_hit = torch.full((need + 4, 2), 77, dtype=torch.int64, device=dev)
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
# 9. errors: their order, status and named offender; nothing is written
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
    expect("SCCG_E_INVALID", "pattern byte 2", lambda: rd.find("ACXG", [(0, 10)]))
    expect("SCCG_E_INVALID", "pattern byte 0", lambda: rd.find(" ACG", [(0, 10)]))
    expect("SCCG_E_INVALID", "pattern byte 3", lambda: co.find(b"ACG\x00", [(0, 0, 10)]))
    expect("SCCG_E_INVALID", "0 letters", lambda: rd.find("", [(0, 10)]))
    expect("SCCG_E_INVALID", "65 letters", lambda: rd.find("A" * 65, [(0, 10)]))
    expect("SCCG_E_INVALID", "65 letters", lambda: co.find_tensor("A" * 65, [(0, 0, 10)]))
    # the pattern before the regions; a bad region, flag and sample named as for segments
    expect("SCCG_E_INVALID", "pattern byte 1", lambda: rd.find("AXG", [(0, 10), (5, L + 1)]))
    expect("SCCG_E_INVALID", "region 1", lambda: rd.find("ACG", [(0, 5), (5, L + 1), (-1, 3)]))
    expect("SCCG_E_INVALID", "region 0", lambda: rd.find("ACG", [(-1, 3)]))
    expect("SCCG_E_INVALID", "region 2", lambda: rd.find_tensor("ACG", [(0, 5), (5, 5), (9, 8)]))
    expect("SCCG_E_INVALID", "region 1", lambda: co.find("ACG", [(0, 0, 5), (1, 0, 5, True)]))   # flag bit 0
    expect("SCCG_E_INVALID", "flag", lambda: co.find("ACG", [(1, 0, 5, True)]))
    expect("SCCG_E_INVALID", "sample 9", lambda: co.find("ACG", [(0, 0, 5), (9, 0, 5)]))
    expect("SCCG_E_INVALID", "sample -1", lambda: co.find("ACG", [(-1, 0, 5)]))
    expect("SCCG_E_INVALID", "region 1", lambda: co.find("ACG", [(0, 0, 5), (3, 0, case.length[3] + 1)]))
    expect("SCCG_E_INVALID", "pattern byte 0", lambda: co.find("!", [(9, 0, 5)]))
    with pytest.raises(ValueError):
        rd.find("ACG", [(0, 5)], strands="x")
    # raw calls over sentinel-filled outputs
    hoff = (ctypes.c_int64 * 4)(*[77] * 4)
    buf = sccg.Buf()
    n = ctypes.c_size_t(77)
    d_off = torch.full((8,), 77, dtype=torch.int64, device=dev)
    d_hit = torch.full((64, 2), 77, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ok = (sccg.Region * 2)((20_000, 20_010), (20_005, 20_009))
    bad_r = (sccg.Region * 2)((0, 10), (5, L + 1))
    okc = (sccg.CohortRegion * 2)((0, 5, 0, 0), (0, 5, 1, 0))
    flag1 = (sccg.CohortRegion * 2)((0, 5, 0, 0), (0, 5, 1, 1))
    flag2 = (sccg.CohortRegion * 2)((0, 5, 0, 0), (0, 5, 1, 2))
    badsample = (sccg.CohortRegion * 2)((0, 5, 0, 0), (0, 5, 9, 0))
    badrange = (sccg.CohortRegion * 2)((0, 5, 0, 0), (6, 5, 1, 0))
    msg = lambda: lib.sccg_last_error(ctx.ptr).decode()
    dev_args = (d_off.data_ptr(), d_hit.data_ptr(), 64, ctypes.byref(n), None)
    for flags in (4, 8, 7, 1 << 31):   # an unknown flag bit: before the regions, behind the pattern
        assert lib.sccg_reader_find(rd.ptr, b"ACG", 3, bad_r, 2, flags, hoff, ctypes.byref(buf)) == I and "flag" in msg()
        assert lib.sccg_reader_find(rd.ptr, b"AXG", 3, bad_r, 2, flags, hoff, ctypes.byref(buf)) == I and "pattern byte 1" in msg()
        assert lib.sccg_cohort_find_device(co.ptr, b"ACG", 3, flag1, 2, flags, *dev_args) == I and "find flag" in msg()
    assert lib.sccg_reader_find(rd.ptr, b"ACG", 3, bad_r, 2, 3, hoff, ctypes.byref(buf)) == I and "region 1" in msg()
    assert lib.sccg_reader_find(rd.ptr, b"ACG", 3, None, 2, 3, hoff, ctypes.byref(buf)) == I
    assert lib.sccg_reader_find(rd.ptr, None, 3, ok, 2, 3, hoff, ctypes.byref(buf)) == I and "pattern" in msg()
    assert lib.sccg_reader_find(rd.ptr, b"ACG", 3, ok, 2, 3, hoff, None) == I
    assert lib.sccg_reader_find_device(rd.ptr, b"ACG", 3, bad_r, 2, 3, *dev_args) == I
    assert lib.sccg_reader_find_device(rd.ptr, b"ACG", 3, bad_r, 2, 3, None, None, 0, ctypes.byref(n), None) == I   # size query
    assert lib.sccg_reader_find_device(rd.ptr, b"ACG", 3, ok, 2, 3, d_off.data_ptr(), d_hit.data_ptr(), 64, None, None) == I
    assert lib.sccg_reader_find_device(rd.ptr, b"ACG", 3, bad_r, 2, 3, d_off.data_ptr() + 4, d_hit.data_ptr(), 64, ctypes.byref(n), None) == I
    assert "d_off" in msg()   # (the alignment before the regions)
    assert lib.sccg_reader_find_device(rd.ptr, b"A!G", 3, ok, 2, 3, d_off.data_ptr() + 4, d_hit.data_ptr(), 64, ctypes.byref(n), None) == I
    assert "pattern byte 1" in msg()   # (the pattern before the alignment)
    for regs, word in ((flag2, "flag"), (flag1, "flag"), (badsample, "sample 9"), (badrange, "outside")):
        assert lib.sccg_cohort_find(co.ptr, b"ACG", 3, regs, 2, 3, hoff, ctypes.byref(buf)) == I, word
        assert word in msg() and "region 1" in msg(), msg()
        assert lib.sccg_cohort_find_device(co.ptr, b"ACG", 3, regs, 2, 3, *dev_args) == I, word
        assert lib.sccg_cohort_find_device(co.ptr, b"ACG", 3, regs, 2, 3, None, None, 0, ctypes.byref(n), None) == I, word
    assert lib.sccg_cohort_find(co.ptr, b"ACG", 3, None, 2, 3, hoff, ctypes.byref(buf)) == I
    assert lib.sccg_cohort_find(co.ptr, b"ACG", 3, okc, 2, 3, hoff, None) == I
    torch.cuda.synchronize()
    assert list(hoff) == [77] * 4 and not buf.data and buf.len == 0 and n.value == 77
    assert bool((d_off == 77).all().item()) and bool((d_hit == 77).all().item())
    # and the good calls over the same buffers work
    eoff, ehit = findlib.want(case.truths[0], "NN", [(20_000, 20_010), (20_005, 20_009)])
    k = len(ehit)
    assert lib.sccg_reader_find_device(rd.ptr, b"NN", 2, ok, 2, 3, *dev_args) == 0 and n.value == k and 0 < k <= 24
    assert d_off[:3].cpu().tolist() == eoff.tolist()
    assert np.array_equal(d_hit.cpu().numpy()[:k], ehit) and bool((d_hit[k:] == 77).all().item())
    assert lib.sccg_reader_find(rd.ptr, b"NN", 2, ok, 2, 3, hoff, ctypes.byref(buf)) == 0
    assert list(hoff)[:3] == eoff.tolist() and buf.len == 16 * k
    lib.sccg_buf_free(ctypes.byref(buf))


# ---------------------------------------------------------------------------------------------
# 10. launches
# ---------------------------------------------------------------------------------------------
def test_launch_count_is_the_constant_design_states(ctx, case):
    """The kernels are bracketed under the profiler's fetch family (its table is closed); a call queues the number
    of launches DESIGN states, whatever n is, for a reader and for a cohort."""
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    stated = re.search(r"a find call queues \*\*(\d+) launches\*\*", text)
    assert stated, 'DESIGN states "a find call queues **K launches**"'
    full = int(stated.group(1))
    assert 1 <= full <= 6
    header = re.sub(r"\n \* ?", " ", open(sccg.HEADER).read())
    words = {"one": 1, "two": 2, "three": 3, "four": 4, "five": 5, "six": 6}
    said = re.search(r"Find: .*?Costs: (\w+) kernel launches \((\w+) for a size query\)", header)
    assert said and words[said.group(1)] == full, "the header states the same number"
    query = words[said.group(2)]
    lib, rd, co = ctx.lib, case.readers[1], case.cohort
    counts, queries = [], []
    m = ctypes.c_size_t()
    try:
        for n in (1, 2000):
            regs = case.regions(1, n, 300, 60 + n)
            ctx.profile(True, families=["fetch"])
            mine = got = rd.find("CCWGG", regs)
            prof = ctx.profile_get()
            assert set(prof) == {"fetch"}, prof
            counts.append(prof["fetch"][1])
            findlib.check(got, findlib.want(case.truths[1], "CCWGG", regs), regs, "profiled")
            items = case.items(n, 300, 70 + n)
            ctx.profile(True, families=["fetch"])
            got = co.find("CCWGG", items)
            counts.append(ctx.profile_get()["fetch"][1])
            findlib.check(got, findlib.want(case.truths6, "CCWGG", items), items, "profiled cohort")
            arr = (sccg.Region * n)(*regs)
            ctx.profile(True, families=["fetch"])
            assert lib.sccg_reader_find_device(rd.ptr, b"CCWGG", 5, arr, n, 3, None, None, 0, ctypes.byref(m), None) == 0
            queries.append(ctx.profile_get()["fetch"][1])
            assert m.value == len(mine[1])
    finally:
        ctx.profile(False)
    assert counts == [full] * 4, counts
    assert queries == [query] * 2, queries


# ---------------------------------------------------------------------------------------------
# 11. the fetches are what they were
# ---------------------------------------------------------------------------------------------
def test_fetches_are_what_they_were(case):
    regions = [(0, 3000), (25_000, 26_111), (7, 8), (40_000, 41_500)]
    rd = case.readers[2]

    def everything():
        return [rd.fetch(regions), rd.fetch_encoded(regions, "onehot", "f16", revcomp=True), rd.fetch_encoded(regions, "index", strand=[1, 0, 1, 0])]
    before, bytes_before = everything(), rd.device_bytes
    off, hits = rd.find("GAATTC", [(0, case.length[2])] + case.regions(2, 500, 2000, 8))
    rd.find_tensor("NNNNNNNNNNNNNNNNNNNNNGG", [(0, case.length[2])])
    assert len(hits) > 10
    assert everything() == before and rd.device_bytes == bytes_before
    assert b"".join(before[0]) == b"".join(case.truths[2][b:e] for b, e in regions)
