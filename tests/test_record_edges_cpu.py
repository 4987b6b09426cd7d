"""The yardstick of the record-edge tests, pinned without a GPU (tests/recgen.py).

* the generator's labels hold by construction: `exact` run lines are ascending and disjoint, the
  oracle succeeds on `exact` and `reject_ok`, fails with the named class on single-fault `error`;
* the oracle's decompression equals the compiled reference's (status 0 / non-zero, and bytes) on
  every case the reference defines -- live where oracle/_ref is built;
* the reference's answers frozen in tests/golden/records.json.gz (which the GPU machine uses, having
  no reference) are the generator's cases and the oracle's answers.
"""
import hashlib

import pytest

import goldens
import oraclelib
import recgen
import reflib

ORC_CLASS = {3: recgen.FORMAT, 4: recgen.RANGE, 5: recgen.PARSE}
CASES = recgen.cases()
FAMILIES = sorted({c.family for c in CASES})


def oracle(c):
    """(oracle status, FASTA or None)"""
    try:
        return 0, oraclelib.decompress(c.record, c.ref_fa)
    except oraclelib.OracleError as e:
        return e.rc, None


@pytest.fixture(scope="module")
def frozen():
    return goldens.record_cases()


def test_families_and_flags():
    assert FAMILIES == list("abcdef")
    assert len(CASES) >= 1300
    flagged = [c for c in CASES if c.undefined]
    # the reference's undefined shapes: members of the run-list and fault families, nothing else
    assert flagged and all(c.family in "bf" and c.klass == recgen.ERROR for c in flagged)
    assert len(flagged) <= 40, [c.name for c in flagged]
    # the sweep puts an item start of every width on every offset, on all three lines
    widths = set()
    for off in range(0, 1101):
        c = CASES[off]
        assert c.name == f"a_off{off:04d}"
        _, lower, nline, enc = recgen.lines_of(c.record)
        for line in (lower, nline, enc):
            assert line[off:off + 1] == b"(", (c.name, line[off:off + 30])
            widths.add(line.index(b")", off) - off + 1)
    assert widths == set(range(5, 26))


def test_exact_run_lines_are_inside_the_grammar():
    """What the oracle does not check and the GPU does: starts ascending, runs disjoint."""
    for c in CASES:
        if c.klass != recgen.EXACT:
            continue
        _, lower, nline, enc = recgen.lines_of(c.record)
        for line in (lower, nline):
            end = 0
            for k, (s, l) in enumerate(recgen.parse_runs(line)):
                assert s >= end and l >= 0 and s + l < 2 ** 31, (c.name, k, s, l)
                end = s + l
            assert not re_other(line), (c.name, line[:60])


def re_other(line: bytes) -> bytes:
    """A run line's bytes that are neither an item nor a ','."""
    return recgen._ITEM.sub(b"", line).replace(b",", b"")


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_matches_the_labels(family):
    for c in CASES:
        if c.family != family:
            continue
        rc, fa = oracle(c)
        if c.klass == recgen.ERROR:
            assert rc in ORC_CLASS, (c.name, rc)
            if not c.name.startswith(recgen.TWO_FAULT):
                assert ORC_CLASS[rc] == c.expect, (c.name, rc)
        else:
            assert rc == 0 and fa is not None, (c.name, rc)


@pytest.mark.skipif(not reflib.HAVE_REF, reason="oracle/_ref not built (reference sources absent)")
@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_vs_reference(family):
    asked = [c for c in CASES if c.family == family and not c.undefined]
    answers = reflib.run_ref_decompress_many([(c.record, c.ref_fa) for c in asked])
    for c, (rrc, rfa) in zip(asked, answers):
        rc, fa = oracle(c)
        assert (rc != 0) == (rrc != 0), (c.name, rc, rrc)
        assert fa == rfa, c.name


def test_frozen_answers(frozen):
    """records.json.gz holds exactly the generator's cases, and the oracle gives its answers."""
    assert list(frozen) == [c.name for c in CASES]
    for c in CASES:
        g = frozen[c.name]
        assert (g["klass"], g["expect"], g["undefined"]) == (c.klass, c.expect, c.undefined), c.name
        assert g["record_sha256"] == hashlib.sha256(c.record).hexdigest() and g["ref_fa"] == c.ref_fa, c.name
        assert g["record"] in (None, c.record), c.name
        rc, fa = oracle(c)
        if c.undefined:
            assert g["rc"] is None and rc != 0, c.name
            continue
        assert (rc != 0) == (g["rc"] != 0), (c.name, rc, g["rc"])
        if rc == 0:
            assert (hashlib.sha256(fa).hexdigest(), len(fa)) == (g["fasta_sha256"], g["fasta_len"]), c.name


def test_probe_positions_cover_the_edges():
    """The fetch windows of the GPU tests do land on the tile edges (recgen.probe_positions)."""
    c = next(c for c in CASES if c.name == "a_off1020")
    rc, fa = oracle(c)
    seq = fa.split(b"\n", 1)[1].replace(b"\n", b"")
    pos = recgen.probe_positions(c.record, len(seq))
    assert pos[0] == 0 and pos[-1] == len(seq) and len(pos) >= 5, pos
