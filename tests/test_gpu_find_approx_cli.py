"""`bin/fetch --find-approx <K> <PATTERN> <record_file> <reference_file> <region>...` on a hand-written record: a
line `>begin-end` per region, then `pos strand mismatches bases` per hit -- 1-based positions, `+` / `-`, the
window as the sample carries it on the forward strand; K = 0 is `--find` with the extra column, and `--find`
itself prints what it printed.  (The usage errors need no GPU: test_find_approx_cpu.py.)"""
import os
import subprocess

import pytest

import cohortlib
import findapproxlib as fa
import findlib
from cohortlib import HAND

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FETCH = os.path.join(REPO, "sccg-genome-compression_amd", "bin", "fetch")


def cli_lines(seq: bytes, pattern: str, regions1, K=None):
    """The expected output for 1-based inclusive regions, from the oracle: K None is `--find`'s."""
    regions = [(b - 1, e) for b, e in regions1]
    off, hits = findlib.want(seq, pattern, regions) if K is None else fa.want(seq, pattern, regions, K)
    out = []
    for i, (b, e) in enumerate(regions1):
        out.append(">%d-%d" % (b, e))
        for row in hits[off[i]:off[i + 1]].tolist():
            cols = ["%d" % (row[0] + 1), "-" if row[1] else "+"] + ["%d" % d for d in row[2:]]
            out.append("\t".join(cols + [seq[row[0]:row[0] + len(pattern)].decode()]))
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("find_approx_cli")
    rfa, rec = HAND["lowercase_spanning_n"]
    (d / "compressed_genome.txt").write_bytes(rec)
    (d / "ref.fa").write_bytes(rfa)
    return str(d / "compressed_genome.txt"), str(d / "ref.fa"), cohortlib.hand_sequence(rfa, rec)


def run(*args):
    return subprocess.run([FETCH] + list(args), capture_output=True)


def test_cli_find_approx_on_a_hand_record(files):
    rec, ref, seq = files
    L = len(seq)
    assert seq == b"TACGTacgtannnncgtagattacaTACGTACGT"   # lowercase 5..24, N 10..13, the literal GATTACA at 18
    regions1 = [(1, L), (19, 25), (20, 25), (19, 24), (1, 10), (15, 15), (26, L)]
    args = ["%d-%d" % r if r[0] != r[1] else str(r[0]) for r in regions1]
    p = run("--find-approx", "1", "GATTACC", rec, ref, *args)   # one letter off the literal
    assert p.returncode == 0, p.stderr
    want = cli_lines(seq, "GATTACC", regions1, 1)
    assert p.stdout.decode().splitlines() == want
    assert want[:4] == [">1-%d" % L, "19\t+\t1\tgattaca", ">19-25", "19\t+\t1\tgattaca"] and want[4:6] == [">20-25", ">19-24"]
    p = run("--find-approx", "2", "ACGTN", rec, ref, "1-%d" % L, "1-14")   # IUPAC, both strands, across the N run within K
    assert p.returncode == 0, p.stderr
    want = cli_lines(seq, "ACGTN", [(1, L), (1, 14)], 2)
    assert p.stdout.decode().splitlines() == want
    assert "2\t+\t0\tACGTa" in want and "14\t+\t1\tncgta" in want and "13\t-\t2\tnncgt" in want and any(ln.split("\t")[1:2] == ["-"] for ln in want)
    p = run("--find-approx", "1", "ACGT", rec, ref, "%d-%d" % (L, L + 1))   # beyond the sequence
    assert p.returncode == 1 and b"outside the sequence" in p.stderr and p.stdout == b""


def test_k0_is_find_with_the_extra_column_and_find_is_unchanged(files):
    rec, ref, seq = files
    L = len(seq)
    for pat, regions1 in (("GATTACA", [(1, L), (19, 25), (20, 25)]), ("ACGTN", [(1, L), (1, 14)]), ("tgtaatc", [(1, L)])):
        args = ["%d-%d" % r for r in regions1]
        f = run("--find", pat, rec, ref, *args)
        a = run("--find-approx", "0", pat, rec, ref, *args)
        assert f.returncode == 0 and a.returncode == 0, (f.stderr, a.stderr)
        flines = f.stdout.decode().splitlines()
        assert flines == cli_lines(seq, pat, regions1) and f.stderr == b""   # what --find printed before
        with_zero = [ln if ln.startswith(">") else "\t".join(ln.split("\t")[:2] + ["0"] + ln.split("\t")[2:]) for ln in flines]
        assert a.stdout.decode().splitlines() == with_zero == cli_lines(seq, pat, regions1, 0)
        assert any(not ln.startswith(">") for ln in flines), pat
