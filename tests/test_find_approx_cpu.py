"""Find with mismatches without a GPU: the two oracles of findapproxlib agree and, at K = 0, are findlib's; a
worked example written out by hand; the ABI's new entry points exist and refuse NULL handles; `fetch
--find-approx` refuses a malformed K, pattern or region before it touches the GPU."""
import ctypes
import os
import random
import subprocess

import numpy as np

import findapproxlib as fa
import findlib
from pkg import sccg

E = sccg.ERR_CODES
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FETCH = os.path.join(REPO, "sccg-genome-compression_amd", "bin", "fetch")
FUNCTIONS = ["sccg_reader_find_approx", "sccg_reader_find_approx_device", "sccg_cohort_find_approx", "sccg_cohort_find_approx_device"]


def cases():
    rng = random.Random(7)
    for k in range(60):
        alphabet = [b"ACGT", b"ACGTN", b"ACGTacgtNn)"][k % 3]
        seq = findlib.random_sequence(rng.randint(0, 300), 500 + k, alphabet)
        m = [1, 2, 3, 8, 17, 33][k % 6]
        pattern = findlib.random_pattern(rng, m, ["ACGT", "ACGTRYSWKMBDHVN", "NWSRY"][(k // 6) % 3])
        if k % 5 == 0 and len(seq) >= m:   # cut from the sequence itself, so that there are near hits
            at = rng.randrange(len(seq) - m + 1)
            cut = seq[at:at + m].decode().upper()
            pattern = cut if all(c in "ACGT" for c in cut) else pattern
        regions = [(0, len(seq))] + [tuple(sorted((rng.randint(0, len(seq)), rng.randint(0, len(seq))))) for _ in range(12)]
        yield k, seq, pattern, regions, rng


def test_oracles_agree():
    seen_k, seen_m = set(), set()
    for k, seq, pattern, regions, rng in cases():
        m = len(pattern)
        kmax = min(m - 1, 15)
        for K in sorted({0, kmax, rng.randint(0, kmax)}):
            seen_k.add(K)
            for strands in ("+", "-", "both"):
                a = fa.want(seq, pattern, regions, K, strands)
                b = fa.want(seq, pattern, regions, K, strands, distances=fa.distances_naive)
                fa.check(a, b, regions, f"case {k} {pattern} K={K} {strands}")
        seen_m.add(m)
    assert seen_m == {1, 2, 3, 8, 17, 33} and {0, 1, 2, 7, 15} <= seen_k


def test_k0_is_findlib_with_a_zero_column():
    for k, seq, pattern, regions, _ in cases():
        for strands in ("+", "-", "both"):
            off, rows = fa.want(seq, pattern, regions, 0, strands)
            woff, whit = findlib.want(seq, pattern, regions, strands)
            assert np.array_equal(off, woff) and np.array_equal(rows[:, :2], whit) and not rows[:, 2].any(), (k, pattern, strands)


def test_oracle_on_a_worked_example():
    #       01234567890123456789012
    seq = b"GAATTCnGAATTCacgtGAATTA"
    L = len(seq)
    # the forward distances of GAATTC, counted by hand letter by letter; the windows over the n (starts 1..6) have d >= 1
    assert fa.distances(seq, "GAATTC", 0, L).tolist() == [0, 4, 6, 6, 6, 6, 4, 0, 4, 5, 6, 5, 4, 5, 6, 5, 4, 1]
    assert fa.distances(seq, "GAATTC", 0, 5).tolist() == [] and fa.distances(seq, "GAATTC", 1, 7).tolist() == [4]
    # a palindrome: the reverse strand's masks are the forward's, so both strands carry the same d
    off, rows = fa.want(seq, "GAATTC", [(0, L), (0, 5), (7, 13), (7, 12), (17, L), (17, L - 1)], 1)
    assert off.tolist() == [0, 6, 6, 8, 8, 10, 10]
    assert rows[:6].tolist() == [[0, 0, 0], [0, 1, 0], [7, 0, 0], [7, 1, 0], [17, 0, 1], [17, 1, 1]]
    assert rows[6:].tolist() == [[7, 0, 0], [7, 1, 0], [17, 0, 1], [17, 1, 1]]
    assert fa.want(seq, "GAATTC", [(0, L)], 0)[1].tolist() == [[0, 0, 0], [0, 1, 0], [7, 0, 0], [7, 1, 0]]
    # the window AATTCn at 1 under AATTCN: the sequence's n is a mismatch even against the pattern's N
    assert fa.distances(seq, "AATTCN", 0, 8).tolist() == [3, 1, 3]
    assert fa.want(seq, "AATTCN", [(0, 8)], 1, "+")[1].tolist() == [[1, 0, 1]]
    assert fa.want(seq, "AATTCN", [(0, 8)], 0, "+")[1].tolist() == []
    assert fa.want(seq, "AATTCN", [(0, 6)], 1, "+")[1].tolist() == []   # it would cross the region's end
    # the palindrome with its last letter altered, GAATTA, at its own site 17: forward 0; the reverse strand's
    # pattern is TAATTC, which misses the site's first and last letter
    assert fa.want(seq, "GAATTA", [(17, L)], 2)[1].tolist() == [[17, 0, 0], [17, 1, 2]]
    assert fa.want(seq, "gaatta", [(17, L)], 1)[1].tolist() == [[17, 0, 0]]
    assert fa.want(seq, "GAATTA", [(0, L)], 1, "+")[1].tolist() == [[0, 0, 1], [7, 0, 1], [17, 0, 0]]
    assert fa.want(seq, "TAATTC", [(0, L)], 1, "-")[1].tolist() == [[0, 1, 1], [7, 1, 1], [17, 1, 0]]   # the same, relabelled


def test_library_exports_the_find_approx_functions():
    lib = sccg.load_library()
    declared = sccg.header_functions()
    for name in FUNCTIONS:
        assert name in declared and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert sccg.FIND_MAX_MISMATCHES == 15


def test_null_handles_are_invalid():
    lib = sccg.load_library()
    I = E["SCCG_E_INVALID"]
    regions = (sccg.Region * 1)((0, 4))
    items = (sccg.CohortRegion * 1)((0, 4, 0, 0))
    off = (ctypes.c_int64 * 2)(5, 5)
    buf = sccg.Buf()
    n = ctypes.c_size_t(7)
    assert lib.sccg_reader_find_approx(None, b"ACGT", 4, regions, 1, 3, 1, off, ctypes.byref(buf)) == I
    assert lib.sccg_cohort_find_approx(None, b"ACGT", 4, items, 1, 3, 1, off, ctypes.byref(buf)) == I
    assert lib.sccg_reader_find_approx_device(None, b"ACGT", 4, regions, 1, 3, 1, None, None, 0, ctypes.byref(n), None) == I
    assert lib.sccg_cohort_find_approx_device(None, b"ACGT", 4, items, 1, 3, 1, None, None, 0, ctypes.byref(n), None) == I
    assert not buf.data and buf.len == 0 and n.value == 7 and list(off) == [5, 5]


def usage_error(*args):
    # (the files do not exist: everything here is refused before anything is opened and before the GPU is touched)
    p = subprocess.run([FETCH] + list(args), capture_output=True)
    assert p.returncode == 1 and p.stdout == b"" and b"Usage:" in p.stderr and b"--find-approx" in p.stderr, (args, p.stderr)
    return p.stderr


def test_cli_usage_errors(tmp_path):
    rec, ref = str(tmp_path / "rec"), str(tmp_path / "ref")
    for bad in ("x", "", "-1", "1x", "+1", "1.0", "16", "99999999999999999999"):   # no decimal number, or beyond 15
        assert b"malformed mismatches" in usage_error("--find-approx", bad, "GATTACAGATTACAGATTACA", rec, ref, "1-10"), bad
    for k, pat in (("7", "GATTACA"), ("8", "GATTACA"), ("1", "G"), ("15", "ACGTACGTACGTACG")):   # K >= m
        assert b"malformed mismatches" in usage_error("--find-approx", k, pat, rec, ref, "1-10"), (k, pat)
    for bad in ("GATXACA", "", "A" * 65, "GAT-ACA"):
        assert b"malformed pattern" in usage_error("--find-approx", "1", bad, rec, ref, "1-10"), bad
    for bad in ("0", "-4", "x", "5-3", "1x", "", "3-", "0-2"):
        assert ("malformed region '" + bad + "'").encode() in usage_error("--find-approx", "1", "GATTACA", rec, ref, "12-14", bad), bad
    for args in ([], ["1"], ["1", "GATTACA"], ["1", "GATTACA", rec], ["1", "GATTACA", rec, ref]):   # too few arguments
        usage_error("--find-approx", *args)
    for mode in ("-i", "--reverse-complement", "--origin", "--locate", "--lift", "--find", "--find-approx"):   # first argument only
        usage_error("--find-approx", mode, "1", "GATTACA", rec, ref, "1-10")
        usage_error("--find-approx", "1", mode, "GATTACA", rec, ref, "1-10")
    # a good call goes on to the files
    p = subprocess.run([FETCH, "--find-approx", "6", "GATTACA", rec, ref, "1-10", "7"], capture_output=True)
    assert p.returncode == 1 and b"Usage:" not in p.stderr and p.stdout == b""


def test_cli_find_keeps_its_message():
    p = subprocess.run([FETCH, "--find", "GATXACA", "rec", "ref", "1-10"], capture_output=True)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.startswith(b"Error: malformed pattern 'GATXACA' (1 to 64 IUPAC nucleotide letters, ACGTURYSWKMBDHVN in either case)\n"
                               b"Usage: " + FETCH.encode() + b" --find <PATTERN> <record_file> <reference_file> <region>...\n"), p.stderr
    assert b"--find-approx" not in p.stderr
