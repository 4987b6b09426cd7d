"""Find without a GPU: the two oracles of findlib agree, the pattern masks the kernels are launched with
(sccg_find_pattern_masks, a pure host function) are the table written out here, and the ABI's new entry
points exist and refuse NULL handles."""
import ctypes
import random

import pytest

import findlib
from pkg import sccg

E = sccg.ERR_CODES
# bit 0 A, 1 C, 2 G, 3 T -- written out, not derived from findlib.IUPAC
MASK = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11, "V": 7,
        "N": 15}
RC = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K", "B": "V", "V": "B",
      "D": "H", "H": "D", "N": "N"}
FUNCTIONS = ["sccg_find_pattern_masks", "sccg_reader_find", "sccg_reader_find_device", "sccg_cohort_find", "sccg_cohort_find_device"]


def test_oracles_agree():
    rng = random.Random(1)
    for k in range(60):
        alphabet = [b"ACGT", b"ACGTN", b"ACGTacgtNn)"][k % 3]
        seq = findlib.random_sequence(rng.randint(0, 300), 100 + k, alphabet)
        m = rng.choice([1, 1, 2, 3, 4, 8, 17])
        letters = ["ACGT", "ACGTRYSWKMBDHVN", "NWSRY"][k % 3]
        pattern = findlib.random_pattern(rng, m, letters)
        if k % 5 == 0 and len(seq) >= m:   # cut from the sequence itself, so that there are hits
            at = rng.randrange(len(seq) - m + 1)
            cut = seq[at:at + m].decode().upper()
            pattern = cut if all(c in "ACGT" for c in cut) else pattern
        regions = [(0, len(seq))] + [tuple(sorted((rng.randint(0, len(seq)), rng.randint(0, len(seq))))) for _ in range(12)]
        for strands in ("+", "-", "both"):
            a = findlib.want(seq, pattern, regions, strands)
            b = findlib.want(seq, pattern, regions, strands, starts=findlib.starts_naive)
            findlib.check(a, b, regions, f"case {k} {pattern} {strands}")


def test_oracle_on_a_worked_example():
    seq = b"GAATTCnGAATTCacgtGGTACCAAA"
    off, hits = findlib.want(seq, "GAATTC", [(0, len(seq)), (0, 5), (1, 13), (7, 13), (7, 12)])
    assert off.tolist() == [0, 4, 4, 6, 8, 8]
    assert hits[:4].tolist() == [[0, 0], [0, 1], [7, 0], [7, 1]]   # a palindrome: both strands at the same pos, forward first
    assert findlib.want(seq, "N", [(5, 8)])[1].tolist() == [[5, 0], [5, 1], [7, 0], [7, 1]]   # the sequence's n matches nothing
    assert findlib.want(seq, "ggtac", [(0, len(seq))], "+")[1].tolist() == [[17, 0]]
    assert findlib.want(seq, "GTACC", [(0, len(seq))], "-")[1].tolist() == [[17, 1]]   # GGTAC reversed and complemented
    assert findlib.want(seq, "TTT", [(0, len(seq))])[1].tolist() == [[23, 1]]


def test_library_exports_the_find_functions():
    lib = sccg.load_library()
    declared = sccg.header_functions()
    for name in FUNCTIONS:
        assert name in declared and hasattr(lib, name), name
    assert sccg.FIND_MAX_PATTERN == 64 and sccg.FIND_STRANDS == {"+": 1, "-": 2, "both": 3}


def test_masks_of_every_letter():
    for letter, mask in MASK.items():
        for pat in (letter, letter.lower()):
            fwd, rev = sccg.find_pattern_masks(pat)
            assert fwd == bytes([mask]), pat
            assert rev == bytes([MASK[RC[letter]]]), pat
        assert findlib.masks(letter) == bytes([mask]) and findlib.revcomp_pattern(letter) == RC[letter]
    assert sccg.find_pattern_masks(b"acgu") == (bytes([1, 2, 4, 8]), bytes([1, 2, 4, 8]))   # bytes too; U is T: ACGT is its own
    assert sccg.find_pattern_masks(b"aacu") == (bytes([1, 1, 2, 8]), bytes([1, 4, 8, 8]))   # AGTT


def test_reverse_complement_masks():
    fwd, rev = sccg.find_pattern_masks("ACGGT")
    assert fwd == bytes([1, 2, 4, 4, 8]) and rev == bytes([1, 2, 2, 4, 8])   # ACCGT
    fwd, rev = sccg.find_pattern_masks("RYBVNSWKMDH")
    assert fwd == bytes(MASK[c] for c in "RYBVNSWKMDH")
    assert rev == bytes(MASK[c] for c in "DHKMWSNBVRY")
    assert sccg.find_pattern_masks("GAATTC")[0] == sccg.find_pattern_masks("GAATTC")[1]   # a palindrome is its own
    long = "ACGTN" * 12 + "RYKM"
    assert len(long) == 64
    fwd, rev = sccg.find_pattern_masks(long)
    assert fwd == bytes(MASK[c] for c in long) and rev == bytes(MASK[RC[c]] for c in reversed(long))


def test_fwd_or_rev_may_be_null():
    lib = sccg.load_library()
    out = (ctypes.c_uint8 * 3)()
    assert lib.sccg_find_pattern_masks(b"ACR", 3, out, None) == 0 and bytes(out) == bytes([1, 2, 5])
    assert lib.sccg_find_pattern_masks(b"ACR", 3, None, out) == 0 and bytes(out) == bytes([10, 4, 8])
    assert lib.sccg_find_pattern_masks(b"ACR", 3, None, None) == 0


def test_bytes_outside_the_alphabet_and_bad_lengths():
    lib = sccg.load_library()
    good = set("ACGTURYSWKMBDHVN".encode()) | set("acgturyswkmbdhvn".encode())
    f, r = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 64)()
    for b in range(256):
        rc = lib.sccg_find_pattern_masks(bytes([b]), 1, f, r)
        assert rc == (0 if b in good else E["SCCG_E_INVALID"]), b
        rc = lib.sccg_find_pattern_masks(b"AC" + bytes([b]) + b"G", 4, f, r)
        assert rc == (0 if b in good else E["SCCG_E_INVALID"]), b
    assert lib.sccg_find_pattern_masks(b"", 0, f, r) == E["SCCG_E_INVALID"]
    assert lib.sccg_find_pattern_masks(b"A" * 64, 64, f, r) == 0
    assert lib.sccg_find_pattern_masks(b"A" * 65, 65, f, r) == E["SCCG_E_INVALID"]
    assert lib.sccg_find_pattern_masks(None, 4, f, r) == E["SCCG_E_INVALID"]
    for bad in ("", "A" * 65, "ACGX", "AC GT", "AC-GT"):
        with pytest.raises(ValueError):
            sccg.find_pattern_masks(bad)


def test_null_handles_are_invalid():
    lib = sccg.load_library()
    I = E["SCCG_E_INVALID"]
    regions = (sccg.Region * 1)((0, 4))
    items = (sccg.CohortRegion * 1)((0, 4, 0, 0))
    off = (ctypes.c_int64 * 2)()
    buf = sccg.Buf()
    n = ctypes.c_size_t(7)
    assert lib.sccg_reader_find(None, b"ACGT", 4, regions, 1, 3, off, ctypes.byref(buf)) == I
    assert lib.sccg_cohort_find(None, b"ACGT", 4, items, 1, 3, off, ctypes.byref(buf)) == I
    assert lib.sccg_reader_find_device(None, b"ACGT", 4, regions, 1, 3, None, None, 0, ctypes.byref(n), None) == I
    assert lib.sccg_cohort_find_device(None, b"ACGT", 4, items, 1, 3, None, None, 0, ctypes.byref(n), None) == I
    assert not buf.data and buf.len == 0 and n.value == 7
