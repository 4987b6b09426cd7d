"""Lift without a GPU: the run-length oracle itself (liftlib) on the worked example written out by hand, the
struct layout, the exported names, the argument handling that needs no device, and the command line's
usage texts."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cohortlib
import liftlib
import locatelib
from cohortlib import HAND, RFA_N
from pkg import sccg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FETCH = os.path.join(REPO, "sccg-genome-compression_amd", "bin", "fetch")
NEW = ["sccg_reader_lift", "sccg_reader_lift_device", "sccg_cohort_lift", "sccg_cohort_lift_device"]

# cohortlib.ERASED_REC over RFA_N ("ACGTNNNNACGT" x 10, |R| = 120): (0,30) copies R' 0..29 to sequence 0..3 and
# 8..33 (a target N run at 4..7), (40,10) copies R' 40..49 to 38..47; every erased run of four is a -2 block
WORKED_WHOLE = [(0, 4, 0), (4, 4, -2), (8, 8, 8), (16, 4, -2), (20, 8, 16), (28, 4, -2), (32, 8, 24), (40, 4, -2), (44, 2, 32),
                (46, 6, -1), (52, 4, -2), (56, 4, -1), (60, 4, 38), (64, 4, -2), (68, 6, 42), (74, 2, -1), (76, 4, -2), (80, 8, -1),
                (88, 4, -2), (92, 8, -1), (100, 4, -2), (104, 8, -1), (112, 4, -2), (116, 4, -1)]
# [2, 70): both ends clipped, the thirteen rows between them unchanged
WORKED_2_70 = [(2, 2, 2), (4, 4, -2), (8, 8, 8), (16, 4, -2), (20, 8, 16), (28, 4, -2), (32, 8, 24), (40, 4, -2), (44, 2, 32),
               (46, 6, -1), (52, 4, -2), (56, 4, -1), (60, 4, 38), (64, 4, -2), (68, 2, 42)]


def test_oracle_on_the_worked_example():
    pos, _ = locatelib.inverse(RFA_N, cohortlib.ERASED_REC)
    assert len(pos) == 120
    assert [tuple(r) for r in liftlib.blocks(pos, 0, 120).tolist()] == WORKED_WHOLE
    assert [tuple(r) for r in liftlib.blocks(pos, 2, 70).tolist()] == WORKED_2_70 and len(WORKED_2_70) == 15
    assert liftlib.blocks(pos, 7, 7).shape == (0, 3)
    off, blk = liftlib.want(pos, [(0, 120), (5, 5), (2, 70)])
    assert off.tolist() == [0, 24, 24, 39]
    liftlib.check_shape(off, blk, [(0, 120), (5, 5), (2, 70)])
    assert np.array_equal(liftlib.expand(blk[:24]), pos)
    assert liftlib.cli_lines(pos, [(1, 8), (47, 47)]) == [">1-8", "1\t4\t1\t4", "5\t8\tN", ">47-47", "47\t47\t-"]


@pytest.mark.parametrize("name", sorted(HAND))
def test_oracle_tiles_and_expands_on_hand_records(name):
    rfa, rec = HAND[name]
    pos, _ = locatelib.inverse(rfa, rec)
    intervals = liftlib.every_pair(min(len(pos), 40))
    off, blk = liftlib.want(pos, intervals)
    liftlib.check_shape(off, blk, intervals, name)
    for i, (b, e) in enumerate(intervals):
        assert np.array_equal(liftlib.expand(blk[off[i]:off[i + 1]]), pos[b:e]), (name, b, e)


def test_header_declares_and_library_exports_lift():
    lib = sccg.load_library()
    names = sccg.header_functions()
    for name in NEW:
        assert name in names, name
        assert hasattr(lib, name), name
    text = open(sccg.HEADER).read()
    assert "typedef struct { int64_t ref, len, pos; } sccg_lift_block;" in text
    for cls in (sccg.Reader, sccg.Cohort):
        assert hasattr(cls, "lift") and hasattr(cls, "lift_tensor"), cls


def test_null_arguments():
    lib = sccg.load_library()
    E = sccg.ERR_CODES["SCCG_E_INVALID"]
    intervals = (sccg.Region * 1)((0, 1))
    items = (sccg.CohortRegion * 1)((0, 1, 0, 0))
    off = (ctypes.c_int64 * 2)(77, 77)
    buf = sccg.Buf()
    n_blk = ctypes.c_size_t(77)
    for n in (0, 1):
        assert lib.sccg_reader_lift(None, intervals, n, off, ctypes.byref(buf)) == E
        assert lib.sccg_cohort_lift(None, items, n, off, ctypes.byref(buf)) == E
        assert lib.sccg_reader_lift_device(None, intervals, n, None, None, 0, ctypes.byref(n_blk), None) == E
        assert lib.sccg_cohort_lift_device(None, items, n, None, None, 0, ctypes.byref(n_blk), None) == E
    assert list(off) == [77, 77] and n_blk.value == 77 and not buf.data and buf.len == 0


LIFT_USAGE = (b" --lift <record_file> <reference_file> <refregion>...\n"
              b"  refregion: begin-end (1-based, inclusive) or pos, of the reference sequence; prints >begin-end, then\n"
              b"  one line per block: rbegin rend tbegin tend (where the bases lie in the sequence) | rbegin rend -\n"
              b"  (no copy) | rbegin rend N (an erased reference N run)\n"
              b"  --lift is the first argument only, not with -i, --origin or --locate\n")
ORIGIN_USAGE = (b" [-i | --origin] <record_file> <reference_file> <region>...\n"
                b"  region: begin-end (1-based, inclusive) or pos\n"
                b"  -i, --reverse-complement (first argument only): every region reverse-complemented\n"
                b"  --origin (first argument only, not with -i): where each base comes from, one line per run:\n"
                b"      tbegin tend rbegin rend (copied from the reference) | tbegin tend * (literal) | tbegin tend N\n")
LOCATE_USAGE = (b" --locate <record_file> <reference_file> <refpos>...\n"
                b"  refpos: a 1-based position of the reference sequence; prints refpos, the first 1-based sequence\n"
                b"  position holding a copy of it (- none, N an erased reference N) and the number of copies\n"
                b"  --locate is the first argument only, not with -i or --origin\n")


def usage_of(args):
    p = subprocess.run([FETCH] + args, capture_output=True)
    assert p.returncode == 1 and p.stdout == b"", args
    assert p.stderr.startswith(b"Usage: " + FETCH.encode()), (args, p.stderr)
    return p.stderr[len(b"Usage: " + FETCH.encode()):]


def test_cli_lift_usage():
    for args in (["--lift"], ["--lift", "rec"], ["--lift", "rec", "ref"], ["--lift", "-i", "rec", "ref", "5"],
                 ["--lift", "--origin", "rec", "ref", "5"], ["--lift", "--locate", "rec", "ref", "5"]):
        assert usage_of(args) == LIFT_USAGE, args


def test_cli_other_usages_are_unchanged():
    for args in (["--origin"], ["--origin", "rec", "ref"], ["--origin", "-i", "rec", "ref", "5"], ["-i", "rec", "ref"], [],
                 ["--origin", "--lift", "rec", "ref", "5"], ["-i", "--lift", "rec", "ref", "5"]):
        assert usage_of(args) == ORIGIN_USAGE, args
    for args in (["--locate"], ["--locate", "rec", "ref"], ["--locate", "--origin", "rec", "ref", "5"],
                 ["--locate", "--lift", "rec", "ref", "5"]):
        assert usage_of(args) == LOCATE_USAGE, args


@pytest.mark.parametrize("region", ["0", "-4", "x", "5-3", "1x", "", "3-", "0-2"])
def test_cli_malformed_region_names_it(region, tmp_path):
    # (the files do not exist: a malformed region is reported before anything is opened)
    p = subprocess.run([FETCH, "--lift", str(tmp_path / "rec"), str(tmp_path / "ref"), "12-14", region], capture_output=True)
    assert p.returncode == 1 and p.stdout == b""
    assert b"Usage:" not in p.stderr
    assert ("'" + region + "'").encode() in p.stderr, p.stderr
