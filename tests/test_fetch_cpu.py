"""CPU-side checks of the region reader (sccg_reader_*, bin/fetch): the header declares and the
library exports the new entry points, their NULL-argument forms fail without a GPU, the `fetch`
command line validates its regions before it touches the GPU, and the profiler's new family sits at
the end of the name table (existing family indices and masks keep their meaning)."""
import ctypes
import os
import subprocess

import pytest

from pkg import sccg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FETCH = os.path.join(REPO, "sccg-genome-compression_amd", "bin", "fetch")
NEW = ["sccg_reader_open", "sccg_reader_open_device", "sccg_reader_close", "sccg_reader_length",
       "sccg_reader_header", "sccg_reader_fetch", "sccg_reader_fetch_device"]
# prof.cpp's name table before the region reader
FAMILIES_BEFORE = ["fasta_strip", "run_extract", "run_text", "local_segments", "local_pass_k10", "local_emit", "n_filter",
                   "first_sweep_anchors", "walk", "presence_scan", "fullc_scan", "match_emit", "walk_chain",
                   "dc_decode", "dc_format", "walk_carry"]


def test_header_declares_and_library_exports_the_reader():
    lib = sccg.load_library()
    names = sccg.header_functions()
    for name in NEW:
        assert name in names, name
        assert hasattr(lib, name), name


def test_null_arguments_rejected():
    lib = sccg.load_library()
    out = ctypes.c_void_p(1)
    assert lib.sccg_reader_open(None, b"", 0, b"", 0, ctypes.byref(out)) != 0
    assert not out.value, "a failed open leaves *out NULL"
    assert lib.sccg_reader_open(None, None, 0, None, 0, None) != 0
    assert lib.sccg_reader_open_device(None, None, 0, None, 0, None, None) != 0
    reg = (sccg.Region * 1)((0, 1))
    buf = sccg.Buf()
    n = ctypes.c_size_t()
    assert lib.sccg_reader_fetch(None, reg, 1, 0, ctypes.byref(buf)) != 0
    assert not buf.data
    assert lib.sccg_reader_fetch_device(None, reg, 1, 0, None, 0, ctypes.byref(n), None) != 0


def test_close_and_length_of_null():
    lib = sccg.load_library()
    lib.sccg_reader_close(None)   # a no-op
    assert lib.sccg_reader_length(None) == -1
    n = ctypes.c_size_t(7)
    lib.sccg_reader_header(None, ctypes.byref(n))
    assert n.value == 0


def test_cli_usage():
    for args in ([], ["rec"], ["rec", "ref"]):
        p = subprocess.run([FETCH] + args, capture_output=True)
        assert p.returncode == 1
        assert b"Usage:" in p.stderr


@pytest.mark.parametrize("region", ["0-5", "5-3", "x", "3-", "-4", "2-3-4", "1-2x", ""])
def test_cli_malformed_region_names_it(region, tmp_path):
    # (the files do not exist: a malformed region is reported before anything is opened)
    p = subprocess.run([FETCH, str(tmp_path / "rec"), str(tmp_path / "ref"), "1-2", region], capture_output=True)
    assert p.returncode == 1
    assert b"Usage:" not in p.stderr
    assert ("'" + region + "'").encode() in p.stderr, p.stderr


def test_cli_valid_region_reaches_the_gpu(tmp_path):
    import torch
    (tmp_path / "rec").write_bytes(b">t\n\n\nACGT\n")
    (tmp_path / "ref").write_bytes(b">r\nACGT\n")
    p = subprocess.run([FETCH, str(tmp_path / "rec"), str(tmp_path / "ref"), "1-2", "3"], capture_output=True)
    if torch.cuda.is_available():   # (run on a GPU machine: the same command succeeds)
        assert p.returncode == 0, p.stderr
        assert p.stdout == b">t:1-2\nAC\n>t:3-3\nG\n"
        return
    assert p.returncode == 1
    assert b"no usable GPU" in p.stderr, p.stderr
    assert p.stdout == b""


def test_fetch_is_the_last_profiler_family():
    lib = sccg.load_library()
    names, i = [], 0
    while True:
        name = lib.sccg_profile_name(i)
        if not name:
            break
        names.append(name.decode())
        i += 1
    assert names == FAMILIES_BEFORE + ["fetch"]
    assert len(names) <= 32, "sccg_profile_mask is a 32-bit mask"
