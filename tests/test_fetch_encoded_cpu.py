"""CPU-side checks of the encoded fetch (sccg_reader_fetch_encoded*, `fetch -i`): the header
declares and the library exports the entry points, the format check needs no GPU, NULL arguments
fail, and the command line recognises `-i` as its first argument only and still validates every
region before it opens anything."""
import ctypes
import os
import subprocess

import pytest

from pkg import sccg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FETCH = os.path.join(REPO, "sccg-genome-compression_amd", "bin", "fetch")
NEW = ["sccg_fetch_bytes_per_base", "sccg_reader_fetch_encoded", "sccg_reader_fetch_encoded_device"]
ASCII, INDEX, ONEHOT = 0, 1, 2
U8, F16, BF16, F32 = 0, 1, 2, 3


def bpb(encoding, dtype, flags=0, reserved=0):
    fmt = sccg.FetchFormat(encoding, dtype, flags, reserved)
    return sccg.load_library().sccg_fetch_bytes_per_base(ctypes.byref(fmt))


def test_header_declares_and_library_exports_the_encoded_fetch():
    lib = sccg.load_library()
    names = sccg.header_functions()
    for name in NEW:
        assert name in names, name
        assert hasattr(lib, name), name


def test_bytes_per_base_of_the_valid_formats():
    got = [bpb(ASCII, U8), bpb(INDEX, U8), bpb(ONEHOT, U8), bpb(ONEHOT, F16), bpb(ONEHOT, BF16), bpb(ONEHOT, F32)]
    assert got == [1, 1, 4, 8, 8, 16]
    for flags in (1, 2, 3):   # SCCG_FETCH_UPPER, SCCG_FETCH_REVCOMP
        assert bpb(INDEX, U8, flags) == 1 and bpb(ASCII, U8, flags) == 1 and bpb(ONEHOT, F32, flags) == 16


@pytest.mark.parametrize("fmt", [(3, U8, 0, 0), (ONEHOT, 4, 0, 0), (INDEX, F16, 0, 0), (INDEX, U8, 0, 1), (INDEX, U8, 4, 0),
                                 (ASCII, F32, 0, 0)],
                         ids=["encoding", "dtype", "f16_index", "reserved", "flag_bit_4", "f32_ascii"])
def test_bytes_per_base_of_invalid_formats_is_zero(fmt):
    assert bpb(*fmt) == 0
    assert sccg.load_library().sccg_fetch_bytes_per_base(None) == 0


def test_null_arguments_rejected():
    lib = sccg.load_library()
    reg = (sccg.Region * 1)((0, 1))
    fmt = sccg.FetchFormat(INDEX, U8, 0, 0)
    buf = sccg.Buf()
    n = ctypes.c_size_t()
    assert lib.sccg_reader_fetch_encoded(None, reg, 1, None, ctypes.byref(fmt), ctypes.byref(buf)) != 0
    assert not buf.data
    assert lib.sccg_reader_fetch_encoded(None, reg, 1, None, None, ctypes.byref(buf)) != 0
    assert not buf.data
    assert lib.sccg_reader_fetch_encoded(None, reg, 1, None, ctypes.byref(fmt), None) != 0
    assert lib.sccg_reader_fetch_encoded_device(None, reg, 1, None, ctypes.byref(fmt), None, 0, ctypes.byref(n), None) != 0
    assert lib.sccg_reader_fetch_encoded_device(None, reg, 1, None, None, None, 0, None, None) != 0


def test_cli_flag_alone_prints_usage():
    for args in (["-i"], ["--reverse-complement"], ["-i", "rec"], ["-i", "rec", "ref"]):
        p = subprocess.run([FETCH] + args, capture_output=True)
        assert p.returncode == 1
        assert b"Usage:" in p.stderr


@pytest.mark.parametrize("flag", ["-i", "--reverse-complement"])
@pytest.mark.parametrize("regions,bad", [(["1-2", "-4"], "-4"), (["2-3-4"], "2-3-4")])
def test_cli_with_flag_names_the_malformed_region(flag, regions, bad, tmp_path):
    # (the files do not exist: a malformed region is reported before anything is opened)
    p = subprocess.run([FETCH, flag, str(tmp_path / "rec"), str(tmp_path / "ref")] + regions, capture_output=True)
    assert p.returncode == 1 and p.stdout == b""
    assert b"Usage:" not in p.stderr
    assert ("malformed region '" + bad + "'").encode() in p.stderr, p.stderr


def test_cli_flag_after_the_files_is_a_region(tmp_path):
    p = subprocess.run([FETCH, str(tmp_path / "rec"), str(tmp_path / "ref"), "-i"], capture_output=True)
    assert p.returncode == 1 and p.stdout == b""
    assert b"malformed region '-i'" in p.stderr, p.stderr
    p = subprocess.run([FETCH, "-i", str(tmp_path / "rec"), str(tmp_path / "ref"), "1-2", "-i"], capture_output=True)
    assert p.returncode == 1 and b"malformed region '-i'" in p.stderr, p.stderr
