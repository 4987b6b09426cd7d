"""CPU-side checks of the shared reference and the cohort fetch (sccg_reference_*,
sccg_reader_open_shared*, sccg_reader_device_bytes, sccg_cohort_*): the header declares and the
library exports every new entry point, and NULL arguments fail before any device is touched."""
import ctypes

from pkg import sccg

NEW = ["sccg_reference_open", "sccg_reference_open_device", "sccg_reference_close", "sccg_reference_device_bytes",
       "sccg_reader_open_shared", "sccg_reader_open_shared_device", "sccg_reader_device_bytes", "sccg_cohort_create",
       "sccg_cohort_close", "sccg_cohort_samples", "sccg_cohort_fetch", "sccg_cohort_fetch_device"]


def test_header_declares_and_library_exports_the_new_entry_points():
    lib = sccg.load_library()
    names = sccg.header_functions()
    for name in NEW:
        assert name in names, name
        assert hasattr(lib, name), name
    text = open(sccg.HEADER).read()
    for word in ("SCCG_REF_ERASED", "SCCG_REF_KEPT", "sccg_cohort_region", "typedef struct sccg_reference sccg_reference",
                 "typedef struct sccg_cohort sccg_cohort"):
        assert word in text, word


def test_cohort_region_layout():
    # { int64 begin, end; int32 sample; uint32 flags; }
    assert ctypes.sizeof(sccg.CohortRegion) == 24
    assert [sccg.CohortRegion.begin.offset, sccg.CohortRegion.end.offset, sccg.CohortRegion.sample.offset,
            sccg.CohortRegion.flags.offset] == [0, 8, 16, 20]
    assert sccg.REF_FORMS == {"erased": 1, "kept": 2}


def test_null_arguments_rejected_and_nothing_written():
    lib = sccg.load_library()
    fa = b">r\nACGT\n"
    out = ctypes.c_void_p(0x5A5A)
    assert lib.sccg_reference_open(None, fa, len(fa), 0, ctypes.byref(out)) != 0
    assert not out.value   # (*out is NULL on every error)
    assert lib.sccg_reference_open(None, fa, len(fa), 0, None) != 0
    out = ctypes.c_void_p(0x5A5A)
    assert lib.sccg_reference_open_device(None, None, 0, 0, ctypes.byref(out), None) != 0
    assert not out.value
    out = ctypes.c_void_p(0x5A5A)
    assert lib.sccg_reader_open_shared(None, b"\n\nAC", 4, ctypes.byref(out)) != 0
    assert not out.value
    out = ctypes.c_void_p(0x5A5A)
    assert lib.sccg_reader_open_shared_device(None, None, 0, ctypes.byref(out), None) != 0
    assert not out.value
    out = ctypes.c_void_p(0x5A5A)
    assert lib.sccg_cohort_create(None, 0, ctypes.byref(out)) != 0
    assert not out.value
    one = (ctypes.c_void_p * 1)(None)
    out = ctypes.c_void_p(0x5A5A)
    assert lib.sccg_cohort_create(one, 1, ctypes.byref(out)) != 0   # a NULL entry
    assert not out.value
    assert lib.sccg_cohort_create(one, 1, None) != 0
    reg = (sccg.CohortRegion * 1)((0, 1, 0, 0))
    fmt = sccg.FetchFormat(1, 0, 0, 0)
    buf = sccg.Buf()
    n = ctypes.c_size_t(77)
    assert lib.sccg_cohort_fetch(None, reg, 1, ctypes.byref(fmt), ctypes.byref(buf)) != 0
    assert not buf.data and buf.len == 0
    assert lib.sccg_cohort_fetch(None, reg, 1, None, ctypes.byref(buf)) != 0
    assert lib.sccg_cohort_fetch(None, reg, 1, ctypes.byref(fmt), None) != 0
    assert lib.sccg_cohort_fetch_device(None, reg, 1, ctypes.byref(fmt), None, 0, ctypes.byref(n), None) != 0
    assert n.value == 77
    assert lib.sccg_cohort_fetch_device(None, reg, 1, None, None, 0, None, None) != 0
    assert lib.sccg_reader_device_bytes(None) == 0
    assert lib.sccg_reference_device_bytes(None) == 0
    assert lib.sccg_cohort_samples(None) == 0


def test_close_functions_accept_null():
    lib = sccg.load_library()
    lib.sccg_reference_close(None)
    lib.sccg_cohort_close(None)
    lib.sccg_reader_close(None)
