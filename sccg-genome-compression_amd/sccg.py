"""ctypes binding of libsccg.so (include/sccg.h) -- the MI355X SCCG hot path.

Mirrors the reference's two entry points (compression.cpp:320 compress_genome up to 7z,
decompression.cpp:117 reconstruct_genome + file body) and the match_sequences seam
(compression.cpp:36).  There is no CPU fallback: if the HIP library or a GPU is missing,
construction raises.
"""
from __future__ import annotations

import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
# SCCG_LIB_PATH: an alternative build of the same library (tuning runs compare variants)
LIB_PATH = os.environ.get("SCCG_LIB_PATH") or os.path.join(HERE, "lib", "libsccg.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "sccg.h")

SCCG_OK = 0
SCCG_E_DELTA_STOI = 4
OPT_EXACT_SWITCH = 1   # sccg_ctx_set_option (include/sccg.h)
FETCH_UPPER = 1        # sccg_reader_fetch flags
FETCH_REVCOMP = 2      # sccg_reader_fetch_encoded: every region on the reverse strand
REF_FORMS = {"erased": 1, "kept": 2}                       # SCCG_REF_*: which R' a record's N line asks for
REF_COORDS = 4                                             # SCCG_REF_COORDS: keep the R' -> R map (origin fetch)
ENCODINGS = {"ascii": 0, "index": 1, "onehot": 2, "origin": 3}     # SCCG_ENC_*
DTYPES = {"u8": 0, "f16": 1, "bf16": 2, "f32": 3, "i32": 4}        # SCCG_DT_* ("i32": with "origin" only)
LOCATE_NONE = -1       # SCCG_LOCATE_NONE: no token copies the reference position (deleted, or a literal)
LOCATE_REF_N = -2      # SCCG_LOCATE_REF_N: the position lies in an N run of the reference that R' has erased
ORIGIN_LITERAL, ORIGIN_N = -1, -2                          # "origin" values that are no reference position
FIND_MAX_PATTERN = 64                                      # SCCG_FIND_MAX_PATTERN
FIND_STRANDS = {"+": 1, "-": 2, "both": 3}                 # SCCG_FIND_FWD, SCCG_FIND_REV, both
FIND_MAX_MISMATCHES = 15                                   # SCCG_FIND_MAX_MISMATCHES
ERRORS = {1: "SCCG_E_INVALID", 2: "SCCG_E_HIP", 3: "SCCG_E_NOMEM", 4: "SCCG_E_DELTA_STOI",
          5: "SCCG_E_FORMAT", 6: "SCCG_E_RANGE", 7: "SCCG_E_PARSE", 8: "SCCG_E_UNSUPPORTED",
          9: "SCCG_E_INTERNAL", 10: "SCCG_E_OPEN_REF", 11: "SCCG_E_OPEN_TGT", 12: "SCCG_E_WRITE"}
ERR_CODES = {v: k for k, v in ERRORS.items()}


class SccgError(RuntimeError):
    def __init__(self, rc: int, msg: str = ""):
        super().__init__(f"{ERRORS.get(rc, rc)}: {msg}")
        self.rc = rc


class Buf(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_size_t)]


class Records(ctypes.Structure):
    _fields_ = [("kind", ctypes.POINTER(ctypes.c_uint8)), ("pos", ctypes.POINTER(ctypes.c_int32)),
                ("len", ctypes.POINTER(ctypes.c_int32)), ("t", ctypes.POINTER(ctypes.c_int64)),
                ("n", ctypes.c_int64)]


class Stats(ctypes.Structure):
    _fields_ = [("mode_global", ctypes.c_int), ("switch_segment", ctypes.c_int64),
                ("target_bases", ctypes.c_int64), ("reference_bases", ctypes.c_int64),
                ("n_matches", ctypes.c_int64), ("literal_bases", ctypes.c_int64),
                ("walk_rounds", ctypes.c_int64), ("walk_chunks", ctypes.c_int64),
                ("record_bytes", ctypes.c_int64), ("walk_chains", ctypes.c_int64),
                ("walk_reference_bases", ctypes.c_int64)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class Region(ctypes.Structure):
    """sccg_region: 0-based, half-open sequence positions."""
    _fields_ = [("begin", ctypes.c_int64), ("end", ctypes.c_int64)]


class CohortRegion(ctypes.Structure):
    """sccg_cohort_region: a region of one sample; flags bit 0 = reverse strand."""
    _fields_ = [("begin", ctypes.c_int64), ("end", ctypes.c_int64), ("sample", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class CohortLocus(ctypes.Structure):
    """sccg_cohort_locus: a position of the reference sequence, asked of one sample; flags 0."""
    _fields_ = [("ref_pos", ctypes.c_int64), ("sample", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class FetchFormat(ctypes.Structure):
    """sccg_fetch_format: encoding (ENCODINGS), ONEHOT's element type (DTYPES), FETCH_* flags, 0."""
    _fields_ = [("encoding", ctypes.c_uint32), ("dtype", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class Params(ctypes.Structure):
    """sccg_params (include/sccg.h): compression.cpp:373-379's constants; other values than the
    defaults are non-parity overrides (local=1 takes only m; local=0 takes 1 <= k <= 32, m)."""
    _fields_ = [("k", ctypes.c_int32), ("k2", ctypes.c_int32), ("L", ctypes.c_int32), ("m", ctypes.c_int32),
                ("T1", ctypes.c_float), ("T2", ctypes.c_int32), ("local", ctypes.c_int32)]


_lib = None


def hip_runtimes() -> list[str]:
    """The distinct libamdhip64 files mapped into this process (/proc/self/maps)."""
    try:
        with open("/proc/self/maps") as f:
            return sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln and "/" in ln})
    except OSError:
        return []


def load_library():
    """Load libsccg.so (raises if it was not built: no silent fallback).

    One HIP runtime per process: torch ships its own libamdhip64 (SONAME libamdhip64.so.7, the same
    as /opt/rocm's that libsccg links), and whichever is loaded first serves every later user of
    that SONAME -- but torch's libraries name the file (libamdhip64.so, RPATH $ORIGIN), so loading
    libsccg before torch maps BOTH runtimes, and torch then sees no GPU.  So torch (when installed)
    is imported first and its runtime serves libsccg too; a process that still ends up with two
    runtimes mapped is refused with a clear message instead of failing later in a HIP call.  The
    C CLIs (no torch) run on /opt/rocm's runtime."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built: run `make` or __graft_entry__.build()")
    try:
        import torch  # noqa: F401  (its HIP runtime first: see above)
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    rts = hip_runtimes()
    if len({os.path.realpath(r) for r in rts}) > 1:
        raise RuntimeError("two HIP runtimes are mapped into this process (" + ", ".join(rts) + "): libsccg was "
                           "loaded before torch; import torch (or sccg) before loading libsccg.so yourself")
    vp, sz, c, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int64
    lib.sccg_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    lib.sccg_ctx_destroy.argtypes = [vp]
    lib.sccg_last_error.argtypes = [vp]
    lib.sccg_last_error.restype = ctypes.c_char_p
    lib.sccg_last_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    lib.sccg_ctx_set_option.argtypes = [vp, ctypes.c_int, i64]
    lib.sccg_compress.argtypes = [vp, c, sz, c, sz, ctypes.POINTER(Buf)]
    lib.sccg_compress_device.argtypes = [vp, vp, sz, vp, sz, vp, sz, ctypes.POINTER(sz), vp]
    if hasattr(lib, "sccg_params_default"):   # (absent from builds older than the overrides: A/B runs)
        lib.sccg_params_default.argtypes = [ctypes.POINTER(Params)]
        lib.sccg_compress_ex.argtypes = [vp, ctypes.POINTER(Params), c, sz, c, sz, ctypes.POINTER(Buf)]
        lib.sccg_compress_device_ex.argtypes = [vp, ctypes.POINTER(Params), vp, sz, vp, sz, vp, sz, ctypes.POINTER(sz), vp]
    if hasattr(lib, "sccg_compress_files"):
        lib.sccg_compress_files.argtypes = [vp, ctypes.POINTER(Params), c, c, c, ctypes.POINTER(sz)]
    lib.sccg_compress_bound.argtypes = [sz, sz]
    lib.sccg_compress_bound.restype = sz
    lib.sccg_match.argtypes = [vp, c, sz, c, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, i64,
                               ctypes.POINTER(Records)]
    lib.sccg_records_free.argtypes = [ctypes.POINTER(Records)]
    if hasattr(lib, "sccg_walk_range"):
        lib.sccg_walk_range.argtypes = [vp, c, sz, c, sz, ctypes.c_int, ctypes.c_int, i64, i64, i64,
                                        ctypes.POINTER(Records), ctypes.POINTER(i64)]
        lib.sccg_walk_range_device.argtypes = [vp, vp, sz, vp, sz, ctypes.c_int, ctypes.c_int, i64, i64, i64,
                                               ctypes.POINTER(Records), ctypes.POINTER(i64), vp]
    lib.sccg_reconstruct.argtypes = [vp, c, sz, c, sz, ctypes.POINTER(Buf)]
    lib.sccg_reconstruct_device.argtypes = [vp, vp, sz, vp, sz, vp, sz, ctypes.POINTER(sz), vp]
    lib.sccg_buf_free.argtypes = [ctypes.POINTER(Buf)]
    if hasattr(lib, "sccg_reader_open"):   # (absent from builds older than the region reader: A/B runs)
        lib.sccg_reader_open.argtypes = [vp, c, sz, c, sz, ctypes.POINTER(vp)]
        lib.sccg_reader_open_device.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(vp), vp]
        lib.sccg_reader_close.argtypes = [vp]
        lib.sccg_reader_close.restype = None
        lib.sccg_reader_length.argtypes = [vp]
        lib.sccg_reader_length.restype = i64
        if hasattr(lib, "sccg_reader_has_coords"):
            lib.sccg_reader_has_coords.argtypes = [vp]
            lib.sccg_reader_has_coords.restype = ctypes.c_int
        lib.sccg_reader_header.argtypes = [vp, ctypes.POINTER(sz)]
        lib.sccg_reader_header.restype = vp
        lib.sccg_reader_fetch.argtypes = [vp, ctypes.POINTER(Region), sz, ctypes.c_uint32, ctypes.POINTER(Buf)]
        lib.sccg_reader_fetch_device.argtypes = [vp, ctypes.POINTER(Region), sz, ctypes.c_uint32, vp, sz,
                                                 ctypes.POINTER(sz), vp]
    if hasattr(lib, "sccg_reader_fetch_encoded"):   # (absent from builds older than the encoded fetch: A/B runs)
        lib.sccg_fetch_bytes_per_base.argtypes = [ctypes.POINTER(FetchFormat)]
        lib.sccg_fetch_bytes_per_base.restype = sz
        lib.sccg_reader_fetch_encoded.argtypes = [vp, ctypes.POINTER(Region), sz, c, ctypes.POINTER(FetchFormat),
                                                  ctypes.POINTER(Buf)]
        lib.sccg_reader_fetch_encoded_device.argtypes = [vp, ctypes.POINTER(Region), sz, c, ctypes.POINTER(FetchFormat),
                                                         vp, sz, ctypes.POINTER(sz), vp]
    if hasattr(lib, "sccg_reference_open"):   # (absent from builds older than the cohort fetch: A/B runs)
        lib.sccg_reference_open.argtypes = [vp, c, sz, ctypes.c_uint32, ctypes.POINTER(vp)]
        lib.sccg_reference_open_device.argtypes = [vp, vp, sz, ctypes.c_uint32, ctypes.POINTER(vp), vp]
        lib.sccg_reference_close.argtypes = [vp]
        lib.sccg_reference_close.restype = None
        lib.sccg_reference_device_bytes.argtypes = [vp]
        lib.sccg_reference_device_bytes.restype = sz
        lib.sccg_reader_open_shared.argtypes = [vp, c, sz, ctypes.POINTER(vp)]
        lib.sccg_reader_open_shared_device.argtypes = [vp, vp, sz, ctypes.POINTER(vp), vp]
        lib.sccg_reader_device_bytes.argtypes = [vp]
        lib.sccg_reader_device_bytes.restype = sz
        lib.sccg_cohort_create.argtypes = [ctypes.POINTER(vp), sz, ctypes.POINTER(vp)]
        lib.sccg_cohort_close.argtypes = [vp]
        lib.sccg_cohort_close.restype = None
        lib.sccg_cohort_samples.argtypes = [vp]
        lib.sccg_cohort_samples.restype = sz
        lib.sccg_cohort_fetch.argtypes = [vp, ctypes.POINTER(CohortRegion), sz, ctypes.POINTER(FetchFormat), ctypes.POINTER(Buf)]
        lib.sccg_cohort_fetch_device.argtypes = [vp, ctypes.POINTER(CohortRegion), sz, ctypes.POINTER(FetchFormat), vp, sz,
                                                 ctypes.POINTER(sz), vp]
    if hasattr(lib, "sccg_reader_enable_locate"):   # (absent from builds older than locate: A/B runs)
        i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(i64)
        lib.sccg_reader_enable_locate.argtypes = [vp]
        lib.sccg_reader_can_locate.argtypes = [vp]
        lib.sccg_reader_locate.argtypes = [vp, i64p, sz, i64p, i32p]
        lib.sccg_reader_locate_device.argtypes = [vp, i64p, sz, vp, vp, vp]
        lib.sccg_cohort_locate.argtypes = [vp, ctypes.POINTER(CohortLocus), sz, i64p, i32p]
        lib.sccg_cohort_locate_device.argtypes = [vp, ctypes.POINTER(CohortLocus), sz, vp, vp, vp]
    if hasattr(lib, "sccg_reader_segments"):   # (absent from builds older than segments: A/B runs)
        i64p = ctypes.POINTER(i64)
        lib.sccg_reader_segments.argtypes = [vp, ctypes.POINTER(Region), sz, i64p, ctypes.POINTER(Buf)]
        lib.sccg_reader_segments_device.argtypes = [vp, ctypes.POINTER(Region), sz, vp, vp, sz, ctypes.POINTER(sz), vp]
        lib.sccg_cohort_segments.argtypes = [vp, ctypes.POINTER(CohortRegion), sz, i64p, ctypes.POINTER(Buf)]
        lib.sccg_cohort_segments_device.argtypes = [vp, ctypes.POINTER(CohortRegion), sz, vp, vp, sz, ctypes.POINTER(sz), vp]
    if hasattr(lib, "sccg_reader_lift"):   # (absent from builds older than lift: A/B runs)
        i64p = ctypes.POINTER(i64)
        lib.sccg_reader_lift.argtypes = [vp, ctypes.POINTER(Region), sz, i64p, ctypes.POINTER(Buf)]
        lib.sccg_reader_lift_device.argtypes = [vp, ctypes.POINTER(Region), sz, vp, vp, sz, ctypes.POINTER(sz), vp]
        lib.sccg_cohort_lift.argtypes = [vp, ctypes.POINTER(CohortRegion), sz, i64p, ctypes.POINTER(Buf)]
        lib.sccg_cohort_lift_device.argtypes = [vp, ctypes.POINTER(CohortRegion), sz, vp, vp, sz, ctypes.POINTER(sz), vp]
    if hasattr(lib, "sccg_reader_find"):   # (absent from builds older than find: A/B runs)
        i64p, u8p, u32 = ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint32
        lib.sccg_find_pattern_masks.argtypes = [c, sz, u8p, u8p]
        lib.sccg_reader_find.argtypes = [vp, c, sz, ctypes.POINTER(Region), sz, u32, i64p, ctypes.POINTER(Buf)]
        lib.sccg_reader_find_device.argtypes = [vp, c, sz, ctypes.POINTER(Region), sz, u32, vp, vp, sz, ctypes.POINTER(sz), vp]
        lib.sccg_cohort_find.argtypes = [vp, c, sz, ctypes.POINTER(CohortRegion), sz, u32, i64p, ctypes.POINTER(Buf)]
        lib.sccg_cohort_find_device.argtypes = [vp, c, sz, ctypes.POINTER(CohortRegion), sz, u32, vp, vp, sz, ctypes.POINTER(sz), vp]
    if hasattr(lib, "sccg_reader_find_approx"):   # (absent from builds older than find with mismatches: A/B runs)
        i64p, u32 = ctypes.POINTER(i64), ctypes.c_uint32
        lib.sccg_reader_find_approx.argtypes = [vp, c, sz, ctypes.POINTER(Region), sz, u32, u32, i64p, ctypes.POINTER(Buf)]
        lib.sccg_reader_find_approx_device.argtypes = [vp, c, sz, ctypes.POINTER(Region), sz, u32, u32, vp, vp, sz,
                                                       ctypes.POINTER(sz), vp]
        lib.sccg_cohort_find_approx.argtypes = [vp, c, sz, ctypes.POINTER(CohortRegion), sz, u32, u32, i64p, ctypes.POINTER(Buf)]
        lib.sccg_cohort_find_approx_device.argtypes = [vp, c, sz, ctypes.POINTER(CohortRegion), sz, u32, u32, vp, vp, sz,
                                                       ctypes.POINTER(sz), vp]
    lib.sccg_profile.argtypes = [vp, ctypes.c_int]
    lib.sccg_profile_mask.argtypes = [vp, ctypes.c_uint32]
    lib.sccg_profile_get.argtypes = [vp, c, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64)]
    lib.sccg_profile_name.argtypes = [ctypes.c_int]
    lib.sccg_profile_name.restype = ctypes.c_char_p
    _lib = lib
    return lib


def header_functions() -> list[str]:
    """Every function the C ABI header declares."""
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|void|size_t|int64_t|const char\*)\s+(sccg_\w+)\s*\(", text, re.M)))


class Context:
    """One GPU context (sccg_ctx).  Not re-entrant; one per device."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.device = device
        self.ptr = ctypes.c_void_p()
        rc = self.lib.sccg_ctx_create(device, ctypes.byref(self.ptr))
        if rc:
            raise SccgError(rc, f"sccg_ctx_create(device={device}) failed: no usable GPU")

    def close(self):
        if self.ptr:
            self.lib.sccg_ctx_destroy(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, rc: int):
        raise SccgError(rc, self.lib.sccg_last_error(self.ptr).decode(errors="replace"))

    def set_option(self, option: int, value: int) -> None:
        """sccg_ctx_set_option (include/sccg.h), e.g. OPT_EXACT_SWITCH."""
        rc = self.lib.sccg_ctx_set_option(self.ptr, option, value)
        if rc:
            self._err(rc)

    def exact_switch(self, on: bool = True) -> None:
        """stats()['switch_segment'] = the reference's first switch (the in-order local pass)
        instead of any switch window (the default mode probe); the record bytes are the same."""
        self.set_option(OPT_EXACT_SWITCH, int(on))

    def stats(self) -> dict:
        st = Stats()
        self.lib.sccg_last_stats(self.ptr, ctypes.byref(st))
        return st.as_dict()

    def _take(self, buf: Buf) -> bytes:
        data = ctypes.string_at(buf.data, buf.len) if buf.data else b""
        self.lib.sccg_buf_free(ctypes.byref(buf))
        return data

    def params(self, **overrides) -> Params:
        """sccg_params: the reference's constants (compression.cpp:373-379) with `overrides` applied."""
        prm = Params()
        self.lib.sccg_params_default(ctypes.byref(prm))
        for name, v in overrides.items():
            if name not in dict(Params._fields_):
                raise TypeError(f"unknown parameter {name!r}")
            setattr(prm, name, v)
        return prm

    def compress(self, ref_fa: bytes, tgt_fa: bytes, **overrides) -> bytes:
        """Bytes of compressed_genome.txt (compression.cpp:320-580, without 7z).  Keyword overrides
        (k, k2, L, m, T1, T2, local) go through sccg_compress_ex as non-parity parameters."""
        buf = Buf()
        if overrides:
            rc = self.lib.sccg_compress_ex(self.ptr, ctypes.byref(self.params(**overrides)), ref_fa, len(ref_fa),
                                           tgt_fa, len(tgt_fa), ctypes.byref(buf))
        else:
            rc = self.lib.sccg_compress(self.ptr, ref_fa, len(ref_fa), tgt_fa, len(tgt_fa), ctypes.byref(buf))
        if rc:
            data = self._take(buf)
            err = SccgError(rc, self.lib.sccg_last_error(self.ptr).decode(errors="replace"))
            err.partial = data
            raise err
        return self._take(buf)

    def compress_files(self, ref_path: str, tgt_path: str, out_path: str, **overrides) -> int:
        """FASTA files -> record file out_path (sccg_compress_files: compression.cpp:181-220, :320-331,
        without 7z); returns the bytes written.  SCCG_E_DELTA_STOI raises after writing the file."""
        n = ctypes.c_size_t()
        prm = ctypes.byref(self.params(**overrides)) if overrides else None
        rc = self.lib.sccg_compress_files(self.ptr, prm, os.fsencode(ref_path), os.fsencode(tgt_path),
                                          os.fsencode(out_path), ctypes.byref(n))
        if rc:
            self._err(rc)
        return n.value

    def reconstruct(self, record: bytes, ref_fa: bytes) -> bytes:
        """Bytes of reconstructed_genome.fa (decompression.cpp after 7z)."""
        buf = Buf()
        rc = self.lib.sccg_reconstruct(self.ptr, ref_fa, len(ref_fa), record, len(record), ctypes.byref(buf))
        if rc:
            self._err(rc)
        return self._take(buf)

    def compress_device(self, d_ref: int, ref_len: int, d_tgt: int, tgt_len: int, d_out: int, out_cap: int,
                        stream: int = 0, **overrides) -> int:
        """HBM-resident compress: device pointers in, record text written to d_out; returns length."""
        n = ctypes.c_size_t()
        if overrides:
            rc = self.lib.sccg_compress_device_ex(self.ptr, ctypes.byref(self.params(**overrides)), d_ref, ref_len,
                                                  d_tgt, tgt_len, d_out, out_cap, ctypes.byref(n), stream or None)
        else:
            rc = self.lib.sccg_compress_device(self.ptr, d_ref, ref_len, d_tgt, tgt_len, d_out, out_cap,
                                               ctypes.byref(n), stream or None)
        if rc:
            self._err(rc)
        return n.value

    def reconstruct_device(self, d_ref: int, ref_len: int, d_rec: int, rec_len: int, d_out: int, out_cap: int,
                           stream: int = 0) -> int:
        n = ctypes.c_size_t()
        rc = self.lib.sccg_reconstruct_device(self.ptr, d_ref, ref_len, d_rec, rec_len, d_out, out_cap,
                                              ctypes.byref(n), stream or None)
        if rc:
            self._err(rc)
        return n.value

    def open_reader(self, record: bytes, ref_fa: bytes) -> "Reader":
        """A region reader over a record (sccg_reader_open): the one-time work of reconstruct, kept.
        Raises what reconstruct raises for the same bytes."""
        ptr = ctypes.c_void_p()
        rc = self.lib.sccg_reader_open(self.ptr, ref_fa, len(ref_fa), record, len(record), ctypes.byref(ptr))
        if rc:
            self._err(rc)
        return Reader(self, ptr)

    def open_reader_device(self, d_ref: int, ref_len: int, d_rec: int, rec_len: int, stream: int = 0) -> "Reader":
        """open_reader on device-resident inputs (sccg_reader_open_device)."""
        ptr = ctypes.c_void_p()
        rc = self.lib.sccg_reader_open_device(self.ptr, d_ref, ref_len, d_rec, rec_len, ctypes.byref(ptr),
                                              stream or None)
        if rc:
            self._err(rc)
        return Reader(self, ptr)

    @staticmethod
    def _forms(forms) -> int:
        bad = [f for f in forms if f not in REF_FORMS]
        if bad or not forms:
            raise ValueError(f"forms {tuple(forms)!r}: a non-empty choice of {sorted(REF_FORMS)}")
        mask = 0
        for f in forms:
            mask |= REF_FORMS[f]
        return mask

    def open_reference(self, ref_fa: bytes, forms=("erased", "kept"), coords: bool = False) -> "Reference":
        """A shared reference (sccg_reference_open): R' held once for every reader opened through it.
        forms: "erased" (records with an N-run line), "kept" (records whose N line is ","), or both.
        coords: also keep the R' -> R map (SCCG_REF_COORDS), so that readers of erased-form records
        can say where on the reference a base comes from (the "origin" encoding)."""
        ptr = ctypes.c_void_p()
        rc = self.lib.sccg_reference_open(self.ptr, ref_fa, len(ref_fa), self._forms(forms) | (REF_COORDS if coords else 0),
                                          ctypes.byref(ptr))
        if rc:
            self._err(rc)
        return Reference(self, ptr)

    def open_reference_device(self, d_ref: int, ref_len: int, forms=("erased", "kept"), stream: int = 0,
                              coords: bool = False) -> "Reference":
        """open_reference on a device-resident FASTA (sccg_reference_open_device)."""
        ptr = ctypes.c_void_p()
        rc = self.lib.sccg_reference_open_device(self.ptr, d_ref, ref_len, self._forms(forms) | (REF_COORDS if coords else 0),
                                                 ctypes.byref(ptr), stream or None)
        if rc:
            self._err(rc)
        return Reference(self, ptr)

    def profile(self, enable: bool = True, families: list | None = None) -> None:
        """Reset and enable (or disable) per-kernel HIP-event timing; `families` (names from
        sccg_profile_name) limits the bracketed launches to those families."""
        if enable and families:
            mask, i = 0, 0
            while True:
                name = self.lib.sccg_profile_name(i)
                if not name:
                    break
                if name.decode() in families:
                    mask |= 1 << i
                i += 1
            if not mask:
                raise ValueError(f"profile: unknown kernel families {families}")
            self.lib.sccg_profile_mask(self.ptr, mask)
            return
        self.lib.sccg_profile(self.ptr, int(enable))

    def profile_get(self) -> dict:
        """{kernel family: (total_ms, launches)} since the last profile() call."""
        out, i = {}, 0
        while True:
            name = self.lib.sccg_profile_name(i)
            if not name:
                return out
            ms, n = ctypes.c_double(), ctypes.c_int64()
            self.lib.sccg_profile_get(self.ptr, name, ctypes.byref(ms), ctypes.byref(n))
            if n.value:
                out[name.decode()] = (ms.value, n.value)
            i += 1

    def compress_bound(self, ref_len: int, tgt_len: int) -> int:
        return self.lib.sccg_compress_bound(ref_len, tgt_len)

    @staticmethod
    def compress_bound_static(ref_len: int, tgt_len: int) -> int:
        """sccg_compress_bound without a context (it needs no device)."""
        return load_library().sccg_compress_bound(ref_len, tgt_len)

    def _walk_out(self, rc: int, recs: Records, ex) -> tuple[list, tuple[int, int]]:
        try:
            if rc:
                self._err(rc)
            out = [(recs.t[i], recs.pos[i], recs.len[i]) for i in range(recs.n)]
        finally:   # (the library frees on its own error paths too; freeing zeroed records is a no-op)
            self.lib.sccg_records_free(ctypes.byref(recs))
        return out, (ex[0], ex[1])

    def walk_range(self, sr: bytes, st: bytes, k: int, m: int, x0: int, p0: int, x_end: int):
        """The global walk (compression.cpp:64-161) from state (x0, P0) until index >= x_end on the
        N-erased uppercase R', T' (sccg_walk_range): ([(t, p, l)], (exit index, exit P))."""
        recs, ex = Records(), (ctypes.c_int64 * 2)()
        rc = self.lib.sccg_walk_range(self.ptr, sr, len(sr), st, len(st), k, m, x0, p0, x_end, ctypes.byref(recs), ex)
        return self._walk_out(rc, recs, ex)

    def walk_range_device(self, d_r: int, nr: int, d_t: int, nt: int, k: int, m: int, x0: int, p0: int, x_end: int,
                          stream: int = 0):
        """walk_range on device-resident R', T' (sccg_walk_range_device)."""
        recs, ex = Records(), (ctypes.c_int64 * 2)()
        rc = self.lib.sccg_walk_range_device(self.ptr, d_r, nr, d_t, nt, k, m, x0, p0, x_end, ctypes.byref(recs), ex,
                                             stream or None)
        return self._walk_out(rc, recs, ex)

    def match(self, sr: bytes, st: bytes, k: int, m: int, glob: bool, offset: int = 0):
        """match_sequences (compression.cpp:36) -> [(kind, p, l, t)] like the oracle's records."""
        recs = Records()
        rc = self.lib.sccg_match(self.ptr, sr, len(sr), st, len(st), k, m, int(glob), offset, ctypes.byref(recs))
        if rc:
            self._err(rc)
        out = [(recs.kind[i], recs.pos[i] if recs.kind[i] else 0, recs.len[i], recs.t[i]) for i in range(recs.n)]
        self.lib.sccg_records_free(ctypes.byref(recs))
        return out


class Reference:
    """sccg_reference: R' shared by the readers opened through it.  close() drops this object's hold;
    the device memory goes with the last of its readers."""

    def __init__(self, ctx: Context, ptr: ctypes.c_void_p):
        self.ctx, self.lib, self.ptr = ctx, ctx.lib, ptr

    def close(self):
        if self.ptr:
            self.lib.sccg_reference_close(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def device_bytes(self) -> int:
        """Device bytes of the forms held (sccg_reference_device_bytes)."""
        return self.lib.sccg_reference_device_bytes(self.ptr)

    def open_reader(self, record: bytes) -> "Reader":
        """Context.open_reader without the strip and without a private R' (sccg_reader_open_shared)."""
        if not self.ptr:
            raise ValueError("the reference is closed")
        ptr = ctypes.c_void_p()
        rc = self.lib.sccg_reader_open_shared(self.ptr, record, len(record), ctypes.byref(ptr))
        if rc:
            self.ctx._err(rc)
        return Reader(self.ctx, ptr)

    def open_reader_device(self, d_rec: int, rec_len: int, stream: int = 0) -> "Reader":
        """open_reader on a device-resident record (sccg_reader_open_shared_device)."""
        if not self.ptr:
            raise ValueError("the reference is closed")
        ptr = ctypes.c_void_p()
        rc = self.lib.sccg_reader_open_shared_device(self.ptr, d_rec, rec_len, ctypes.byref(ptr), stream or None)
        if rc:
            self.ctx._err(rc)
        return Reader(self.ctx, ptr)


class Reader:
    """sccg_reader: ranges of the target read from a record without rebuilding it.  It owns its
    device memory (independent of later calls on the context); close it before the context."""

    def __init__(self, ctx: Context, ptr: ctypes.c_void_p):
        self.ctx, self.lib, self.ptr = ctx, ctx.lib, ptr

    def close(self):
        if self.ptr:
            self.lib.sccg_reader_close(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def length(self) -> int:
        """Bases in the sequence (the FASTA body without its line ends)."""
        return self.lib.sccg_reader_length(self.ptr)

    @property
    def has_coords(self) -> bool:
        """Whether the "origin" encoding works on this reader (sccg_reader_has_coords): its record's N
        line is ",", or it was opened through a Reference with coords=True."""
        return bool(self.lib.sccg_reader_has_coords(self.ptr))

    @property
    def device_bytes(self) -> int:
        """The reader's own persistent device allocation (sccg_reader_device_bytes): without R' when
        it was opened through a Reference."""
        return self.lib.sccg_reader_device_bytes(self.ptr)

    @property
    def header(self) -> bytes:
        """The record's header line ('>' included) without its line end; b"" when it has none."""
        n = ctypes.c_size_t()
        p = self.lib.sccg_reader_header(self.ptr, ctypes.byref(n))
        return ctypes.string_at(p, n.value) if n.value else b""

    @staticmethod
    def _regions(regions):
        regions = list(regions)
        arr = (Region * len(regions))(*[(int(b), int(e)) for b, e in regions]) if regions else None
        return regions, arr

    def fetch(self, regions, upper: bool = False) -> list[bytes]:
        """One bytes object per (begin, end) pair (0-based, half-open), from one batched call."""
        regions, arr = self._regions(regions)
        buf = Buf()
        rc = self.lib.sccg_reader_fetch(self.ptr, arr, len(regions), FETCH_UPPER if upper else 0, ctypes.byref(buf))
        if rc:
            self.ctx._err(rc)
        data = self.ctx._take(buf)
        out, at = [], 0
        for b, e in regions:
            out.append(data[at:at + (e - b)])
            at += e - b
        return out

    def fetch_device(self, regions, d_out: int, out_cap: int, upper: bool = False, stream: int = 0) -> int:
        """The regions' bases concatenated into device memory d_out (capacity out_cap); returns their
        length.  d_out = 0 is a size query; a capacity too small raises SCCG_E_NOMEM with the size
        needed in the error's `needed`."""
        regions, arr = self._regions(regions)
        n = ctypes.c_size_t()
        rc = self.lib.sccg_reader_fetch_device(self.ptr, arr, len(regions), FETCH_UPPER if upper else 0,
                                               d_out or None, out_cap, ctypes.byref(n), stream or None)
        if rc:
            err = SccgError(rc, self.lib.sccg_last_error(self.ctx.ptr).decode(errors="replace"))
            err.needed = n.value
            raise err
        return n.value

    @staticmethod
    def _format(encoding: str, dtype: str, revcomp: bool, upper: bool) -> FetchFormat:
        if encoding not in ENCODINGS or dtype not in DTYPES:
            raise ValueError(f"encoding {encoding!r} / dtype {dtype!r}: one of {sorted(ENCODINGS)} / {sorted(DTYPES)}")
        return FetchFormat(ENCODINGS[encoding], DTYPES[dtype], (FETCH_UPPER if upper else 0) | (FETCH_REVCOMP if revcomp else 0), 0)

    @staticmethod
    def _strand(strand, n: int):
        if strand is None:
            return None
        strand = bytes(1 if x else 0 for x in strand)
        if len(strand) != n:
            raise ValueError(f"{len(strand)} strands for {n} regions")
        return strand or None

    def fetch_encoded(self, regions, encoding: str = "index", dtype: str = "u8", strand=None, revcomp: bool = False,
                      upper: bool = False) -> bytes:
        """The regions' bases concatenated and encoded (sccg_reader_fetch_encoded): "ascii" and
        "index" (A 0, C 1, G 2, T 3, other 4) one byte per base, "onehot" four `dtype` elements per
        base.  strand: one truthy / falsy value per region, truthy = reverse complement; revcomp:
        all of them.  "origin" (dtype "i32"): one little-endian int32 per base -- the 0-based
        position in the reference sequence a token copied it from, ORIGIN_LITERAL (-1) for a literal of
        the record, ORIGIN_N (-2) inside one of the target's N runs; a reversed region's values come
        in reverse order, unchanged.  It needs has_coords."""
        regions, arr = self._regions(regions)
        fmt = self._format(encoding, dtype, revcomp, upper)
        buf = Buf()
        rc = self.lib.sccg_reader_fetch_encoded(self.ptr, arr, len(regions), self._strand(strand, len(regions)),
                                                ctypes.byref(fmt), ctypes.byref(buf))
        if rc:
            self.ctx._err(rc)
        return self.ctx._take(buf)

    def fetch_encoded_device(self, regions, d_out: int, out_cap: int, encoding: str = "index", dtype: str = "u8", strand=None,
                             revcomp: bool = False, upper: bool = False, stream: int = 0) -> int:
        """fetch_encoded into device memory d_out (capacity out_cap bytes, aligned to the element);
        returns the bytes written.  d_out = 0 is a size query; a capacity too small raises
        SCCG_E_NOMEM with the bytes needed in the error's `needed`."""
        regions, arr = self._regions(regions)
        fmt = self._format(encoding, dtype, revcomp, upper)
        n = ctypes.c_size_t()
        rc = self.lib.sccg_reader_fetch_encoded_device(self.ptr, arr, len(regions), self._strand(strand, len(regions)),
                                                       ctypes.byref(fmt), d_out or None, out_cap, ctypes.byref(n),
                                                       stream or None)
        if rc:
            err = SccgError(rc, self.lib.sccg_last_error(self.ctx.ptr).decode(errors="replace"))
            err.needed = n.value
            raise err
        return n.value

    def fetch_tensor(self, regions, encoding: str = "onehot", dtype=None, strand=None, revcomp: bool = False, stream=None):
        """A torch tensor on the context's device: [n, L] ("index", "ascii": uint8; "origin": int32) or [n, L, 4]
        ("onehot": dtype, default torch.float16) when every region has the same length L, else flat
        [F] / [F, 4].  stream: a torch stream (default: the current one)."""
        import torch
        regions = [(int(b), int(e)) for b, e in regions]
        names = {torch.uint8: "u8", torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32", torch.int32: "i32"}
        if encoding == "origin":
            dtype = torch.int32 if dtype is None else dtype
            if dtype != torch.int32:
                raise ValueError("'origin' is int32")
        elif encoding != "onehot":
            dtype = torch.uint8 if dtype is None else dtype
            if dtype != torch.uint8:
                raise ValueError(f"{encoding!r} is uint8")
        elif dtype is None:
            dtype = torch.float16
        if dtype not in names:
            raise ValueError(f"dtype {dtype}: one of {list(names)}")
        dev = torch.device("cuda", self.ctx.device)
        F = sum(e - b for b, e in regions)
        shape = (F, 4) if encoding == "onehot" else (F,)
        out = torch.empty(shape, dtype=dtype, device=dev)
        s = torch.cuda.current_stream(dev) if stream is None else stream
        self.fetch_encoded_device(regions, out.data_ptr(), out.numel() * out.element_size(), encoding, names[dtype], strand,
                                  revcomp, stream=s.cuda_stream)
        lens = {e - b for b, e in regions}
        if len(lens) == 1 and regions:
            out = out.view(len(regions), lens.pop(), *shape[1:])
        return out

    def enable_locate(self) -> None:
        """Build the locate index on the device (sccg_reader_enable_locate; a second call does
        nothing).  Needs has_coords.  Enable it before the reader joins a Cohort that is to locate in it."""
        rc = self.lib.sccg_reader_enable_locate(self.ptr)
        if rc:
            self.ctx._err(rc)

    @property
    def can_locate(self) -> bool:
        return bool(self.lib.sccg_reader_can_locate(self.ptr))

    def locate(self, ref_positions):
        """(pos int64 [n], copies int32 [n]) for 0-based positions of the reference sequence: the first
        sequence position a token copied each from (LOCATE_NONE: none; LOCATE_REF_N: an erased N of the
        reference) and how many sequence positions hold a copy.  One launch per call."""
        import numpy as np
        q = np.ascontiguousarray(ref_positions, dtype=np.int64).reshape(-1)
        pos, copies = np.empty(q.size, dtype=np.int64), np.empty(q.size, dtype=np.int32)
        i64p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
        rc = self.lib.sccg_reader_locate(self.ptr, q.ctypes.data_as(i64p), q.size, pos.ctypes.data_as(i64p), copies.ctypes.data_as(i32p))
        if rc:
            self.ctx._err(rc)
        return pos, copies

    def segments(self, regions):
        """The regions' alignment to the reference, run-length coded (sccg_reader_segments): (off int64 [n + 1],
        seg int64 [m, 3]) -- region i's segments are seg[off[i]:off[i + 1]], rows (pos, len, ref): `len` bases
        from sequence position `pos` copied from reference positions ref, ref + 1, ... (ref >= 0), all
        literals (ref -1) or all of a target N run (ref -2); maximal, tiling the region.  Needs has_coords."""
        regions, arr = self._regions(regions)
        return _segments_host(self.ctx, self.lib.sccg_reader_segments, self.ptr, arr, len(regions))

    def segments_tensor(self, regions, stream=None):
        """segments() into torch tensors on the context's device."""
        regions, arr = self._regions(regions)
        return _segments_tensor(self.ctx, self.lib.sccg_reader_segments_device, self.ptr, arr, len(regions), stream)

    def lift(self, intervals):
        """Intervals of the reference onto this sample, run-length coded (sccg_reader_lift): (off int64 [n + 1],
        blk int64 [m, 3]) -- interval i's blocks are blk[off[i]:off[i + 1]], rows (ref, len, pos): `len`
        reference bases from `ref` lie at sequence positions pos, pos + 1, ... (pos >= 0), have no copy (pos
        LOCATE_NONE) or are one erased N run of the reference (pos LOCATE_REF_N); maximal, tiling the interval.
        What locate() says per base.  Needs can_locate."""
        intervals, arr = self._regions(intervals)
        return _segments_host(self.ctx, self.lib.sccg_reader_lift, self.ptr, arr, len(intervals))

    def lift_tensor(self, intervals, stream=None):
        """lift() into torch tensors on the context's device."""
        intervals, arr = self._regions(intervals)
        return _segments_tensor(self.ctx, self.lib.sccg_reader_lift_device, self.ptr, arr, len(intervals), stream)

    def find(self, pattern, regions, strands="both"):
        """Where an IUPAC pattern (str or bytes, 1 to FIND_MAX_PATTERN letters of ACGTURYSWKMBDHVN, case-blind)
        occurs in the regions (sccg_reader_find): (off int64 [n + 1], hits int64 [h, 2]) -- region i's hits are
        hits[off[i]:off[i + 1]], rows (pos, strand) in ascending pos, forward (0) before reverse (1); a reverse
        hit is reported at the leftmost forward position of its window.  strands: "both", "+" or "-".  A
        sequence base that is not A, C, G or T matches no letter, not even N."""
        regions, arr = self._regions(regions)
        pat, flags = _find_args(pattern, strands)
        return _segments_host(self.ctx, self.lib.sccg_reader_find, self.ptr, arr, len(regions), cols=2, head=(pat, len(pat)),
                              mid=(flags,))

    def find_tensor(self, pattern, regions, strands="both", stream=None):
        """find() into torch tensors on the context's device."""
        regions, arr = self._regions(regions)
        pat, flags = _find_args(pattern, strands)
        return _segments_tensor(self.ctx, self.lib.sccg_reader_find_device, self.ptr, arr, len(regions), stream, cols=2,
                                head=(pat, len(pat)), mid=(flags,))

    def find_approx(self, pattern, regions, mismatches, strands="both"):
        """find() within `mismatches` substitutions (sccg_reader_find_approx; 0 <= mismatches <= FIND_MAX_MISMATCHES,
        fewer than the pattern's letters): (off int64 [n + 1], hits int64 [h, 3]), rows (pos, strand, mismatches) in
        find()'s order.  A sequence base that is not A, C, G or T is a mismatch against every letter, N included."""
        regions, arr = self._regions(regions)
        pat, flags = _find_args(pattern, strands)
        return _segments_host(self.ctx, self.lib.sccg_reader_find_approx, self.ptr, arr, len(regions), cols=3,
                              head=(pat, len(pat)), mid=(flags, _find_mismatches(mismatches)))

    def find_approx_tensor(self, pattern, regions, mismatches, strands="both", stream=None):
        """find_approx() into torch tensors on the context's device."""
        regions, arr = self._regions(regions)
        pat, flags = _find_args(pattern, strands)
        return _segments_tensor(self.ctx, self.lib.sccg_reader_find_approx_device, self.ptr, arr, len(regions), stream, cols=3,
                                head=(pat, len(pat)), mid=(flags, _find_mismatches(mismatches)))

    def locate_tensor(self, ref_positions, stream=None):
        """locate() into torch tensors on the context's device: (pos int64 [n], copies int32 [n])."""
        import numpy as np
        import torch
        q = np.ascontiguousarray(ref_positions, dtype=np.int64).reshape(-1)
        dev = torch.device("cuda", self.ctx.device)
        pos, copies = torch.empty(q.size, dtype=torch.int64, device=dev), torch.empty(q.size, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev) if stream is None else stream
        rc = self.lib.sccg_reader_locate_device(self.ptr, q.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), q.size,
                                                pos.data_ptr() or None, copies.data_ptr() or None, s.cuda_stream or None)
        if rc:
            self.ctx._err(rc)
        return pos, copies


def _segments_host(ctx, call, ptr, arr, n, cols=3, head=(), mid=()):
    """(off int64 [n + 1], rows int64 [m, cols]) of a host segments, lift or find call (sccg_*_segments, sccg_*_lift,
    sccg_*_find: head = its pattern arguments before the region list, mid = its flags behind it)."""
    import numpy as np
    off = np.zeros(n + 1, dtype=np.int64)
    buf = Buf()
    rc = call(ptr, *head, arr, n, *mid, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.byref(buf))
    if rc:
        ctx._err(rc)
    return off, np.frombuffer(ctx._take(buf), dtype="<i8").reshape(-1, cols).copy()


def _segments_tensor(ctx, call, ptr, arr, n, stream, cols=3, head=(), mid=()):
    """The same pair as device tensors (sccg_*_segments_device, sccg_*_lift_device, sccg_*_find_device): one call to
    size, one into exactly-sized tensors."""
    import torch
    dev = torch.device("cuda", ctx.device)
    s = torch.cuda.current_stream(dev) if stream is None else stream
    m = ctypes.c_size_t()
    rc = call(ptr, *head, arr, n, *mid, None, None, 0, ctypes.byref(m), s.cuda_stream or None)
    if rc:
        ctx._err(rc)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    seg = torch.empty((m.value, cols), dtype=torch.int64, device=dev)
    if m.value:
        rc = call(ptr, *head, arr, n, *mid, off.data_ptr(), seg.data_ptr(), m.value, ctypes.byref(m), s.cuda_stream or None)
        if rc:
            ctx._err(rc)
    return off, seg


def _find_args(pattern, strands):
    """A find call's pattern as bytes and its strand flags."""
    pat = pattern.encode("latin-1") if isinstance(pattern, str) else bytes(pattern)
    if strands not in FIND_STRANDS:
        raise ValueError(f'strands is "both", "+" or "-", not {strands!r}')
    return pat, FIND_STRANDS[strands]


def _find_mismatches(mismatches):
    """A find_approx call's mismatch bound as the uint32 the library takes (it checks the range)."""
    k = int(mismatches)
    if k < 0 or k > 0xFFFFFFFF:
        raise ValueError(f"mismatches is 0 to {FIND_MAX_MISMATCHES}, not {mismatches!r}")
    return k


def find_pattern_masks(pattern):
    """The 4-bit masks (bit 0 A, 1 C, 2 G, 3 T) of an IUPAC pattern and of its reverse complement
    (sccg_find_pattern_masks; no GPU): (fwd, rev), bytes of the pattern's length.  ValueError for a pattern that is
    empty, longer than FIND_MAX_PATTERN or holds a byte outside ACGTURYSWKMBDHVN (either case)."""
    lib = load_library()
    pat = pattern.encode("latin-1") if isinstance(pattern, str) else bytes(pattern)
    fwd, rev = (ctypes.c_uint8 * max(len(pat), 1))(), (ctypes.c_uint8 * max(len(pat), 1))()
    if lib.sccg_find_pattern_masks(pat, len(pat), fwd, rev):
        raise ValueError(f"not an IUPAC pattern of 1 to {FIND_MAX_PATTERN} letters: {pattern!r}")
    return bytes(fwd[:len(pat)]), bytes(rev[:len(pat)])


class Cohort:
    """sccg_cohort: the encoded fetch over many readers of one context, each region naming its sample,
    in one launch per call.  It keeps references to its Readers but does not own them: close the
    cohort before them."""

    def __init__(self, readers):
        self.readers = list(readers)
        if not self.readers:
            raise ValueError("a cohort needs at least one reader")
        self.ctx = self.readers[0].ctx
        self.lib = self.ctx.lib
        arr = (ctypes.c_void_p * len(self.readers))(*[r.ptr.value for r in self.readers])
        self.ptr = ctypes.c_void_p()
        rc = self.lib.sccg_cohort_create(arr, len(self.readers), ctypes.byref(self.ptr))
        if rc:
            self.ctx._err(rc)

    def close(self):
        if self.ptr:
            self.lib.sccg_cohort_close(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def samples(self) -> int:
        return self.lib.sccg_cohort_samples(self.ptr)

    @staticmethod
    def _items(items):
        """(sample, begin, end) or (sample, begin, end, reverse) -> sccg_cohort_region array."""
        items = [tuple(it) for it in items]
        rows = [(int(it[1]), int(it[2]), int(it[0]), 1 if len(it) > 3 and it[3] else 0) for it in items]
        return rows, ((CohortRegion * len(rows))(*rows) if rows else None)

    def fetch_encoded(self, items, encoding: str = "index", dtype: str = "u8", revcomp: bool = False, upper: bool = False) -> bytes:
        """The items' bases concatenated and encoded as Reader.fetch_encoded does (sccg_cohort_fetch).
        items: (sample, begin, end) or (sample, begin, end, reverse); revcomp: all of them reversed."""
        rows, arr = self._items(items)
        fmt = Reader._format(encoding, dtype, revcomp, upper)
        buf = Buf()
        rc = self.lib.sccg_cohort_fetch(self.ptr, arr, len(rows), ctypes.byref(fmt), ctypes.byref(buf))
        if rc:
            self.ctx._err(rc)
        return self.ctx._take(buf)

    def fetch_encoded_device(self, items, d_out: int, out_cap: int, encoding: str = "index", dtype: str = "u8",
                             revcomp: bool = False, upper: bool = False, stream: int = 0) -> int:
        """fetch_encoded into device memory d_out (capacity out_cap bytes, aligned to the element);
        returns the bytes written.  d_out = 0 is a size query; a capacity too small raises
        SCCG_E_NOMEM with the bytes needed in the error's `needed`."""
        rows, arr = self._items(items)
        fmt = Reader._format(encoding, dtype, revcomp, upper)
        n = ctypes.c_size_t()
        rc = self.lib.sccg_cohort_fetch_device(self.ptr, arr, len(rows), ctypes.byref(fmt), d_out or None, out_cap,
                                               ctypes.byref(n), stream or None)
        if rc:
            err = SccgError(rc, self.lib.sccg_last_error(self.ctx.ptr).decode(errors="replace"))
            err.needed = n.value
            raise err
        return n.value

    def fetch_tensor(self, items, encoding: str = "onehot", dtype=None, revcomp: bool = False, stream=None):
        """Reader.fetch_tensor over the cohort: [n, L] or [n, L, 4] when every item has the same
        length L, else flat [F] / [F, 4]."""
        import torch
        items = [tuple(it) for it in items]
        names = {torch.uint8: "u8", torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32", torch.int32: "i32"}
        if encoding == "origin":
            dtype = torch.int32 if dtype is None else dtype
            if dtype != torch.int32:
                raise ValueError("'origin' is int32")
        elif encoding != "onehot":
            dtype = torch.uint8 if dtype is None else dtype
            if dtype != torch.uint8:
                raise ValueError(f"{encoding!r} is uint8")
        elif dtype is None:
            dtype = torch.float16
        if dtype not in names:
            raise ValueError(f"dtype {dtype}: one of {list(names)}")
        dev = torch.device("cuda", self.ctx.device)
        F = sum(int(it[2]) - int(it[1]) for it in items)
        shape = (F, 4) if encoding == "onehot" else (F,)
        out = torch.empty(shape, dtype=dtype, device=dev)
        s = torch.cuda.current_stream(dev) if stream is None else stream
        self.fetch_encoded_device(items, out.data_ptr(), out.numel() * out.element_size(), encoding, names[dtype], revcomp,
                                  stream=s.cuda_stream)
        lens = {int(it[2]) - int(it[1]) for it in items}
        if len(lens) == 1 and items:
            out = out.view(len(items), lens.pop(), *shape[1:])
        return out

    def segments(self, items):
        """Reader.segments over the cohort (sccg_cohort_segments): items (sample, begin, end), forward only."""
        rows, arr = self._items(items)
        return _segments_host(self.ctx, self.lib.sccg_cohort_segments, self.ptr, arr, len(rows))

    def segments_tensor(self, items, stream=None):
        """segments() into torch tensors on the context's device."""
        rows, arr = self._items(items)
        return _segments_tensor(self.ctx, self.lib.sccg_cohort_segments_device, self.ptr, arr, len(rows), stream)

    def lift(self, items):
        """Reader.lift over the cohort (sccg_cohort_lift): items (sample, begin, end) of each sample's reference.
        A sample answers only if its reader had enable_locate() called before this cohort was created."""
        rows, arr = self._items(items)
        return _segments_host(self.ctx, self.lib.sccg_cohort_lift, self.ptr, arr, len(rows))

    def lift_tensor(self, items, stream=None):
        """lift() into torch tensors on the context's device."""
        rows, arr = self._items(items)
        return _segments_tensor(self.ctx, self.lib.sccg_cohort_lift_device, self.ptr, arr, len(rows), stream)

    def find(self, pattern, items, strands="both"):
        """Reader.find over the cohort (sccg_cohort_find): items (sample, begin, end); the strands are the call's."""
        rows, arr = self._items(items)
        pat, flags = _find_args(pattern, strands)
        return _segments_host(self.ctx, self.lib.sccg_cohort_find, self.ptr, arr, len(rows), cols=2, head=(pat, len(pat)),
                              mid=(flags,))

    def find_tensor(self, pattern, items, strands="both", stream=None):
        """find() into torch tensors on the context's device."""
        rows, arr = self._items(items)
        pat, flags = _find_args(pattern, strands)
        return _segments_tensor(self.ctx, self.lib.sccg_cohort_find_device, self.ptr, arr, len(rows), stream, cols=2,
                                head=(pat, len(pat)), mid=(flags,))

    def find_approx(self, pattern, items, mismatches, strands="both"):
        """Reader.find_approx over the cohort (sccg_cohort_find_approx): items (sample, begin, end)."""
        rows, arr = self._items(items)
        pat, flags = _find_args(pattern, strands)
        return _segments_host(self.ctx, self.lib.sccg_cohort_find_approx, self.ptr, arr, len(rows), cols=3,
                              head=(pat, len(pat)), mid=(flags, _find_mismatches(mismatches)))

    def find_approx_tensor(self, pattern, items, mismatches, strands="both", stream=None):
        """find_approx() into torch tensors on the context's device."""
        rows, arr = self._items(items)
        pat, flags = _find_args(pattern, strands)
        return _segments_tensor(self.ctx, self.lib.sccg_cohort_find_approx_device, self.ptr, arr, len(rows), stream, cols=3,
                                head=(pat, len(pat)), mid=(flags, _find_mismatches(mismatches)))

    @staticmethod
    def _loci(items):
        """(sample, ref_pos) -> sccg_cohort_locus array."""
        rows = [(int(r), int(s), 0) for s, r in items]
        return rows, ((CohortLocus * len(rows))(*rows) if rows else None)

    def locate(self, items):
        """Reader.locate over the cohort (sccg_cohort_locate): items (sample, ref_pos) -> (pos int64 [n],
        copies int32 [n]), one launch.  A sample answers only if its reader had enable_locate() called
        before this cohort was created."""
        import numpy as np
        rows, arr = self._loci(items)
        pos, copies = np.empty(len(rows), dtype=np.int64), np.empty(len(rows), dtype=np.int32)
        rc = self.lib.sccg_cohort_locate(self.ptr, arr, len(rows), pos.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                         copies.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        if rc:
            self.ctx._err(rc)
        return pos, copies

    def locate_tensor(self, items, stream=None):
        """locate() into torch tensors on the context's device."""
        import torch
        rows, arr = self._loci(items)
        dev = torch.device("cuda", self.ctx.device)
        pos, copies = torch.empty(len(rows), dtype=torch.int64, device=dev), torch.empty(len(rows), dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev) if stream is None else stream
        rc = self.lib.sccg_cohort_locate_device(self.ptr, arr, len(rows), pos.data_ptr() or None, copies.data_ptr() or None,
                                                s.cuda_stream or None)
        if rc:
            self.ctx._err(rc)
        return pos, copies

    def fetch_tensor_at(self, items, length: int, encoding: str = "onehot", dtype=None, revcomp: bool = False):
        """The window of `length` bases that starts where reference position ref_pos lies in each sample:
        items (sample, ref_pos) -> (tensor [n, length] or [n, length, 4] as fetch_tensor gives it, found
        bool [n]).  A row is zero and not found when the position has no copy in the sample (locate()'s
        negative answers) or the window would pass the sample's end.  One locate and one fetch launch."""
        import torch
        items = [(int(s), int(r)) for s, r in items]
        length = int(length)
        if length <= 0:
            raise ValueError("fetch_tensor_at: length must be positive")
        pos, _ = self.locate(items)
        found = [p >= 0 and p + length <= self.readers[s].length for (s, _), p in zip(items, pos.tolist())]
        windows = [(s, int(p), int(p) + length) for (s, _), p, f in zip(items, pos.tolist(), found) if f]
        dev = torch.device("cuda", self.ctx.device)
        mask = torch.tensor(found, dtype=torch.bool, device=dev)
        if len(windows) == len(items) and items:
            return self.fetch_tensor(windows, encoding, dtype, revcomp), mask
        got = self.fetch_tensor(windows, encoding, dtype, revcomp)   # (none found: the empty fetch, for its dtype checks)
        out = torch.zeros((len(items), length) + ((4,) if encoding == "onehot" else ()), dtype=got.dtype, device=dev)
        if windows:
            out[mask] = got.view(len(windows), length, *out.shape[2:])
        return out, mask
