"""One hand-built record (tests/recgen.py) through every entry point of the decoder, against the
oracle's answer and the class rule.  Shared by test_gpu_record_edges.py and its child processes."""
from __future__ import annotations

import ctypes
import hashlib

import fetchlib
import oraclelib
import recgen
from pkg import sccg

E = sccg.ERR_CODES
FAILS = (E["SCCG_E_FORMAT"], E["SCCG_E_PARSE"], E["SCCG_E_RANGE"])


def oracle(c):
    """(0, FASTA) or (oracle status, None)"""
    try:
        return 0, oraclelib.decompress(c.record, c.ref_fa)
    except oraclelib.OracleError as e:
        return e.rc, None


def status_of(f):
    try:
        return 0, f()
    except sccg.SccgError as e:
        return e.rc, None


def class_rule(c, rc, fa, want_fa):
    """The outcome the case's class allows; returns "bytes" or the status name."""
    name = c.name
    if c.klass == recgen.EXACT:
        assert rc == 0, f"{name}: status {rc}, the oracle succeeds"
        assert fa == want_fa, f"{name}: bytes differ from the oracle's"
    elif c.klass == recgen.REJECT_OK:
        assert rc in (0, E["SCCG_E_PARSE"]), f"{name}: status {rc}, only the oracle's bytes or SCCG_E_PARSE"
        assert rc or fa == want_fa, f"{name}: accepted with bytes that differ from the oracle's"
    else:
        assert want_fa is None, f"{name}: the oracle succeeds on an `error` case"
        assert rc in FAILS, f"{name}: status {rc}, the oracle fails"
        assert rc == E[c.expect], f"{name}: status {rc}, want {c.expect}"
    return "bytes" if rc == 0 else sccg.ERRORS[rc]


class Env:
    """A context, the references on the device and as shared references opened with both forms."""

    def __init__(self, device: int = 0):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", device)
        torch.zeros(1, device=self.dev)   # torch's HIP runtime before the library context
        self.ctx = sccg.Context(device)
        self.d_refs, self.shared = {}, {}

    def close(self):
        for r in self.shared.values():
            r.close()
        self.ctx.close()

    def dev_bytes(self, b: bytes):
        return self.torch.frombuffer(bytearray(b), dtype=self.torch.uint8).to(self.dev)

    def d_ref(self, ref_fa: bytes):
        if ref_fa not in self.d_refs:
            self.d_refs[ref_fa] = self.dev_bytes(ref_fa)
        return self.d_refs[ref_fa]

    def shared_ref(self, ref_fa: bytes):
        if ref_fa not in self.shared:
            self.shared[ref_fa] = self.ctx.open_reference(ref_fa, forms=("erased", "kept"))
        return self.shared[ref_fa]

    def reconstruct_device(self, c, d_rec, d_out: int, cap: int):
        """(status, *out_len) of sccg_reconstruct_device, the length also on failure"""
        n = ctypes.c_size_t()
        rc = self.ctx.lib.sccg_reconstruct_device(self.ctx.ptr, self.d_ref(c.ref_fa).data_ptr(), len(c.ref_fa), d_rec.data_ptr(),
                                                  len(c.record), d_out or None, cap, ctypes.byref(n), None)
        return rc, n.value


def windows(probes, length: int):
    """Every 1- to 3-base window within 70 bases of a probe position."""
    out = set()
    for p in probes:
        for b in range(max(0, p - 70), min(length, p + 70)):
            for w in (1, 2, 3):
                if b + w <= length:
                    out.add((b, b + w))
    return sorted(out)


def check_reconstruct(env: Env, c, want_fa, frozen=None) -> tuple[int, bytes | None, str]:
    """sccg_reconstruct and the three device forms; returns (status, bytes, outcome)."""
    torch = env.torch
    rc, fa = status_of(lambda: env.ctx.reconstruct(c.record, c.ref_fa))
    outcome = class_rule(c, rc, fa, want_fa)
    if frozen is not None and frozen["rc"] is not None and rc == 0:   # the compiled reference's own answer
        assert frozen["rc"] == 0 and (hashlib.sha256(fa).hexdigest(), len(fa)) == (frozen["fasta_sha256"], frozen["fasta_len"]), c.name
    d_rec = env.dev_bytes(c.record)
    qrc, need = env.reconstruct_device(c, d_rec, 0, 0)                      # size query
    assert qrc == rc, f"{c.name}: the size query returns {qrc}, reconstruct {rc}"
    if rc:
        d_o = torch.full((4096,), 0xAA, dtype=torch.uint8, device=env.dev)
        drc, _ = env.reconstruct_device(c, d_rec, d_o.data_ptr(), 4096)
        assert drc == rc, f"{c.name}: the device form returns {drc}, reconstruct {rc}"
        return rc, None, outcome
    assert need == len(fa), f"{c.name}: the size query gives {need}, the output has {len(fa)}"
    d_o = torch.full((need + 64,), 0xAA, dtype=torch.uint8, device=env.dev)
    src, sneed = env.reconstruct_device(c, d_rec, d_o.data_ptr(), need - 1)  # one byte short
    torch.cuda.synchronize()
    assert src == E["SCCG_E_NOMEM"] and sneed == need, f"{c.name}: one byte short gives {src}, size {sneed} (want {need})"
    assert bool((d_o[need - 1:] == 0xAA).all().item()), f"{c.name}: a call that failed wrote past its capacity"
    frc, fneed = env.reconstruct_device(c, d_rec, d_o.data_ptr(), need)      # the exact capacity
    torch.cuda.synchronize()
    got = d_o.cpu().numpy().tobytes()
    assert frc == 0 and fneed == need and got[:need] == fa, f"{c.name}: the device form differs"
    assert got[need:] == b"\xaa" * 64, f"{c.name}: the device form wrote past the output"
    return rc, fa, outcome


def check_readers(env: Env, c, rc: int, fa, with_windows: bool = True):
    """sccg_reader_open and _open_shared: reconstruct's status; on success length, header, the whole
    sequence, windows at the targeted edges, SCCG_FETCH_UPPER and an index fetch."""
    hdr, truth = fetchlib.split_fasta(fa) if fa is not None else (None, None)
    for how, opener in (("open", lambda: env.ctx.open_reader(c.record, c.ref_fa)),
                        ("open_shared", lambda: env.shared_ref(c.ref_fa).open_reader(c.record))):
        rrc, rd = status_of(opener)
        assert rrc == rc, f"{c.name}: {how} returns {rrc}, reconstruct {rc}"
        if rd is None:
            continue
        with rd:
            L = rd.length
            assert L == len(truth), f"{c.name}: {how} length {L}, want {len(truth)}"
            assert rd.header == hdr, f"{c.name}: {how} header {rd.header!r}"
            assert rd.fetch([(0, L)]) == [truth], f"{c.name}: {how} whole fetch differs"
            assert rd.fetch([(0, L)], upper=True) == [truth.upper()], f"{c.name}: {how} upper fetch differs"
            if L:
                assert rd.fetch_encoded([(0, L)], encoding="index") == fetchlib.encode(truth, "index"), f"{c.name}: {how} index"
            if with_windows and how == "open" and L:
                regions = windows(recgen.probe_positions(c.record, L), L)
                got = rd.fetch(regions)
                if got != [truth[b:e] for b, e in regions]:
                    k = next(k for k, (b, e) in enumerate(regions) if got[k] != truth[b:e])
                    raise AssertionError(f"{c.name}: window {regions[k]} gives {got[k]!r}, want {truth[regions[k][0]:regions[k][1]]!r}")


def check_case(env: Env, c, frozen=None, with_windows: bool = True) -> str:
    _, want_fa = oracle(c)
    rc, fa, outcome = check_reconstruct(env, c, want_fa, frozen)
    check_readers(env, c, rc, fa, with_windows)
    return outcome
