#!/usr/bin/env python3
"""Regenerate the golden fixtures from the REAL reference (oracle/_ref, built from
/root/reference by `make -C oracle ref`).  Run in the build container only:

    python tests/golden/make_golden.py [--force]     (--force: rewrite existing fixtures too)

Writes
  tests/golden/cases/<name>.json.gz   inputs + the reference's outputs and exit codes
  tests/golden/synth_manifest.json    sha256 of the reference's record text / reconstruction
                                      for larger generator seeds (the inputs are regenerated
                                      from tools/synth.c by the tests; only hashes are kept)
  tests/golden/records.json.gz        (--records: this file alone) the reference's decompression of
                                      every hand-built record of tests/recgen.py: exit status, sha256
                                      and length of its FASTA; the inputs too, but for the offset
                                      sweep, whose records the generator rebuilds (their sha256)
The reference binaries run with the stub 7z (oracle/stub7z) on PATH; stdout is discarded.
"""
from __future__ import annotations

import base64
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import bytegen  # noqa: E402
import fuzzgen  # noqa: E402
import recgen  # noqa: E402
import reflib  # noqa: E402
import synthlib  # noqa: E402

REF_BIN = os.path.join(REPO, "oracle", "_ref")
STUB = os.path.join(REPO, "oracle", "stub7z")

N_LOCAL = 24
N_GLOBAL = 12
N_PAREN = 16   # targets whose literals hold '(' ')' ',' (delta_encode's own token scan)
SYNTH_SEEDS = [  # (profile, ref_len, tgt_len, seed)
    ("hg", 300_000, 301_000, 1),
    ("hg", 2_000_000, 2_003_000, 2),
    ("local", 2_000_000, 2_000_000, 3),
    ("t2t", 1_000_000, 1_000_000, 4),
    ("hg", 8_000_000, 8_020_000, 21),
]


def run_reference(ref_fa: bytes, tgt_fa: bytes) -> dict:
    env = dict(os.environ, PATH=STUB + os.pathsep + os.environ.get("PATH", ""))
    with tempfile.TemporaryDirectory() as d:
        rp, tp = os.path.join(d, "ref.fa"), os.path.join(d, "tgt.fa")
        open(rp, "wb").write(ref_fa)
        open(tp, "wb").write(tgt_fa)
        out = os.path.join(d, "out")
        c = subprocess.run([os.path.join(REF_BIN, "compression"), rp, tp, out], env=env,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        rec_path = os.path.join(out, "compressed_genome.txt")
        rec = open(rec_path, "rb").read() if os.path.exists(rec_path) else None
        res = {"compress_rc": c.returncode, "record": rec, "decompress_rc": None, "fasta": None}
        if c.returncode == 0:
            dec = os.path.join(d, "dec")
            dc = subprocess.run([os.path.join(REF_BIN, "decompression"), rec_path + ".7z", rp, dec],
                                env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            res["decompress_rc"] = dc.returncode
            fp = os.path.join(dec, "reconstructed_genome.fa")
            if dc.returncode == 0 and os.path.exists(fp):
                res["fasta"] = open(fp, "rb").read()
        return res


def byte_cases() -> dict:
    """Arbitrary byte values and '>' line layouts (tests/bytegen.py): odd bytes shared by both sides in
    local and global mode, references with several '>' lines, targets whose header is not the first
    line, and single byte classes placed at every word / lane / tile offset."""
    cases = {}
    for i in range(2):
        cases[f"bytes_local_{i:02d}"] = bytegen.odd_pair(i, 6000, "local")
        cases[f"bytes_global_{i:02d}"] = bytegen.odd_pair(i, 9000, "global")
    ref, tgt = bytegen.odd_sequences(900, 14_000, "local")
    for case in ("many_records", "gt_at_tile", "gt_long_tile"):
        cases[f"refhdr_{case}"] = (bytegen.ref_layout(ref.tobytes(), case), bytegen.to_fasta(tgt, b">t", 70))
    for case in ("line69", "odd_bytes", "second_gt"):
        cases[f"tgthdr_{case}"] = (bytegen.to_fasta(ref, b">r", 70), bytegen.tgt_header_layout(tgt.tobytes(), case))
    for cls, side in (("tab", "tgt"), ("0xc1", "ref"), ("@", "tgt"), ("n", "tgt")):
        cases[f"placed_{bytegen.slug(cls)}_{side}"] = bytegen.placed(cls, side)
    return cases


def b64(x: bytes | None):
    return None if x is None else base64.b64encode(x).decode()


def record_goldens() -> None:
    """tests/golden/records.json.gz: the compiled reference on every recgen case it defines."""
    cases = recgen.cases()
    asked = [c for c in cases if not c.undefined]
    answers = dict(zip((c.name for c in asked), reflib.run_ref_decompress_many([(c.record, c.ref_fa) for c in asked])))
    ref_ids = {v: k for k, v in recgen.REFS.items()}
    doc = {"refs": {k: b64(v) for k, v in recgen.REFS.items()}, "cases": []}
    for c in cases:
        rc, fa = answers.get(c.name, (None, None))
        doc["cases"].append({"name": c.name, "klass": c.klass, "expect": c.expect, "undefined": c.undefined,
                             "ref": ref_ids[c.ref_fa], "record": None if c.name.startswith("a_off") else b64(c.record),
                             "record_sha256": hashlib.sha256(c.record).hexdigest(), "rc": rc,
                             "fasta_sha256": hashlib.sha256(fa).hexdigest() if fa is not None else None,
                             "fasta_len": len(fa) if fa is not None else None})
    path = os.path.join(HERE, "records.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(f"records.json.gz: {len(cases)} cases, {len(asked)} answered by the reference, {os.path.getsize(path)} bytes")


def main() -> None:
    if not os.path.exists(os.path.join(REF_BIN, "compression")):
        sys.exit("oracle/_ref not built: run `make -C oracle ref` (needs /root/reference)")
    if "--records" in sys.argv:
        return record_goldens()
    cases = {}
    for i in range(N_LOCAL):
        cases[f"local_{i:02d}"] = fuzzgen.local_case(i)
    for i in range(N_GLOBAL):
        cases[f"global_{i:02d}"] = fuzzgen.global_case(i)
    for i in range(N_PAREN):
        cases[f"paren_{i:02d}"] = fuzzgen.paren_case(i)
    cases.update(fuzzgen.quirk_cases())
    cases.update(byte_cases())
    outdir = os.path.join(HERE, "cases")
    os.makedirs(outdir, exist_ok=True)
    force = "--force" in sys.argv
    for name, (rfa, tfa) in sorted(cases.items()):
        if not force and os.path.exists(os.path.join(outdir, name + ".json.gz")):
            continue   # fixtures are deterministic; keep the committed files byte-stable
        res = run_reference(rfa, tfa)
        doc = {"name": name, "ref_fa": b64(rfa), "tgt_fa": b64(tfa),
               "compress_rc": res["compress_rc"], "record": b64(res["record"]),
               "decompress_rc": res["decompress_rc"], "fasta": b64(res["fasta"])}
        with gzip.open(os.path.join(outdir, name + ".json.gz"), "wt") as f:
            json.dump(doc, f)
        print(f"{name:32s} rc={res['compress_rc']}/{res['decompress_rc']} "
              f"rec={len(res['record'] or b'')}B")
    manifest = []
    for prof, rl, tl, seed in SYNTH_SEEDS:
        rfa, tfa = synthlib.synth_pair(prof, rl, tl, seed)
        res = run_reference(rfa, tfa)
        manifest.append({"profile": prof, "ref_len": rl, "tgt_len": tl, "seed": seed,
                         "ref_fa_sha256": hashlib.sha256(rfa).hexdigest(),
                         "tgt_fa_sha256": hashlib.sha256(tfa).hexdigest(),
                         "compress_rc": res["compress_rc"],
                         "record_sha256": hashlib.sha256(res["record"]).hexdigest(),
                         "record_len": len(res["record"]),
                         "fasta_sha256": hashlib.sha256(res["fasta"]).hexdigest() if res["fasta"] else None})
        print(manifest[-1])
    with open(os.path.join(HERE, "synth_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    record_goldens()


if __name__ == "__main__":
    main()
