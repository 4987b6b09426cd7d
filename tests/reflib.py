"""The compiled reference's decompression (oracle/_ref, built where the reference sources exist)."""
from __future__ import annotations

import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(REPO, "oracle", "_ref")
HAVE_REF = os.path.exists(os.path.join(REF_BIN, "decompression"))


def run_ref_decompress(rec: bytes, rfa: bytes):
    """decompression <arc> <ref> <out> with the stub 7z (which copies the archive to out/<stem>):
    (exit status, reconstructed_genome.fa or None)."""
    env = dict(os.environ, PATH=os.path.join(REPO, "oracle", "stub7z") + os.pathsep + os.environ["PATH"])
    with tempfile.TemporaryDirectory() as d:
        ap, rp = os.path.join(d, "compressed_genome.txt.7z"), os.path.join(d, "r.fa")
        open(ap, "wb").write(rec)
        open(rp, "wb").write(rfa)
        p = subprocess.run([os.path.join(REF_BIN, "decompression"), ap, rp, os.path.join(d, "o")], env=env,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
        if p.returncode:
            return p.returncode, None
        return 0, open(os.path.join(d, "o", "reconstructed_genome.fa"), "rb").read()


def run_ref_decompress_many(pairs, workers: int = 8):
    """run_ref_decompress over [(record, reference FASTA)], a few processes at a time, in order."""
    with ThreadPoolExecutor(workers) as ex:
        return list(ex.map(lambda p: run_ref_decompress(*p), pairs))
