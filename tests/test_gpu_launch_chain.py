"""GPU: the fused links of a pair's launch chain, byte for byte against the oracle.

The strip's scan is one launch whose last block scans the block totals, and the write pass composes
the tile offsets itself; k_cand_stats merges its own partials; k_commit sorts the frozen list and
k_round_close re-speculates in their last blocks; the first k-mer is read beside the reference strip.
Every one of them hands work to "the block that arrives last" through a ticket that must be zero
again afterwards.  So: FASTA lengths around the scan block (1024 tiles of 4 KiB), a carried line
status across a scan block, a round end over several blocks, the unusual first steps, and contexts
reused and run side by side.
"""
import json
import os
import subprocess
import sys
import threading

import pytest

from pkg import sccg  # (puts the package directory on sys.path first)
import oraclelib
import synthlib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 4096          # strip tile: FASTA bytes
SCAN_B = 1024        # tiles per scan block
# FASTA byte lengths -> 1, 1023, 1024, 1025 and 2050 tiles
LENGTHS = {"t1": 3000, "t1023": 1023 * TILE - 7, "t1024": 1024 * TILE, "t1025": 1024 * TILE + 1, "t2050": 2049 * TILE + 1234}

_cache: dict = {}


def _base():
    """one hg pair of 8.6 Mb (50 bases per line); the other pairs are cut from it (the target is a
    mutated copy of the reference, so equal cuts still align)"""
    if "base" not in _cache:
        _cache["base"] = synthlib.synth_pair("hg", 8_600_000, 8_600_000, 801)
    return _cache["base"]


def _cut(fa: bytes, n: int, first_line: int = 0) -> bytes:
    """a FASTA of exactly n bytes that ends with a full line: the header (padded to make up the
    length) and whole sequence lines from `first_line` on"""
    h = fa.index(b"\n")
    w = fa.index(b"\n", h + 1) - h   # line width with its line feed
    k = (n - h - 1) // w
    pad = n - h - 1 - k * w
    out = fa[:h] + b"x" * pad + b"\n" + fa[h + 1 + first_line * w: h + 1 + (first_line + k) * w]
    assert len(out) == n and out.endswith(b"\n") and not out.endswith(b"\n\n")
    return out


def _with_ref_headers(rfa: bytes) -> bytes:
    """extra '>' lines in the reference: one early, one that starts in tile 1023 and ends in tile 1024
    (the line status carried into tile 1024 crosses a scan block), one late"""
    out = rfa
    for at, width in ((10 * TILE, 30), (SCAN_B * TILE - 20, 200), (2040 * TILE, 50)):
        p = out.rfind(b"\n", 0, at) + 1
        out = out[:p] + b">" + b"x" * width + b"\n" + out[p:]
    return out


def _pair(name: str) -> tuple[bytes, bytes]:
    if name not in _cache:
        rfa, tfa = _base()
        if name == "t1":   # (from 200 kb in: the pair opens with a long run of N)
            pair = (_cut(rfa, LENGTHS[name], 4000), _cut(tfa, LENGTHS[name], 4000))
        elif name in LENGTHS:
            pair = (_cut(rfa, LENGTHS[name]), _cut(tfa, LENGTHS[name]))
        elif name == "refhdr":
            r2 = _with_ref_headers(_cut(rfa, LENGTHS["t2050"] - 32 - 202 - 52))
            # the middle line: starts in tile 1023, its line feed is in tile 1024
            s = r2.find(b">" + b"x" * 200)
            assert s // TILE == SCAN_B - 1 and (s + 201) // TILE == SCAN_B, (s, s // TILE)
            pair = (r2, _cut(tfa, LENGTHS["t2050"]))
        elif name == "crlf":   # (about 1024.5 tiles once every line feed is two bytes)
            n = 4_115_650
            pair = (_cut(rfa, n).replace(b"\n", b"\r\n"), _cut(tfa, n).replace(b"\n", b"\r\n"))
        else:
            raise KeyError(name)
        want = {"t1": 1, "t1023": 1023, "t1024": 1024, "t1025": 1025, "crlf": 1025}.get(name, 2050)
        for fa in pair:
            assert (len(fa) + TILE - 1) // TILE == want, (name, len(fa))
        _cache[name] = pair
    return _cache[name]


def _oracle(name: str) -> bytes:
    key = "rec:" + name
    if key not in _cache:
        _cache[key] = oraclelib.compress(*_pair(name))
    return _cache[key]


@pytest.fixture(scope="module")
def ctx():
    c = sccg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_exact():
    c = sccg.Context(0)
    c.exact_switch(True)   # the in-order local pass: the strips write both copies
    yield c
    c.close()


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", ["t1", "t1023", "t1024", "t1025", "t2050", "refhdr", "crlf"])
def test_scan_block_edges(ctx, ctx_exact, name, exact):
    rfa, tfa = _pair(name)
    c = ctx_exact if exact else ctx
    rec = c.compress(rfa, tfa)
    assert rec == _oracle(name)
    # (the reference writes line feeds: a CRLF target comes back as the oracle's reconstruction)
    want = tfa if name != "crlf" else _cache.setdefault("fa:crlf", oraclelib.decompress(_oracle(name), rfa))
    assert c.reconstruct(rec, rfa) == want


# ---- the round's end over several blocks -----------------------------------------------------
ROUND_PAIRS = (("hg", 1_500_000, 811), ("t2t", 1_500_000, 812))


@pytest.fixture(scope="module")
def round_refs(tmp_path_factory):
    """the oracle's walks (whole target, and from a state a fifth of the way into it: more than 512
    chunks are left), once for both runs"""
    out = {}
    for prof, n, seed in ROUND_PAIRS:
        rfa, tfa = synthlib.synth_pair(prof, n, n, seed)
        R, T = oraclelib.global_sequences(rfa, tfa)
        full = oraclelib.walk_range(R, T, 14, 100, 0, -1, len(T))
        t, p, l = [m for m in full[0] if m[0] + m[2] <= len(T) // 5][-1]
        mid = oraclelib.walk_range(R, T, 14, 100, t + l, p + l - 1, len(T))
        out[prof] = {"full": full, "state": [t + l, p + l - 1], "mid": mid}
    path = tmp_path_factory.mktemp("launch_chain") / "round_refs.json"
    path.write_text(json.dumps(out))
    return str(path)


_ROUND_CHILD = """
import json, sys
sys.path.insert(0, {here!r})
import synthlib, oraclelib
from pkg import sccg
refs = json.load(open({refs!r}))
c = sccg.Context(0)
out = []
for prof, n, seed in {pairs!r}:
    rfa, tfa = synthlib.synth_pair(prof, n, n, seed)
    R, T = oraclelib.global_sequences(rfa, tfa)
    x0, p0 = refs[prof]["state"]
    for what, a in (("full", (0, -1)), ("mid", (x0, p0))):
        runs = []
        for rep in range(3):
            got = json.loads(json.dumps(c.walk_range(R, T, 14, 100, a[0], a[1], len(T))))
            st = c.stats()
            runs.append((got == refs[prof][what], st["walk_rounds"], st["walk_chunks"], got))
        out.append(dict(prof=prof, what=what, exact=[r[0] for r in runs], rounds=[r[1] for r in runs],
                        chunks=[r[2] for r in runs], same=all(r[3] == runs[0][3] for r in runs)))
print(json.dumps(out))
"""


def _round_runs(refs: str, shift, det: bool):
    """2 Ki chunks: > 512 chunks, so the round-end grid (256 chunks per block) and k_commit have
    several blocks and their tails run in whichever arrives last; with a quarter-size anchor table
    (SCCG_ANCHOR_SHIFT=-2) most first guesses are wrong and the rounds carry, freeze and
    re-speculate.  A child process: the knobs are read once per process.  Three repeats of the walk
    over the whole target and from the mid-state, for an hg and a T2T-like pair of 1.5 Mb."""
    code = _ROUND_CHILD.format(here=HERE, refs=refs, pairs=ROUND_PAIRS)
    env = dict(os.environ, SCCG_WALK_CHUNK="2048")
    if shift:
        env["SCCG_ANCHOR_SHIFT"] = shift
    if det:
        env["SCCG_ANCHOR_DET"] = "1"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res) == 4
    for e in res:
        print(e)
        assert all(e["exact"]), e
        assert all(ch > 512 for ch in e["chunks"]), e
        assert e["same"], e
    return res


@pytest.mark.parametrize("shift", [None, "-2"])
def test_round_end_over_several_blocks(round_refs, shift):
    _round_runs(round_refs, shift, False)


@pytest.mark.parametrize("shift", [None, "-2"])
def test_round_end_rounds_repeat(round_refs, shift):
    """The three repeats of each call take the same number of rounds.

    With SCCG_ANCHOR_DET=1, as tests/test_gpu_parity.py::test_walk_rounds_deterministic sets it: by
    default the anchor table's slots are plain stores (the last writer wins), so the chunks' first
    guesses and with them the number of rounds change from call to call while the matches stay
    exact.  Measured without it on one MI355X, walk_rounds of three repeats with 2 Ki chunks: hg
    whole target 678 / 675 / 685 on the tree before the round end was fused and 618 / 608 / 618,
    668 / 691 / 676 after it; T2T-like from the mid-state 235 / 194 / 279 and 498 / 285 / 518."""
    for e in _round_runs(round_refs, shift, True):
        assert len(set(e["rounds"])) == 1, e


# ---- the first step's chain ------------------------------------------------------------------
def _first_step_pairs():
    if "first" not in _cache:
        rfa, tfa = synthlib.synth_pair("hg", 200_000, 200_500, 821)
        R, _ = oraclelib.global_sequences(rfa, tfa)
        hdr, body = tfa.split(b"\n", 1)
        absent = next(k for k in (bytes(b"ACGT"[(i >> (2 * j)) & 3] for j in range(14)) for i in range(977, 1 << 28, 7919))
                      if k not in R)
        tail = R[1000:1036]   # (36 bases: the inserted line is 50 wide like the others)
        _cache["first"] = {
            "leading_n": (rfa, hdr + b"\n" + (b"N" * 50 + b"\n") * 370 + body),          # 18 500 N: > 16 KiB
            "absent_kmer": (rfa, hdr + b"\n" + absent + tail + b"\n" + body),
            "iupac_kmer": (rfa, hdr + b"\n" + R[500:505] + b"R" + R[506:550] + b"\n" + body),
        }
    return _cache["first"]


@pytest.mark.parametrize("case", ["leading_n", "absent_kmer", "iupac_kmer"])
def test_first_step_chain(ctx, case):
    rfa, tfa = _first_step_pairs()[case]
    assert ctx.compress(rfa, tfa) == oraclelib.compress(rfa, tfa)


# ---- the tickets reset themselves ------------------------------------------------------------
def test_counters_reset_between_calls(ctx):
    big, small = _pair("t2050"), _pair("t1")
    first = ctx.compress(*big)
    assert ctx.compress(*small) == _oracle("t1")
    third = ctx.compress(*big)
    assert first == third == _oracle("t2050")


def test_two_contexts_side_by_side():
    """two contexts in two threads, as the bench's lanes: each result is its single-threaded record"""
    jobs = [["t2050", "t1", "t1023"], ["t1025", "t1024", "refhdr"]]
    with sccg.Context(0) as c:
        single = {n: c.compress(*_pair(n)) for names in jobs for n in names}
    for n, rec in single.items():
        assert rec == _oracle(n), n
    got: list = [None, None]
    errs: list = []
    go = threading.Barrier(2)

    def lane(i):
        try:
            with sccg.Context(0) as c:
                go.wait(timeout=30)
                got[i] = [c.compress(*_pair(n)) for n in jobs[i]]
        except Exception as e:   # noqa: BLE001  (reported by the main thread)
            errs.append(e)

    ts = [threading.Thread(target=lane, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i, names in enumerate(jobs):
        assert got[i] == [single[n] for n in names], names
