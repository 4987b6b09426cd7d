"""GPU: the chunked walk on directed scenarios (walklib), record for record against the oracle.

The walk cuts the target into chunks and speculates; the rounds re-walk, carry, freeze, chain and
re-speculate until the result is the sequential walk of compression.cpp:64-161.  Each scenario puts
one kind of event -- a SNP, an indel, a jump across the gate's |c - P| <= m edge, a literal stretch
of a threshold length, a stuck stretch with its rescue, a tandem array, the pn2 == 0 fallback of
:134-138 -- at j*S + d beside a chunk edge, and a failure names the scenario, the first differing
record, its chunk and what was planted.

* the match seam at the default chunk, every family; the gate family also at m = 0 and m = 127;
* proof that the path ran: the walk's chunk count, and for the sentinel families the number of
  k_fullc launches against the oracle's fallback matches;
* the same scenarios regenerated for chunks of 1024 and 4096 bases and under a quarter-size anchor
  table, each in a child process (the knobs are read once per process);
* the sentinel families from mid-states through walk_range;
* insertion, tandem and the sentinel families through the record text and back;
* the edge and gate families at k = 21 against the oracle's parameterised walk.
"""
import json
import os
import subprocess
import sys
import time

import pytest

from pkg import sccg  # (puts the package directory on sys.path first)
import fuzzgen
import oraclelib
import walklib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
S0 = walklib.DEFAULT_CHUNK
FAMILIES = sorted(walklib.FAMILIES)
STARTUP_SECONDS = 120   # a child's imports, its context and the first call's code load


@pytest.fixture(scope="module")
def ctx():
    c = sccg.Context(0)
    yield c
    c.close()


def _report(what, results, t0):
    secs = [r["secs"] for r in results]
    print(f"{what}: {len(results)} scenarios, {time.perf_counter() - t0:.2f} s in all, ctx.match {sum(secs):.2f} s, "
          f"slowest {max(secs):.3f} s")


@pytest.mark.parametrize("name", FAMILIES)
def test_seam_parity(ctx, name):
    t0 = time.perf_counter()
    res = walklib.run_parity(ctx, oraclelib, [(name, v) for v in walklib.variants(name, S0)], S0)
    _report(name, res, t0)
    bad = walklib.parity_errors(res)
    assert not bad, "\n".join(bad)
    if name in walklib.SENTINEL:
        assert all(r["launches"] >= walklib.FULLC_LAUNCHES for r in res)


@pytest.mark.parametrize("m", [0, 127])
def test_gate_at_other_m(ctx, m):
    """m = 127: 2m + 1 = 255 window slots of the 256"""
    t0 = time.perf_counter()
    res = walklib.run_parity(ctx, oraclelib, [("gate", v) for v in walklib.gate_variants_m(m)], S0, m=m)
    _report(f"gate m={m}", res, t0)
    bad = walklib.parity_errors(res)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["edge", "gate"])
def test_k21(ctx, name):
    """k = 21: the keys are the first 15 bases, confirmed by extension; no reference output of its
    own, so against the oracle's parameterised walk (as tests/test_gpu_params.py)"""
    t0 = time.perf_counter()
    res = walklib.run_parity(ctx, oraclelib, [(name, v) for v in walklib.variants(name, S0)], S0, k=21)
    _report(f"{name} k=21", res, t0)
    bad = walklib.parity_errors(res)
    assert not bad, "\n".join(bad)


# ---- other chunk lengths, poor speculation: a fresh process per setting ----------------------
_CHILD = """
import json, sys
sys.path.insert(0, {here!r})
import walklib, oraclelib
from pkg import sccg
c = sccg.Context(0)
cases = [(n, tuple(v)) for n, v in json.loads({cases!r})]
print(json.dumps(walklib.run_parity(c, oraclelib, cases, {S})))
"""


def _child(cases, S, env_extra):
    """run_parity in a child process with the knobs of env_extra.  The time limit is the code's own
    worst case (walklib.worst_case_seconds: 4 * C + 16 rounds a target, one escalation per fallback
    match): a walk that does not terminate ends the child and fails the test."""
    code = _CHILD.format(here=HERE, cases=json.dumps([(n, list(v)) for n, v in cases]), S=S)
    limit = STARTUP_SECONDS + walklib.worst_case_seconds(cases, S)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env_extra), capture_output=True, text=True,
                       timeout=limit)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res) == len(cases)
    _report(f"child {env_extra} (limit {limit:.0f} s)", res, t0)
    return res


@pytest.mark.parametrize("S", walklib.SMALL_CHUNKS)
def test_small_chunks(S):
    """S = 1024: FROZEN_MIN spans four chunks, a stretch stuck for 8 chunks is about 8 kb, a 70-copy
    sentinel array crosses three chunk edges"""
    cases = [(name, v) for name in FAMILIES for v in walklib.variants(name, S)]
    res = _child(cases, S, {"SCCG_WALK_CHUNK": str(S)})
    bad = walklib.parity_errors(res)
    assert not bad, "\n".join(bad)
    assert {r["name"] for r in res} == set(FAMILIES)


def test_poor_speculation():
    """a quarter-size anchor table (SCCG_ANCHOR_SHIFT=-2): wrong first guesses push the escalations
    into carried and fix-up chunks"""
    cases = [("insertion", v) for v in walklib.variants("insertion", S0) if v[3]]
    cases += [(name, v) for name in ("stuck_rescued",) + walklib.SENTINEL for v in walklib.variants(name, S0)]
    res = _child(cases, S0, {"SCCG_ANCHOR_SHIFT": "-2"})
    bad = walklib.parity_errors(res)
    assert not bad, "\n".join(bad)


# ---- walk_range from mid-states ----------------------------------------------------------------
@pytest.mark.parametrize("name", walklib.SENTINEL)
def test_walk_range_from_mid_states(ctx, name):
    """enter the walk at the oracle's state just before the planted stretch and one chunk before it
    (inside the literal run, where P is the same); the matches and the exit state"""
    t0 = time.perf_counter()
    n = 0
    for v in walklib.variants(name, S0):
        R, T, log = walklib.scenario(name, S0, v)
        at = log[0]["t"]
        full, _ = oraclelib.walk_range(R, T, 14, 100, 0, -1, len(T))
        t, p, l = [x for x in full if x[0] + x[2] <= at][-1]
        states = {(t + l, p + l - 1), (max(t + l, at - S0), p + l - 1)}
        for x0, p0 in sorted(states):
            want = oraclelib.walk_range(R, T, 14, 100, x0, p0, len(T))
            assert want[0] == [x for x in full if x[0] >= x0], (name, v, x0, p0)
            got = ctx.walk_range(R, T, 14, 100, x0, p0, len(T))
            assert got[1] == want[1], (name, v, x0, p0, got[1], want[1])
            assert got[0] == want[0], f"{name} {v!r} from ({x0}, {p0}): " + walklib.first_diff(got[0], want[0], S0, log, 0)
            n += 1
    print(f"{name}: {n} range walks, {time.perf_counter() - t0:.2f} s")


# ---- the record text ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(walklib.text_variants(S0)))
def test_record_text(ctx, name):
    """k_chunk_text's short, medium and long gap paths, k_long_copy's 64 Ki pieces, and for
    sentinel_far a negative delta across the out-of-gate match: the record and its reconstruction"""
    t0 = time.perf_counter()
    vs = walklib.text_variants(S0)[name]
    for v in vs:
        R, T, log = walklib.scenario(name, S0, v)
        rfa, tfa = fuzzgen.to_fasta(R.decode(), ">r"), fuzzgen.to_fasta(T.decode(), ">t")
        want = oraclelib.compress_params(rfa, tfa, local=0)
        got = ctx.compress(rfa, tfa, local=0)
        st = ctx.stats()
        if got != want:
            i = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            pytest.fail(f"{name} {v!r}: record byte {i} of {len(got)} / {len(want)}: got {got[max(0, i - 40):i + 40]!r}, "
                        f"oracle {want[max(0, i - 40):i + 40]!r}; planted: {log}")
        assert st["mode_global"] == 1 and st["walk_chunks"] == -(-len(T) // S0) >= 3, (name, v, st)
        assert ctx.reconstruct(got, rfa) == oraclelib.decompress(want, rfa) == tfa, (name, v)
    print(f"{name}: {len(vs)} records, {time.perf_counter() - t0:.2f} s")
