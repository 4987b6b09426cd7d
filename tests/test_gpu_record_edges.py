"""The record decoder at the edges of its grammar (GPU): hand-built records (tests/recgen.py) through
sccg_reconstruct, sccg_reconstruct_device (size query, one byte short, exact capacity),
sccg_reader_open and sccg_reader_open_shared, against the oracle and the three classes:

  exact      status and bytes equal the oracle's
  reject_ok  the oracle's exact bytes or SCCG_E_PARSE, nothing else
  error      FORMAT / PARSE / RANGE, the named class where the record holds one fault; with two
             faults PARSE, whatever their order in the file

All entry points agree with the rule and with each other.  The expected bytes come from the live
oracle and are checked against the compiled reference's frozen answers
(tests/golden/records.json.gz).  Every comparison is byte or status equality.

Family g (a run line of more than 32 MiB, which takes the scan-based run-line parser) uses the
oracle alone.  Family a runs once more under SCCG_DC_SPEC=0 and under SCCG_STRIP_KC=0
SCCG_DC_RUNS_FIRST=0, each in a child process (the knobs are read once per process).
"""
import json
import os
import subprocess
import sys
import time

import pytest

import fetchlib
import goldens
import oraclelib
import recedge
import recgen

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu

CASES = recgen.cases()
SWEEP = [c for c in CASES if c.name.startswith("a_off")]
GROUPS = {f"a_off{lo:04d}_{min(lo + 99, len(SWEEP) - 1):04d}": SWEEP[lo:lo + 100] for lo in range(0, len(SWEEP), 100)}
GROUPS["a_special"] = [c for c in CASES if c.family == "a" and not c.name.startswith("a_off")]
for _f in "bcdef":
    GROUPS[_f] = [c for c in CASES if c.family == _f]
assert sum(len(v) for v in GROUPS.values()) == len(CASES)


@pytest.fixture(scope="module")
def env():
    e = recedge.Env(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def frozen():
    return goldens.record_cases()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_record_edges(env, frozen, group, capsys):
    outcomes = {}
    for c in GROUPS[group]:
        outcomes[c.name] = recedge.check_case(env, c, frozen[c.name])
    with capsys.disabled():   # the accept / reject line, on record
        for name, o in outcomes.items():
            if name[0] == "e":
                print(f"\n  reject_ok {name}: {o}", end="")


def test_reject_line_is_the_documented_one(env):
    """The class rule lets a `reject_ok` record decode to the oracle's bytes.  The grammar as written
    down (recgen's docstring) places every record of family e outside it, so each is
    SCCG_E_PARSE today: a change of the accept / reject line changes this test and that paragraph
    together, on purpose."""
    for c in GROUPS["e"]:
        rc, _ = recedge.status_of(lambda: env.ctx.reconstruct(c.record, c.ref_fa))
        assert rc == recedge.E["SCCG_E_PARSE"], f"{c.name}: status {rc}"


def test_long_run_line(env):
    """Family g: a run line just over 32 MiB takes the scan-based parser (k_run_items_flag,
    k_run_items_parse, k_run_finish), once as the lowercase line and once as the N line."""
    t0 = time.time()
    ref, rec_lower, rec_n = recgen.long_line_case()
    for what, rec in (("lowercase line", rec_lower), ("N line", rec_n)):
        _, lower, nline, _ = recgen.lines_of(rec)
        assert max(len(lower), len(nline)) > 64 * 1024 * 512, what
        want = oraclelib.decompress(rec, ref)
        got = env.ctx.reconstruct(rec, ref)
        assert got == want, f"long {what}: reconstruction differs from the oracle's"
        hdr, truth = fetchlib.split_fasta(want)
        with env.ctx.open_reader(rec, ref) as rd:
            assert rd.length == len(truth) and rd.header == hdr, what
            assert rd.fetch([(0, len(truth))]) == [truth], what
            L = len(truth)
            regions = [(b, b + 3) for b in list(range(0, 200)) + list(range(L // 2 - 100, L // 2 + 100)) + list(range(L - 203, L - 3))]
            assert rd.fetch(regions) == [truth[b:e] for b, e in regions], what
    print(f"long run line: {time.time() - t0:.1f} s")


CHILD = r"""
import json, sys
sys.path.insert(0, HERE)
import recedge, recgen
env = recedge.Env(0)
bad = []
n = 0
for c in recgen.cases():
    if c.family != "a":
        continue
    n += 1
    try:
        _, want = recedge.oracle(c)
        recedge.check_reconstruct(env, c, want)
    except AssertionError as e:
        bad.append(str(e)[:200])
env.close()
print(json.dumps({"n": n, "bad": bad[:20], "nbad": len(bad)}))
"""


@pytest.mark.parametrize("knobs", [{"SCCG_DC_SPEC": "0"}, {"SCCG_STRIP_KC": "0", "SCCG_DC_RUNS_FIRST": "0"}],
                         ids=["fill_after_readback", "round5_strip_and_order"])
def test_family_a_under_knobs(knobs):
    env = dict(os.environ)
    for k in ("SCCG_DC_SPEC", "SCCG_STRIP_KC", "SCCG_DC_RUNS_FIRST"):
        env.pop(k, None)
    env.update(knobs)
    p = subprocess.run([sys.executable, "-c", f"HERE = {HERE!r}\n" + CHILD], env=env, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["n"] == len([c for c in CASES if c.family == "a"]) and d["nbad"] == 0, d
