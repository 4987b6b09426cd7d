"""The environment variables the native code reads are exactly the ones DESIGN.md §7 lists, and every
variable a test sets is one of them (a knob nothing documents or nothing reads is dead code)."""
import pathlib
import re

REPO = pathlib.Path(__file__).resolve().parent.parent
PKG = REPO / "sccg-genome-compression_amd"
NAME = r"SCCG_[A-Z0-9_]+"


def _read_by_code():
    names = set()
    for d in ("csrc", "cli"):
        for f in sorted((PKG / d).iterdir()):
            if f.suffix in (".hip", ".cpp", ".h"):
                names |= set(re.findall(r'(?:getenv|env_int)\(\s*"(%s)"' % NAME, f.read_text()))
    return names


def _listed_in_design():
    text = (REPO / "DESIGN.md").read_text()
    m = re.search(r"^\* Environment variables the native code reads.*?(?=^\* )", text, re.S | re.M)
    assert m, "DESIGN.md §7 lost its 'Environment variables the native code reads' paragraph"
    return set(re.findall(NAME, m.group(0)))


def _set_by_tests():
    pats = (r'[(,]\s*(%s)=' % NAME, r'["\'](%s)["\']\s*:' % NAME, r'setenv\(\s*["\'](%s)["\']' % NAME)
    names = set()
    for f in sorted((REPO / "tests").rglob("*.py")):
        if f.name != pathlib.Path(__file__).name:
            for p in pats:
                names |= set(re.findall(p, f.read_text()))
    return names


def test_knobs_read_are_the_knobs_documented():
    code, doc = _read_by_code(), _listed_in_design()
    assert code, "found no getenv / env_int call: the scan is broken"
    assert code == doc, f"read but not listed: {sorted(code - doc)}; listed but not read: {sorted(doc - code)}"


def test_knobs_set_by_tests_exist():
    code, tests = _read_by_code(), _set_by_tests()
    assert {"SCCG_ANCHOR_SHIFT", "SCCG_TEST_OOM", "SCCG_DC_SPEC"} <= tests, "the scan of tests/ is broken"
    assert tests <= code, f"set by a test, read by nothing: {sorted(tests - code)}"
