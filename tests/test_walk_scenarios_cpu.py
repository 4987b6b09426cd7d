"""CPU: the walk scenarios of walklib keep reaching what they were written for.

For every pinned scenario, at the default chunk and at the small chunk lengths the GPU tests run
with: the guards hold on the oracle's records (a scenario that lost its fallback match, its stuck
stretch or its chunk edge to a chance hit is a failed test), the generator is deterministic, and
the oracle's walk from the start state gives the same matches as its match_sequences.
"""
import pytest

import oraclelib
import walklib

CHUNKS = (walklib.DEFAULT_CHUNK,) + walklib.SMALL_CHUNKS
FAMILIES = sorted(walklib.FAMILIES)


def _check(name, S, variant, m=walklib.M):
    R, T, log = walklib.scenario(name, S, variant)
    assert (R, T, log) == walklib.scenario(name, S, variant), (name, S, variant)
    recs = oraclelib.match(R, T, walklib.K, m, True)
    g = walklib.check_guards(name, S, variant, R, T, log, recs, m)
    walked, (ex, _) = oraclelib.walk_range(R, T, walklib.K, m, 0, -1, len(T))
    assert walked == [(t, p, l) for kind, p, l, t in recs if kind], (name, S, variant)
    assert ex >= len(T) - walklib.K + 1
    return g


@pytest.mark.parametrize("S", CHUNKS)
@pytest.mark.parametrize("name", FAMILIES)
def test_guards_hold(name, S):
    vs = walklib.variants(name, S)
    assert len(vs) == len(set(vs)) >= 8
    figures = [_check(name, S, v) for v in vs]
    # every family has SNP variants whose trajectories hold hundreds of matches
    assert any(walklib.expected_matches(name, S, v) for v in vs), name
    assert max(f["n_matches"] for f in figures) >= walklib.MIN_MATCHES


@pytest.mark.parametrize("m", [0, 127])
def test_gate_guards_at_other_m(m):
    for v in walklib.gate_variants_m(m):
        _check("gate", walklib.DEFAULT_CHUNK, v, m)


@pytest.mark.parametrize("S", CHUNKS)
def test_gate_edge_between_99_and_100(S):
    """the same placement with 99 and with 100 reference bases deleted: aligned, and stuck to the end"""
    by = {}
    for v in walklib.variants("gate", S):
        if v[0] == "del" and v[1] in (99, 100) and v[3] == 2:
            R, T, log = walklib.scenario("gate", S, v)
            by[v[1]] = walklib.measure(R, T, oraclelib.match(R, T, 14, 100, True), 14, 100, S)["longest_literal"], len(T) - log[0]["t"]
    assert by[99][0] < 64 and by[100][0] >= by[100][1] - 14, by


@pytest.mark.parametrize("S", CHUNKS)
def test_events_land_on_chunk_edges(S):
    """every offset of D8 is used on both sides of an edge, for several j >= 1, in each family"""
    for name in FAMILIES:
        seen = set()
        for v in walklib.variants(name, S):
            _, T, log = walklib.scenario(name, S, v)
            for e in log:
                t = e.get("middle", e["t"])
                d = (t + S // 2) % S - S // 2
                if d in walklib.D8 and (t - d) // S >= 1:
                    seen.add((d, (t - d) // S))
        assert {d for d, _ in seen} == set(walklib.D8), (name, sorted(seen))
        assert len({j for _, j in seen}) >= 2, (name, sorted(seen))


@pytest.mark.parametrize("S", CHUNKS)
def test_sentinel_counts(S):
    """the fallback of compression.cpp:134-138 is what the sentinel families reach: c sentinel hits
    and the first match, all picking p = 0, in sentinel_near; one out-of-gate match at
    the planted offset, to the planted b, in sentinel_far"""
    for v in walklib.variants("sentinel_near", S):
        R, T, log = walklib.scenario("sentinel_near", S, v)
        recs = oraclelib.match(R, T, 14, 100, True)
        g = walklib.measure(R, T, recs, 14, 100, S)
        assert g["sentinel_hits"] == log[0]["c"] + 1 and g["first_is_sentinel"], (v, g["sentinel_hits"])
        assert all(p == 0 for kind, p, l, t in recs if kind and t in g["sentinel_at"]), v
    for v in walklib.variants("sentinel_far", S):
        R, T, log = walklib.scenario("sentinel_far", S, v)
        recs = oraclelib.match(R, T, 14, 100, True)
        at = log[0]["out_of_gate_at"]
        hit = [(p, l) for kind, p, l, t in recs if kind and t == at]
        assert hit and hit[0][0] == log[0]["b"] and hit[0][1] >= 200, (v, hit, log)


def test_text_variants_are_scenarios():
    tv = walklib.text_variants(walklib.DEFAULT_CHUNK)
    assert sorted(tv) == ["insertion", "sentinel_far", "sentinel_near", "tandem"]
    for name, vs in tv.items():
        for v in vs:
            R, T, log = walklib.scenario(name, walklib.DEFAULT_CHUNK, v)
            recs = oraclelib.match(R, T, 14, 100, True)
            walklib.check_guards(name, walklib.DEFAULT_CHUNK, v, R, T, log, recs)
            if name == "insertion" and v[0] >= 65535:
                assert len(T) >= 200_000 and (log[0]["t"], v[0]) in [(t, l) for kind, p, l, t in recs if not kind]
    assert any(v[0] == 70 for v in tv["sentinel_near"])
