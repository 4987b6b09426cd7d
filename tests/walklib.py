"""Directed scenarios for the global walk (compression.cpp:64-161) and guards that say what each one
reaches -- pure CPU, test infrastructure only.

A scenario is a seeded, deterministic function of (name, S, variant): S is the walk's chunk length,
and every planted event lands at a target offset j*S + d next to a chunk edge.  It returns
(R, T, log): N-free uppercase bytes for the match seam and the planted events with their target
offsets (for failure messages and for the guards).

The guards are computed from the ORACLE's records alone (oraclelib.match), never from the code
under test: a scenario whose guard fails no longer reaches the path it was written for, and that
is a failed test.  Seeds come from the scenario's own name; RESEED pins another one for the few
scenarios that lose their event to a chance hit.

Families (see each generator): edge, gate, insertion, stuck_rescued, tandem, sentinel_near,
sentinel_far.
"""
from __future__ import annotations

import random
import zlib

K, M = 14, 100                       # the reference's k-mer length and gate (compression.cpp:373-379)
D8 = (-15, -14, -13, -1, 0, 1, 13, 14)   # event offsets from a chunk edge: around k and around 0
SNP_RATES = (0.0, 1 / 500, 1 / 60)
QUIET = 32                           # no background SNP this close to a planted event or a piece's end
MIN_MATCHES = 100                    # what a SNP variant's trajectory must hold ...
MIN_EXPECTED = 130                   # ... where its aligned bases times its rate promise this many
SMALL_CHUNKS = (1024, 4096)
DEFAULT_CHUNK = 16384                # walk_chunk()'s value for targets under ~130 Mb

# scenarios that need another seed than their name's: {(name, S, variant): salt}
RESEED: dict = {}

_ACGT = b"ACGT"


def _rng(name: str, S: int, variant) -> random.Random:
    salt = RESEED.get((name, S, variant), 0)
    return random.Random(zlib.crc32(f"{name}|{S}|{variant!r}|{salt}".encode()))


def _rand(rng: random.Random, n: int) -> bytearray:
    return bytearray(rng.choices(_ACGT, k=n))


def _other(rng: random.Random, *avoid: int) -> int:
    """a base that is none of `avoid`"""
    return rng.choice([c for c in _ACGT if c not in avoid])


def _len(S: int, spec) -> int:
    """a length given as a number or in chunks: "S-1", "S", "S+1", "3S+5", "8S+100" """
    if isinstance(spec, int):
        return spec
    a, _, b = spec.partition("S")
    return (int(a) if a else 1) * S + (int(b) if b else 0)


def rest_for(S: int) -> int:
    """aligned bases after a scenario's last event: three chunks, and enough for well over 100
    matches at the 1/60 SNP rate"""
    return max(3 * S, 8192)


def n_chunks_for(S: int) -> int:
    """target chunks of a plain scenario: a few at the default chunk, more at the small ones (so
    that a 1/60 SNP background still gives well over 100 matches)"""
    return 6 if S >= 8192 else 8 if S >= 4096 else 14


class _Build:
    """The target, piece by piece: aligned stretches of R (with background SNPs), skips in R,
    literal bytes; `r` is the reference cursor, `n` the target length so far."""

    def __init__(self, rng: random.Random, R: bytearray, snp: float, r0: int = 0):
        self.rng, self.R, self.snp = rng, R, snp
        self.parts: list[bytes] = []
        self.n, self.r = 0, r0
        self.log: list[dict] = []

    def put(self, b) -> None:
        self.parts.append(bytes(b))
        self.n += len(b)

    def aligned_to(self, t_off: int, quiet=()) -> None:
        """R[r:] up to target length t_off, SNPs at the background rate but none within QUIET of
        the piece's ends or of the target offsets in `quiet`"""
        n = t_off - self.n
        assert n >= 0 and self.r + n <= len(self.R), (t_off, self.n, self.r, len(self.R))
        seg = bytearray(self.R[self.r:self.r + n])
        if self.snp and n > 2 * QUIET:
            for i in self.rng.sample(range(QUIET, n - QUIET), int((n - 2 * QUIET) * self.snp)):
                if all(abs(self.n + i - q) >= QUIET for q in quiet):
                    seg[i] = _other(self.rng, seg[i])
        self.put(seg)
        self.r += n

    def aligned_n(self, n: int) -> None:
        self.aligned_to(self.n + n)

    def event(self, what: str, **kw) -> dict:
        e = dict(what=what, t=self.n, **kw)
        self.log.append(e)
        return e

    def insertion(self, ins: bytearray) -> None:
        """bytes that extend neither the match before them nor the one after: the literal is theirs"""
        if ins:
            if ins[0] == self.R[self.r]:
                ins[0] = _other(self.rng, ins[0])
            if ins[-1] == self.R[self.r - 1]:
                ins[-1] = _other(self.rng, ins[-1], self.R[self.r] if len(ins) == 1 else 0)
        self.put(ins)

    def jump(self, to: int) -> None:
        """the target goes on at R[to:]: the byte it goes on with is made to end the match before it
        (R is changed there, at a position the target has not used yet)"""
        i = max(to, self.r)           # the later of the two positions is still unused
        j = min(to, self.r)
        if self.R[i] == self.R[j]:
            self.R[i] = _other(self.rng, self.R[i])
        self.r = to

    def done(self):
        return bytes(self.R), b"".join(self.parts), self.log


# ---- families --------------------------------------------------------------------------------
def edge(S: int, variant):
    """scan_end / lastk edges: a SNP, a 1-20 base insertion, a 1-20 base deletion and an undisturbed
    match, each at its own chunk edge j*S + d (which event gets which edge rotates with idx), and a
    target that ends at nch*S + {0, 1, 13, 14, 15} with a SNP 14-16 bases before its end; odd idx: R
    ends where the target's last base aligns.  variant = (d, idx)"""
    d, idx = variant
    rng = _rng("edge", S, variant)
    nch = n_chunks_for(S)
    tail = (0, 1, 13, 14, 15)[idx % 5]
    ins_len = (1, 2, 5, 13, 14, 15, 19, 20)[idx % 8]
    del_len = (20, 19, 15, 14, 13, 7, 2, 1)[idx % 8]
    R = _rand(rng, nch * S + 600)
    b = _Build(rng, R, SNP_RATES[idx % 3], r0=37)
    kinds = ["snp", "ins", "del", "cross"]
    kinds = kinds[idx % 4:] + kinds[:idx % 4]
    edges = [j * S + d for j in range(1, 5)]
    for at, kind in zip(edges, kinds):
        b.aligned_to(at, quiet=edges)
        if kind == "snp":
            b.event("snp")
            b.put(bytes([_other(rng, R[b.r])]))
            b.r += 1
        elif kind == "ins":
            b.event("insertion", g=ins_len)
            b.insertion(_rand(rng, ins_len))
        elif kind == "del":
            b.event("deletion", bases=del_len)
            b.jump(b.r + del_len)
        else:
            b.event("undisturbed")
    # a SNP 16, 15 or 14 bases before the target's end: the last match starts at the last k-mer but
    # one (lastk - 1), at the last k-mer (lastk), or not at all (k - 1 literal bases)
    end = nch * S + tail
    snp_at = end - K - 2 + idx % 3
    b.aligned_to(snp_at, quiet=edges + [snp_at])
    b.event("end_snp", before_end=end - snp_at)
    b.put(bytes([_other(rng, R[b.r])]))
    b.r += 1
    b.aligned_to(end, quiet=[end - 1])       # (quiet: too short for a background SNP anyway)
    b.event("target_end", tail=tail)
    if idx % 2:
        del R[b.r:]
    return b.done()


def gate(S: int, variant):
    """The gate's |c - P| <= m edge: the target skips `size` reference bases (kind "del": the next
    candidate is size + 1 past P) or goes back by them (kind "back": size - 1 before P) at j*S + d
    and goes on aligned to its end -- within the gate the walk stays aligned; a deletion outside it
    is stuck to the target's end, a backward jump outside it comes back after size - 1 - m literals.
    variant = (kind, size, d, j, snp index)"""
    kind, size, d, j, si = variant
    rng = _rng("gate", S, variant)
    nch = n_chunks_for(S)
    R = _rand(rng, nch * S + 1000)
    b = _Build(rng, R, SNP_RATES[si], r0=37 + 200)
    b.aligned_to(j * S + d)
    b.event(kind, size=size)
    b.jump(b.r + size if kind == "del" else b.r - size)
    b.aligned_to(nch * S + 77)
    return b.done()


def gate_stuck(variant, m: int) -> bool:
    """whether the gate scenario is stuck to the target's end at this m: a deletion's candidate is
    size + 1 past P and moves away with every literal step; at m = 0 any SNP before the event does
    the same (the next aligned candidate is 2 past P)"""
    kind, size, si = variant[0], variant[1], variant[4]
    return (kind == "del" and size + 1 > m) or (m == 0 and SNP_RATES[si] > 0)


def gate_literal(variant, m: int) -> int:
    """the literal steps a backward jump costs: its candidate starts size - 1 before P and comes one
    nearer with every literal step, so it is back in the gate after size - 1 - m of them"""
    kind, size = variant[0], variant[1]
    return max(0, size - 1 - m) if kind == "back" else 0


def insertion(S: int, variant):
    """A literal stretch of a threshold length g at j*S + d between two aligned stretches: random
    bases, or (decoy) a copy of a distant stretch of R that the anchors vote onto a diagonal the
    sequential walk never takes.  variant = (g, d, j, decoy, snp index[, chunks after it])"""
    gs, d, j, decoy, si = variant[:5]
    rest = variant[5] * S if len(variant) > 5 else rest_for(S)
    g = _len(S, gs)
    rng = _rng("insertion", S, variant)
    at = j * S + d
    used = 37 + at + rest + 50            # reference bases the aligned stretches take
    R = _rand(rng, used + 500 + (g + 2000 if decoy else 0))
    b = _Build(rng, R, SNP_RATES[si], r0=37)
    b.aligned_to(at)
    b.event("decoy" if decoy else "insertion", g=g, literal=(at, g))
    if decoy:
        src = used + 1500
        b.insertion(bytearray(R[src:src + g]))
    else:
        b.insertion(_rand(rng, g))
    b.aligned_n(rest + 50)
    return b.done()


def stuck_rescued(S: int, variant):
    """A deletion of 500 > m reference bases freezes P; the target goes on aligned (so the chunks'
    anchors vote for a diagonal out of the gate) for g bases, then a copy of R[P-30 : P+300] brings
    the walk back and the target goes on from there.  The deletion (at "del") or the rescuing copy
    (at "rescue") lands at j*S + d, with j raised until the stuck stretch fits before it.
    variant = (g, d, j, at, snp index)"""
    gs, d, j, where, si = variant
    g = _len(S, gs)
    rng = _rng("stuck_rescued", S, variant)
    if where == "rescue":
        while j * S + d - g < 300:
            j += 1
    at = j * S + d - (g if where == "rescue" else 0)
    R = _rand(rng, 37 + at + 500 + g + rest_for(S) + 1000)
    b = _Build(rng, R, SNP_RATES[si], r0=37)
    b.aligned_to(at)
    P = b.r - 1
    b.event("deletion", bases=500, P=P, literal=(at, g))
    b.jump(b.r + 500)
    b.aligned_n(g)
    last = bytearray(b.parts[-1])
    if last[-1] == R[P - 31]:         # the stuck stretch's last base does not extend the copy backwards
        last[-1] = _other(rng, last[-1])
        b.parts[-1] = bytes(last)
    b.event("rescue", copy=(P - 30, P + 300))
    b.put(R[P - 30:P + 300])
    b.r = P + 300
    b.aligned_n(rest_for(S) - 300)
    return b.done()


def tandem_lead(S: int) -> int:
    """chunks before the array's own j at small S: the walk may leave the array stuck, so the matches
    a SNP variant needs come from the aligned stretch before it"""
    return max(0, 8192 // S - 1)


def tandem(S: int, variant):
    """The tie rules of compression.cpp:110-138 across a chunk edge: R holds an array of units of
    length u spanning more than 2m, the target has `delta` copies more or fewer with SNPs inside, and
    the target's array has its middle at j*S + d: many candidates of equal length in one window.
    variant = (u, delta, d, j, snp index)"""
    u, delta, d, j, si = variant
    rng = _rng("tandem", S, variant)
    j += tandem_lead(S)
    n = max(8, (2 * M + 60) // u + 1)
    tn = n + delta
    t0 = j * S + d - (tn * u) // 2
    unit = _rand(rng, u)
    a0 = 37 + t0
    R = _rand(rng, a0) + unit * n + _rand(rng, rest_for(S) + 500)
    b = _Build(rng, R, SNP_RATES[si], r0=37)
    b.aligned_to(t0)
    b.event("tandem", unit=u, ref_copies=n, tgt_copies=tn, middle=j * S + d)
    arr = bytearray(unit * tn)
    for i in rng.sample(range(len(arr)), max(1, len(arr) // 60)):
        arr[i] = _other(rng, arr[i])
    b.put(arr)
    b.r = a0 + n * u
    b.aligned_n(rest_for(S) + 50)
    return b.done()


_PLACE = {"edge1": "S", "edge2": "2S", "mid1": "S", "mid2": "2S", "deep": "8S"}


def _first_copy_at(S: int, place: str, d: int) -> int:
    """where a sentinel family's planted stretch starts: at a chunk edge (edge1, edge2), inside the
    chunk after it (mid1, mid2), or at least 8 chunks in (deep)"""
    return _len(S, _PLACE[place]) + (0 if place.startswith("edge") else S // 3) + d


def sentinel_near(S: int, variant):
    """Repeated escalations: T = R[:50] + random(g) + (R[:41] with its last base changed) * c +
    the aligned rest from R[41:].  P stays <= m, so at every copy the gated pick is p = 0 -- the
    reference's "none" -- and it takes the ungated pick (compression.cpp:134-138), which is p = 0
    again.  place "gap": see below.  variant = (c, place, d, snp index)"""
    c, place, d, si = variant
    rng = _rng("sentinel_near", S, variant)
    R = _rand(rng, 41 + rest_for(S) + 500)
    b = _Build(rng, R, SNP_RATES[si])
    copy = bytearray(R[:41])
    copy[40] = _other(rng, R[40])
    b.put(R[:50])
    if place == "gap":
        # c copies that end 60 bases before chunk 2 (chunk 1 ends with P = 39 after a short literal
        # run: resumed after its escalations, neither converged nor frozen), a literal chunk 2, and
        # one more copy at 3S + d, entered with that P after a whole literal chunk
        at1, at = 2 * S - 41 * c - 60, 3 * S + d
        b.put(_rand(rng, at1 - 50))
        b.put(copy * c)
        b.put(_rand(rng, at - b.n))
        b.event("sentinel_copies", c=c + 1, every=41, sentinel_at=[at1 + 41 * i for i in range(c)] + [at])
        b.put(copy)
    else:
        at = _first_copy_at(S, place, d)
        b.put(_rand(rng, at - 50))
        b.event("sentinel_copies", c=c, every=41, sentinel_at=[at + 41 * i for i in range(c)])
        b.put(copy * c)
    b.r = 41
    b.aligned_n(rest_for(S) + 50)
    return b.done()


def sentinel_far(S: int, variant):
    """k_fullc's search rather than its trivial answer: R[:14] is planted again at b in R's second
    half; T = R[:50] + random(g) + R[b:b+200] + the aligned rest.  The gated pick is p = 0 (length
    14), the ungated one is b (length >= 200): the next match is out of the gate.  double: the
    200 bases stand at two places in R and the target leaves both after them, so the ungated picks
    tie and the one nearer to P wins.  variant = (place, d, double, snp index)"""
    place, d, double, si = variant
    rng = _rng("sentinel_far", S, variant)
    at = _first_copy_at(S, place, d)
    rest = rest_for(S) + 50
    b1 = rest + 800
    b2 = b1 + 201 + rest + 600
    R = _rand(rng, (b2 + 600) if double else 2 * b1 - 200)
    R[b1:b1 + K] = R[:K]
    if R[b1 + K] == R[K]:             # the copy at 0 matches the planted stretch for exactly k bases
        R[b1 + K] = _other(rng, R[K])
    b = _Build(rng, R, SNP_RATES[si])
    if double:
        R[b2:b2 + 200] = R[b1:b1 + 200]
    b.put(R[:50])
    b.put(_rand(rng, at - 50))
    b.event("sentinel_far", b=b1, b_other=b2 if double else None, out_of_gate_at=at)
    b.put(R[b1:b1 + 200])
    b.r = b1 + 200
    if double:
        b.put(bytes([_other(rng, R[b1 + 200], R[b2 + 200])]))
        b.r += 1
    b.aligned_n(rest)
    return b.done()


FAMILIES = {"edge": edge, "gate": gate, "insertion": insertion, "stuck_rescued": stuck_rescued,
            "tandem": tandem, "sentinel_near": sentinel_near, "sentinel_far": sentinel_far}
SENTINEL = ("sentinel_near", "sentinel_far")


def scenario(name: str, S: int, variant):
    return FAMILIES[name](S, variant)


# ---- the pinned scenarios --------------------------------------------------------------------
G_LENGTHS = (13, 14, 15, 31, 32, 33, 100, 101, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
             "S-1", "S", "S+1", "3S+5")
GATE_SIZES = (98, 99, 100, 101, 102)
GATE_SIZES_127 = (126, 127, 128, 129)      # the same edge at m = 127 (2m + 1 = 255 window slots)
UNITS = (1, 2, 3, 7, 14, 15, 50, 99, 100, 101, 171)
TEXT_G = (31, 32, 33, 4095, 4096, 4097)
TEXT_G_LONG = (65535, 65536, 65537)        # k_long_copy's 64 Ki pieces: targets of > 200 kb


def variants(name: str, S: int) -> list:
    """the pinned variants of a family at chunk length S (the same at every S, except the ones the
    small chunks add: a stretch stuck for 8 chunks, a first copy 8 chunks in)"""
    small = S < DEFAULT_CHUNK
    out: list = []
    if name == "edge":
        out = [(d, i + 8 * r) for r in range(2) for i, d in enumerate(D8)]
    elif name == "gate":
        for ki, kind in enumerate(("del", "back")):
            for i, size in enumerate(GATE_SIZES):
                n = 5 * ki + i
                out.append((kind, size, D8[n % 8], 2, (n + 2) % 3))
                out.append((kind, size, D8[(n + 3) % 8], 3, n % 3))
    elif name == "insertion":
        for i, g in enumerate(G_LENGTHS):
            out.append((g, D8[i % 8], 1 + i % 3, False, (i + 2) % 3))
            if _len(S, g) >= 31:
                out.append((g, D8[(i + 5) % 8], 1 + (i + 1) % 3, True, i % 3))
    elif name == "stuck_rescued":
        for i, g in enumerate(G_LENGTHS + (("8S+100",) if small else ())):
            out.append((g, D8[(i + 1) % 8], 1 + i % 2, "del", (i + 2) % 3))
        for i, g in enumerate((1024, 4096, "S")):
            out.append((g, D8[(3 * i + 2) % 8], 2, "rescue", (i + 2) % 3))
    elif name == "tandem":
        for i, u in enumerate(UNITS):
            out.append((u, 3, D8[i % 8], 1 + i % 2, (i + 2) % 3))
            out.append((u, -3, D8[(i + 4) % 8], 2 - i % 2, i % 3))
    elif name == "sentinel_near":
        places = [("edge1", d) for d in D8] + [("edge2", -14), ("edge2", 0), ("mid1", 0), ("mid2", 5)]
        if small:
            places.append(("deep", 7))
        for i, (pl, d) in enumerate(places):
            for c in (1, 4, 70):
                if c == 70 and pl == "edge1" and d not in (-1, 0):
                    continue
                out.append((c, pl, d, (i + c) % 3))
        out += [(4, "gap", 0, 2), (4, "gap", 13, 0), (1, "gap", 1, 1), (4, "gap", -14, 1)]
    elif name == "sentinel_far":
        places = [("edge1", d) for d in D8] + [("edge2", -1), ("edge2", 0), ("mid1", 0), ("mid2", 5)]
        if small:
            places.append(("deep", 7))
        for i, (pl, d) in enumerate(places):
            out.append((pl, d, False, (i + 2) % 3))
            if i % 3 == 0:
                out.append((pl, d, True, i % 3))
    else:
        raise KeyError(name)
    return out


def gate_variants_m(m: int) -> list:
    """the gate family's subset run at m = 0 and m = 127 (with the same edge moved to m = 127)"""
    sub = [v for v in variants("gate", DEFAULT_CHUNK) if v[3] == 2]
    if m == 127:
        for i, size in enumerate(GATE_SIZES_127):
            sub.append(("del", size, D8[i % 8], 2, (i + 2) % 3))
            sub.append(("back", size, D8[(i + 4) % 8], 3, i % 3))
    return sub


def text_variants(S: int) -> dict:
    """the scenarios that go through the record text, by family"""
    ins = [(g, D8[i % 8], 1, False, (i + 2) % 3) for i, g in enumerate(TEXT_G)]
    ins += [(g, D8[(i + 3) % 8], 1, False, 2, 8) for i, g in enumerate(TEXT_G_LONG)]
    near, far = variants("sentinel_near", S), variants("sentinel_far", S)
    near = [v for v in near if v[0] == 70][:2] + [v for v in near if v[0] != 70][::4][:6]
    return {"insertion": ins, "sentinel_near": near, "sentinel_far": far[::2][:8],
            "tandem": variants("tandem", S)}


# ---- guards ----------------------------------------------------------------------------------
def measure(R: bytes, T: bytes, recs, k: int, m: int, S: int) -> dict:
    """What the oracle's records [(kind, p, l, t)] say the walk met.
    sentinel_hits: matches whose k-mer is R[:k], taken while the previous P <= m (first_is_sentinel:
    the walk's first match is one of them -- its P is -1); out_of_gate: the target offsets of
    matches after the first with |p - P_prev| > m."""
    P = -1
    first = True
    hits, first_hit, oog, lits, nm = [], False, [], [], 0
    head = R[:k]
    for kind, p, l, t in recs:
        if not kind:
            lits.append((t, l))
            continue
        nm += 1
        if P <= m and T[t:t + k] == head:
            hits.append(t)
            first_hit = first_hit or first
        if not first and abs(p - P) > m:
            oog.append(t)
        P = p + l - 1
        first = False
    return dict(sentinel_hits=len(hits), sentinel_at=hits, first_is_sentinel=first_hit, out_of_gate=oog,
                longest_literal=max((l for _, l in lits), default=0), literals=lits, n_matches=nm,
                n_chunks=-(-len(T) // S))


def expected_matches(name: str, S: int, variant, m: int = M) -> bool:
    """whether this scenario must hold MIN_MATCHES matches: a SNP variant whose aligned stretches
    promise them (a gate scenario that is stuck aligns only up to its event)"""
    if name == "edge":
        rate = SNP_RATES[variant[1] % 3]
    else:   # (the sentinel families' variants have four fields, the others five or six)
        rate = SNP_RATES[variant[3 if name in SENTINEL else 4]]
    if name == "gate":
        aligned = (variant[3] * S) if gate_stuck(variant, m) else n_chunks_for(S) * S
        if m == 0 and rate:
            return False          # every SNP leaves a gate of 0: stuck from the first one on
    elif name == "edge":
        aligned = n_chunks_for(S) * S
    elif name == "tandem":
        aligned = (variant[3] + tandem_lead(S)) * S - 300
    else:
        aligned = rest_for(S) - 300
    return aligned * rate >= MIN_EXPECTED


def check_guards(name: str, S: int, variant, R: bytes, T: bytes, log, recs, m: int = M, k: int = K) -> dict:
    """assert what the family needs of the oracle's records; returns measure()'s figures"""
    g = measure(R, T, recs, k, m, S)
    tag = f"{name} S={S} {variant!r} m={m}: "
    brief = {x: g[x] for x in ("sentinel_hits", "out_of_gate", "longest_literal", "n_matches", "n_chunks")}
    assert g["n_chunks"] >= 3, tag + f"{brief}"
    assert not (set(T) | set(R)) - set(_ACGT), tag + "bases other than ACGT"
    if expected_matches(name, S, variant, m):
        assert g["n_matches"] >= MIN_MATCHES, tag + f"{brief}"
    ev = {e["what"]: e for e in log}
    if name == "sentinel_near":
        e = ev["sentinel_copies"]
        assert g["sentinel_hits"] >= e["c"], tag + f"{brief}"
        assert set(e["sentinel_at"]) <= set(g["sentinel_at"]), tag + f"planted {e['sentinel_at'][:3]}.., taken {g['sentinel_at'][:5]}.."
    elif name == "sentinel_far":
        e = ev["sentinel_far"]
        assert e["out_of_gate_at"] in g["out_of_gate"], tag + f"{brief} planted at {e['out_of_gate_at']}"
        assert e["out_of_gate_at"] in g["sentinel_at"], tag + f"{brief}"
    elif name == "edge" and k == K:
        be, last = ev["end_snp"]["before_end"], tuple(recs[-1])
        want = (0, 0, k, len(T) - k) if be == k else (1, last[1], be - 1, len(T) - be + 1)
        assert last == want, tag + f"last record {last}, planted a SNP {be} before the end"
    elif name == "gate":
        e = log[0]
        if gate_stuck(variant, m):
            # (to the target's end but for a chance hit in the window: one stuck stretch in about
            # twenty meets one, tens of kilobases in)
            assert g["longest_literal"] >= min(len(T) - e["t"] - k, max(S, 4096)), tag + f"{brief} event at {e['t']} of {len(T)}"
        else:
            n = gate_literal(variant, m)
            assert g["longest_literal"] < max(64, n + 17), tag + f"{brief}"
            assert n < 16 or [x for x in g["literals"] if abs(x[0] - e["t"]) <= 16 and abs(x[1] - n) <= 16], tag + f"{brief}"
    elif name in ("insertion", "stuck_rescued"):
        e = log[0]
        at, n = e["literal"]
        near = [(t, l) for t, l in g["literals"] if abs(t - at) <= 16 and abs(l - n) <= 16]
        assert near, tag + f"no literal of {n} at {at}: {[x for x in g['literals'] if abs(x[0] - at) < 64]}"
    return g


def first_diff(got, want, S: int, log, t_index: int = 3) -> str:
    """the first differing record of two record lists ((kind, p, l, t), or (t, p, l) with t_index 0),
    its chunk and its distance to a chunk edge"""
    i = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    a = got[i] if i < len(got) else None
    b = want[i] if i < len(want) else None
    if a is None and b is None:
        return "the records are equal"
    t = (b or a)[t_index]
    edge_d = min(t % S, S - t % S)
    return (f"record {i} of {len(got)} / {len(want)}: got {a}, oracle {b}; target offset {t} = chunk {t // S}, "
            f"{edge_d} from a chunk edge; planted: {log}")


# ---- the seam against the oracle, for a list of scenarios ------------------------------------
FULLC_LAUNCHES = 2        # run_fullc (walk.hip): two k_fullc launches for one resolution of the fallback
ROUND_SECONDS = 0.05      # allowance per walk round: a handful of launches and at most four readbacks
ESCALATION_SECONDS = 0.05  # and per escalation: one run_fullc, seven small writes, one resumed walk


def worst_case_seconds(cases, S: int) -> float:
    """An upper bound for walking `cases` [(name, variant)], from the code's own limit: run_rounds
    gives up (SCCG_E_INTERNAL) after 4 * C + 16 rounds of a C-chunk target, and every fallback match
    costs one escalation; each at a hundred times what it takes on an MI355X."""
    total = 0.0
    for name, v in cases:
        _, T, log = scenario(name, S, v)
        C = -(-len(T) // S)
        esc = sum(e.get("c", 1) for e in log if e["what"].startswith("sentinel"))
        total += (4 * C + 16) * ROUND_SECONDS + (esc + 1) * ESCALATION_SECONDS + 0.5
    return total


def run_parity(ctx, oracle, cases, S: int, m: int = M, k: int = K, guards: bool = True) -> list:
    """ctx.match against oracle.match for every (name, variant) of `cases` at chunk length S (the
    context must walk with that chunk).  One dict per case: ok, the first differing record with its
    chunk (diff), the chunks the walk had, and for the sentinel families the k_fullc launches seen
    and the least the oracle's fallback matches imply (the walk's first match, P = -1, is found by
    the first step's sweep and is no escalation)."""
    import time
    out = []
    for name, v in cases:
        R, T, log = scenario(name, S, v)
        want = oracle.match(R, T, k, m, True)
        g = check_guards(name, S, v, R, T, log, want, m) if guards and k == K else measure(R, T, want, k, m, S)
        sentinel = name in SENTINEL
        if sentinel:
            ctx.profile(True, families=["fullc_scan"])
        t0 = time.perf_counter()
        got = ctx.match(R, T, k, m, True)
        secs = time.perf_counter() - t0
        launches = None
        if sentinel:
            launches = ctx.profile_get().get("fullc_scan", (0.0, 0))[1]
            ctx.profile(False)
        ok = got == want
        out.append(dict(name=name, variant=list(v), ok=ok, diff=None if ok else first_diff(got, want, S, log),
                        chunks=ctx.stats()["walk_chunks"], want_chunks=g["n_chunks"], launches=launches,
                        need_launches=FULLC_LAUNCHES * (g["sentinel_hits"] - int(g["first_is_sentinel"])) if sentinel else None,
                        sentinel_hits=g["sentinel_hits"], secs=round(secs, 4)))
    return out


def parity_errors(results) -> list:
    """what is wrong in run_parity's results, as messages"""
    bad = []
    for r in results:
        tag = f"{r['name']} {tuple(r['variant'])!r}: "
        if not r["ok"]:
            bad.append(tag + r["diff"])
        if r["chunks"] < 3 or r["chunks"] != r["want_chunks"]:
            bad.append(tag + f"walked {r['chunks']} chunks, the target has {r['want_chunks']}")
        if r["launches"] is not None and (r["launches"] < r["need_launches"] or r["launches"] < r["sentinel_hits"] or not r["launches"]):
            bad.append(tag + f"{r['launches']} k_fullc launches for {r['sentinel_hits']} fallback matches of the oracle "
                             f"(at least {r['need_launches']})")
    return bad
