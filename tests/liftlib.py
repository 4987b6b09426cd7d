"""The truth of the lift call (sccg_*_lift), never the code under test: a numpy run-length coding of
locatelib's per-position inverse by the definition in sccg.h, and two truths that need no oracle -- the
blocks expanded back per reference base are what the GPU's own locate of the same positions returns, and
the origin fetch of a block's sequence stretch returns the block's reference positions.  Every check also
asserts the shape of an answer: the blocks tile each interval and no two neighbours could merge."""
import numpy as np

import originlib
import segmentslib
from segmentslib import every_pair, random_regions   # noqa: F401  (the interval lists are the segments tests')


def blocks(pos: np.ndarray, b: int, e: int) -> np.ndarray:
    """The blocks of reference interval [b, e) as rows (ref, len, pos): maximal runs of sequence positions
    ascending by one, of -1, of -2.  (The same coding as segmentslib.rle, on the other axis.)"""
    return segmentslib.rle(pos, b, e)


def want(pos_of, items):
    """(off, blk) of a batch: items (begin, end) with pos_of one array, or (sample, begin, end) with a list."""
    return segmentslib.want(pos_of, items)


def expand(blk: np.ndarray) -> np.ndarray:
    """The per-base locate answers that block rows spell, concatenated."""
    return segmentslib.expand(blk)


def check_shape(off, blk, bounds, what=""):
    """Layout, tiling, ascending ref, len > 0, pos >= -2, no two neighbours mergeable."""
    segmentslib.check_shape(off, blk, bounds, what)


def check_oracle(got, exp, items, what=""):
    segmentslib.check_oracle(got, exp, items, what)


def check_free(rd, intervals, off, blk, what=""):
    """The oracle-free truths of one reader's intervals, on the GPU's own outputs."""
    if not len(blk):
        return
    q = np.concatenate([np.arange(b, e, dtype=np.int64) for b, e in intervals])
    assert np.array_equal(expand(blk), rd.locate(q)[0]), f"{what}: the blocks do not expand to locate's answers"
    hit = blk[blk[:, 2] >= 0]
    if len(hit):
        org = originlib.fetch(rd, [(int(p), int(p + l)) for _, l, p in hit.tolist()]).astype(np.int64)
        ln = hit[:, 1]
        ref = np.repeat(hit[:, 0], ln) + np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
        assert np.array_equal(org, ref), f"{what}: the origin fetch of a block is not its reference stretch"


def check(rd, pos, intervals, what="", free=True):
    """One reader call against the oracle and the oracle-free truths; returns (off, blk)."""
    intervals = [(int(b), int(e)) for b, e in intervals]
    got = rd.lift(intervals)
    check_shape(got[0], got[1], intervals, what)
    check_oracle(got, want(pos, intervals), intervals, what)
    if free:
        check_free(rd, intervals, got[0], got[1], what)
    return got


def check_cohort(co, poss, items, readers=None, what=""):
    items = [(int(s), int(b), int(e)) for s, b, e in items]
    got = co.lift(items)
    check_shape(got[0], got[1], [(b, e) for _, b, e in items], what)
    check_oracle(got, want(poss, items), items, what)
    if readers is not None:
        off, blk = got
        for s in sorted({s for s, _, _ in items}):
            idx = [k for k, it in enumerate(items) if it[0] == s]
            sel = np.concatenate([blk[off[k]:off[k + 1]] for k in idx]) if idx else blk[:0]
            check_free(readers[s], [items[k][1:] for k in idx], None, sel, f"{what} sample {s}")
    return got


def cli_lines(pos, regions1):
    """`fetch --lift`'s output for 1-based inclusive regions of the reference, from the oracle's blocks."""
    out = []
    for b1, e1 in regions1:
        out.append(">%d-%d" % (b1, e1))
        for ref, ln, p in blocks(pos, b1 - 1, e1).tolist():
            tail = "%d\t%d" % (p + 1, p + ln) if p >= 0 else "-" if p == -1 else "N"
            out.append("%d\t%d\t%s" % (ref + 1, ref + ln, tail))
    return out
