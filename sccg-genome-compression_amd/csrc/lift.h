// lift.h -- launchers of lift.hip (reference intervals onto a sample, run-length coded), driven by
// sccg_api.cpp.
#pragma once
#include "locate.h"

// One lift call over nreg >= 1 validated intervals of the reference: interval i is [d_beg[i], d_end[i])
// of R as src sees it, or as d_tab[d_samp[i]] does when src is null; every source has enabled locating.
// The shape is segments.h's SgCall, mirrored onto the reference axis: the scratch is the caller's,
// lf_scratch_words(nreg) int64 at d_scratch; lf_count queues the first four launches and leaves the
// number of blocks at *lf_total_slot (device); lf_write queues the last two, straight behind them or
// after the caller has read the total: blk[d_off[i], d_off[i + 1]) = the blocks of interval i, d_off[0]
// = 0, d_off[nreg] = the total (d_off null: the offsets stay in the scratch); d_blk holds cap blocks,
// nothing beyond them is written, and a total beyond cap (the caller reads it) leaves the buffers
// unspecified.  Six launches per call whatever nreg, the interval sizes and the samples touched are,
// all under the profiler's fetch family; no host wait in either.  The locate index is read as it is.
struct LfCall {
    const LcSrc* src;
    const LcSrc* d_tab;
    const int64_t* d_beg;
    const int64_t* d_end;
    const int32_t* d_samp;
    int64_t nreg;
    int64_t bound_items;   // >= the sources' elementary intervals + nreg (sizes the grid, not the work)
    int64_t* d_scratch;
};
int64_t lf_scratch_words(int64_t nreg);
const int64_t* lf_total_slot(const LfCall& c);
int lf_count(const LfCall& c, hipStream_t s);
int lf_write(const LfCall& c, int64_t cap, int64_t* d_off, sccg_lift_block* d_blk, hipStream_t s);
