// segments.h -- launchers of segments.hip (a region's alignment to the reference, run-length coded),
// driven by sccg_api.cpp.
#pragma once
#include "decomp.h"

// One segments call over nreg >= 1 validated forward regions: region i is [d_beg[i], d_end[i]) of src,
// or of d_tab[d_samp[i]] when src is null; every source has reference coordinates.  The scratch is the
// caller's, sg_scratch_words(nreg) int64 at d_scratch.  sg_count queues the first four launches and
// leaves the number of segments at *sg_total_slot (device).  sg_write queues the last two, straight
// behind them or after the caller has read the total: seg[d_off[i], d_off[i + 1]) = the segments of
// region i, d_off[0] = 0, d_off[nreg] = the total (d_off null: the offsets stay in the scratch); d_seg
// holds cap segments, nothing beyond them is written, and a total beyond cap (the caller reads it)
// leaves the buffers unspecified.  Six launches per call whatever nreg, the region sizes and the
// samples touched are, all under the profiler's fetch family; no host wait in either.
struct SgCall {
    const DcFetchSrc* src;
    const DcCohortEntry* d_tab;
    const int64_t* d_beg;
    const int64_t* d_end;
    const int32_t* d_samp;
    int64_t nreg;
    int64_t bound_items;   // >= the regions' record blocks + nreg (sizes the grid, not the work)
    int64_t* d_scratch;
};
int64_t sg_scratch_words(int64_t nreg);
const int64_t* sg_total_slot(const SgCall& c);
int sg_count(const SgCall& c, hipStream_t s);
int sg_write(const SgCall& c, int64_t cap, int64_t* d_off, sccg_segment* d_seg, hipStream_t s);
// The calls' scan, one launch of one block under the fetch family: out[k] = in[0] + .. + in[k - 1], k <= m
// (lift.hip's flat work space is laid out by it too).
int sg_scan(const int64_t* in, int64_t* out, int64_t m, hipStream_t s);
