// find.h -- launchers of the find kernels (decomp.hip, beside the fetch kernels whose span decode they
// share): where an IUPAC pattern occurs in the regions, on either strand; driven by sccg_api.cpp.
#pragma once
#include "decomp.h"

// One find call over nreg >= 1 validated regions.  Region i is [d_beg[i], d_beg[i] + len_i) of src, or of
// d_tab[d_samp[i]] when src is null, and owns fd_candidates(len_i, m) candidate starts; d_pre is the
// exclusive prefix of those (nreg + 1 entries, d_pre[nreg] = F, which may be 0).  fwd / rev: the m mask
// nibbles (bit 0 A, 1 C, 2 G, 3 T) of the pattern and of its reverse complement; they travel in the
// kernel arguments.  The scratch is the caller's, fd_scratch_words(F) int64 at d_scratch.
// fd_count queues two launches and leaves the number of hits at *fd_total_slot (device); fd_write queues
// the third, straight behind them or after the caller has read the total: hit[d_off[i], d_off[i + 1]) =
// the hits of region i in ascending pos, forward before reverse, d_off[0] = 0, d_off[nreg] = the total
// (d_off null: no offsets); d_hit holds cap hits, nothing beyond them is written, and a total beyond cap
// (the caller reads it) leaves the buffers unspecified.  Three launches per call whatever nreg, the region
// sizes and the samples touched are, all under the profiler's fetch family; no host wait in either.
struct FdCall {
    const DcFetchSrc* src;
    const DcCohortEntry* d_tab;
    const int64_t* d_pre;
    const int64_t* d_beg;
    const int32_t* d_samp;
    int64_t nreg, F;
    int m;
    uint8_t fwd[SCCG_FIND_MAX_PATTERN], rev[SCCG_FIND_MAX_PATTERN];
    bool want_fwd, want_rev;
    int64_t* d_scratch;
    int K;   // find with mismatches only: substitutions allowed, 0 <= K <= SCCG_FIND_MAX_MISMATCHES, K < m
};
int64_t fd_candidates(int64_t len, int m);
int64_t fd_scratch_words(int64_t F);
const int64_t* fd_total_slot(const FdCall& c);
int fd_count(const FdCall& c, hipStream_t s);
int fd_write(const FdCall& c, int64_t cap, int64_t* d_off, sccg_hit* d_hit, hipStream_t s);

// Find with mismatches: the same call, c.K set, the same three launches over the same flat space and the same
// total slot; a hit is a start within K substitutions on a strand, a row {pos, strand, mismatches}.  The
// scratch is fa_scratch_words(F) int64: Find's 34 a tile and 128 a tile of 4-bit distances.
int64_t fa_scratch_words(int64_t F);
int fa_count(const FdCall& c, hipStream_t s);
int fa_write(const FdCall& c, int64_t cap, int64_t* d_off, sccg_hit_mm* d_hit, hipStream_t s);
