// locate.h -- launchers of locate.hip (reference position -> sequence position), driven by sccg_api.cpp.
#pragma once
#include "decomp.h"

// The locate index of one reader (sccg_reader_enable_locate), in a device allocation of the reader's
// own.  Token i is the i-th token of nonzero length in record order; it copies R' positions
// [tp[i], tp[i] + l) to decoded offsets [to[i], to[i] + l).  ep holds every token start and end once,
// ascending: elementary interval k is [ep[k], ep[k + 1]) (the last one, from ep[ne - 1] on, is
// covered by nothing).  cover[k] is the number of tokens that cover it.  tree is an implicit segment
// tree over the elementary intervals, leaf k at node ne + k, node x's parent x >> 1, node 0 unused:
// every token has left its index, by minimum, on the O(log ne) canonical nodes of its leaves, so the
// first token in record order covering leaf k is the minimum over k's ancestors.
struct LcIndex {
    const uint32_t* tp;
    const int64_t* to;
    const uint32_t* ep;
    const int32_t* cover;
    const uint32_t* tree;
    int64_t nt, ne;
};
// What a locate query reads: the index, the target's N runs (decoded offset -> sequence position) and
// the runs of 'N' in R that R' has erased (rm.n == 0: R' is R).  A cohort's locate table holds one
// per sample; nt < 0 there marks a sample that had not enabled locating at create.
struct LcSrc {
    LcIndex ix;
    DcRuns nr, rm;
};

// ---- the build: three phases, a host read of a count between them (nt, then ne) ----
// 1. d_cnt[b] = tokens of nonzero length starting in record block b (S's 64-byte blocks), d_off their
//    exclusive prefix, *d_nt their number.  d_partial: scan_partials_needed(blocks).
int lc_count_tokens(const DcFetchSrc& S, int64_t* d_cnt, int64_t* d_off, int64_t* d_nt, int64_t* d_partial, hipStream_t s);
// 2. the nt tokens in record order (tp, tl, to), their 2 nt starts and ends sorted into `sorted` (keys:
//    2 nt scratch; tmp: lc_sort_temp_bytes(2 nt)), flag[k] = sorted[k] opens a new value and rank its
//    exclusive prefix (2 nt entries each), *d_ne = the distinct values.
size_t lc_sort_temp_bytes(int64_t nkeys);
int lc_endpoints(const DcFetchSrc& S, const int64_t* d_off, int64_t nt, uint32_t* tp, int32_t* tl, int64_t* to, uint32_t* keys,
                 uint32_t* sorted, void* tmp, size_t tmp_bytes, int64_t* flag, int64_t* rank, int64_t* d_ne, int64_t* d_partial,
                 hipStream_t s);
// 3. ep, cover and tree (ne, 2 ne entries: the reader's own memory) from the sorted endpoints; delta and
//    excl: ne scratch entries each (they may be phase 2's flag and rank).
int lc_index(const uint32_t* tp, const int32_t* tl, int64_t nt, const uint32_t* sorted, const int64_t* rank, int64_t ne,
             uint32_t* ep, int32_t* cover, uint32_t* tree, int64_t* delta, int64_t* excl, int64_t* d_partial, hipStream_t s);

// One locate call: d_pos[i] (and d_copies[i], when given) for reference positions d_q[i], i < n, each
// inside [0, |R|) of its source -- src, or d_tab[d_samp[i]] when src is null.  One launch whatever n
// and the samples touched are, bracketed under the profiler's fetch family (the family table is
// closed: "fetch" is its last entry).
struct LcLocate {
    const LcSrc* src;
    const LcSrc* d_tab;
    const int64_t* d_q;
    const int32_t* d_samp;
    int64_t n;
    int64_t* d_pos;
    int32_t* d_copies;
};
int lc_locate(const LcLocate& c, hipStream_t s);
