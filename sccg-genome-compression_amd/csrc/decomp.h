// decomp.h -- launchers of decomp.hip (reconstruction), driven by sccg_api.cpp.
#pragma once
#include "internal.h"

struct DcRuns {
    int32_t* start;   // run starts (ascending, disjoint)
    int32_t* len;     // run lengths
    int64_t* cum;     // exclusive prefix of len
    int64_t n;        // runs
    int64_t total;    // sum of len
};

// every '\n' of the record text, unordered: d_buf[0] = their count, d_buf[1, 1 + DC_NL_CAP) the
// first DC_NL_CAP found (one pass; the caller sorts them, or uses dc_find_lines when there are more)
constexpr int DC_NL_CAP = 32;
// (d_err, if given, is zeroed in the same stream-ordered launch as the count)
int dc_newlines(const uint8_t* d_rec, int64_t n, int64_t* d_buf, hipStream_t s, int32_t* d_err = nullptr);
// positions of the first four '\n' of the record text (n when absent) -> d_nl[0..3]
int dc_find_lines(const uint8_t* d_rec, int64_t n, int64_t* d_nl, hipStream_t s);
// exclusive max-scan of parenthesis positions: d_lp[i] = last '(' or ')' strictly before i
// (negative when none)
int dc_last_paren(const uint8_t* d_s, int64_t n, int64_t* d_lp, int64_t* d_partial, hipStream_t s);
// parse a lowercase / N run line (decompression.cpp:126-207) into r (arrays pre-allocated with
// capacity dc_run_cap(n)); d_err bit0 set on text outside the grammar.  No host wait: d_count[0]
// = runs, d_count[1] = total run length stay on the device (the caller reads them into r->n /
// r->total); d_lp, d_flag, d_dlt hold >= max(n, dc_run_cap(n)) + 1 entries.
int64_t dc_run_cap(int64_t n);
int dc_parse_runs(const uint8_t* d_s, int64_t n, DcRuns* r, int64_t* d_lp, int64_t* d_flag, int64_t* d_dlt,
                  int64_t* d_partial, int32_t* d_err, int64_t* d_count, hipStream_t s);
// both run lines (line 0 -> r0 / d_count0, line 1 -> r1 / d_count1) in one launch set when both take
// the tiled parser (d_flag and d_dlt then hold their tile summaries), else one after the other
int dc_parse_runs2(const uint8_t* s0, int64_t n0, DcRuns* r0, int64_t* d_count0, const uint8_t* s1, int64_t n1, DcRuns* r1,
                   int64_t* d_count1, int64_t* d_lp, int64_t* d_flag, int64_t* d_dlt, int64_t* d_partial, int32_t* d_err,
                   hipStream_t s);
// d_err bit2: the last N run (count d_ncnt[0]) ends past the decoded length *d_D + N count d_ncnt[1]
int dc_n_check(const DcRuns& nr, const int64_t* d_ncnt, const int64_t* d_D, int32_t* d_err, hipStream_t s);
// record line, per 64-byte block: state at its first byte -> d_lp, output bytes -> d_contrib, token
// deltas -> d_dlt, and their exclusive prefixes (output offset, running p) -> d_off, d_dsum;
// *d_total = decoded length; d_err bit 0 on text outside the grammar
int dc_decode_prepare(const uint8_t* d_s, int64_t n, int64_t* d_lp, int64_t* d_contrib, int64_t* d_dlt, int64_t* d_off,
                      int64_t* d_dsum, int64_t* d_partial, int32_t* d_err, int64_t* d_total, hipStream_t s);
// literals and token copies into d_dec (capacity dcap), with the range check against *d_nref:
// d_err bit 1 for a token beyond the reference (known only after the fill)
int dc_decode_fill(const uint8_t* d_s, int64_t n, const int64_t* d_lp, const int64_t* d_off, const int64_t* d_dsum,
                   const uint8_t* d_R, uint8_t* d_dec, hipStream_t s, const int64_t* d_nref, int32_t* d_err,
                   int64_t dcap = INT64_MAX);
// that range check alone (the fill without writing): d_err bit 1
int dc_tok_range(const uint8_t* d_s, int64_t n, const int64_t* d_lp, const int64_t* d_off, const int64_t* d_dsum,
                 const int64_t* d_nref, int32_t* d_err, hipStream_t s);
// N insertion + lowercase + 50-column wrap of nres result bytes into d_out (no final '\n');
// d_index: scratch of dc_format_index_words(nres) int64 (the formatter's block index)
int64_t dc_format_index_words(int64_t nres);
// The formatter's block index into d_index (it needs the run lists, not the decoded bytes, so it
// can run beside the token fill, on another stream).
int dc_format_index(int64_t nres, const DcRuns& nr, const DcRuns& lr, int64_t* d_index, uint8_t* d_out, hipStream_t s);
// The formatter, over the index dc_format_index wrote for the same nres and d_out; the stream
// first waits for wait_before (the index's stream).
int dc_format(const uint8_t* d_dec, int64_t nres, const DcRuns& nr, const DcRuns& lr, const int64_t* d_index, uint8_t* d_out,
              hipStream_t s, hipEvent_t wait_before);

// What a region fetch reads (a reader's own copies, sccg_api.cpp): the record line and its 64-byte
// block index (state, decoded offset, running p: dc_decode_prepare's d_lp, d_off, d_dsum), R' and
// both run lists (cum: the N runs' only).  Byte buffers carry the usual readable slack.
// rm (the origin fetch alone): the runs of 'N' in the reference sequence R that R' has erased -- R'
// position v is R position v + (len of every run with start - cum <= v); rm.n == 0: R' is R.
struct DcFetchSrc {
    const uint8_t* rec;
    int64_t nrec;
    const int64_t* bin;
    const int64_t* boff;
    const int64_t* bdsum;
    const uint8_t* R;
    DcRuns nr, lr;
    DcRuns rm;
};
// A source as the fetch kernels take it: with what they would otherwise derive per launch (nn =
// S.nr.n, nlr = S.lr.n, ntot = the N bases of the sequence).  A cohort's device table
// (sccg_cohort_create) holds one per sample.
struct DcCohortEntry {
    DcFetchSrc S;
    int64_t nn, nlr, ntot;
};
// One fetch: d_out[0, bytes per base * F), base-major, the bases of regions [d_beg[i], d_beg[i] +
// d_pre[i + 1] - d_pre[i]), i < nreg, concatenated (d_pre: exclusive prefix of the lengths,
// d_pre[nreg] = F).  src given: all from that reader (d_tab, d_samp unused); src null: region i reads
// d_tab[d_samp[i]].  Region i is on the reverse strand (position end - 1 - q at output base q) when bit
// 63 of d_beg[i] is set or all_rev.  The format (enc: SCCG_ENC_*, dt: SCCG_DT_*, a valid pair):
//   ASCII / INDEX / ONEHOT  the sequence byte, its code, its one-hot elements (complemented when
//                           reversed); upper (no lowercase runs) matters for ASCII only
//   ORIGIN (I32)            the position in the reference sequence a token copied the base from (R'
//                           positions through S.rm; R' is not read), -1 for a literal, -2 inside one of
//                           the target's N runs; unchanged on the reverse strand
// (sccg_reader_fetch's bytes are ASCII with no region reversed.)  d_out is aligned to the element.
// Regions, samples and tokens were validated by the caller.
struct DcFetch {
    const DcFetchSrc* src;
    const DcCohortEntry* d_tab;
    const int64_t* d_pre;
    const int64_t* d_beg;
    const int32_t* d_samp;
    int64_t nreg, F;
    int enc, dt;
    bool upper, all_rev;
    void* d_out;
};
// One launch whatever nreg and the samples touched are, under the profiler's fetch family.
int dc_fetch(const DcFetch& c, hipStream_t s);

// The R' -> R map: the maximal runs of the byte 'N' in the stripped, original-case reference d_R[0, n)
// (n < 2^31, 16-byte aligned, 16 readable bytes behind it).  dc_refmap_count: d_nruns[0] = the runs
// (d_nruns[1] the same), d_os / d_oe the tiles' ranks for the write (d_cs, d_ce, d_os, d_oe: dc_refmap_tiles(n)
// entries each; d_partial: 2 * scan_partials_needed(tiles)).  dc_refmap_write: m's arrays (m->n runs, as
// counted) filled -- start, len, cum -- and *d_total = the N in all of them (d_partial:
// scan_partials_needed(m->n)).  No host wait in either.
int64_t dc_refmap_tiles(int64_t n);
int dc_refmap_count(const uint8_t* d_R, int64_t n, int64_t* d_cs, int64_t* d_ce, int64_t* d_os, int64_t* d_oe, int64_t* d_nruns,
                    int64_t* d_partial, hipStream_t s);
int dc_refmap_write(const uint8_t* d_R, int64_t n, const int64_t* d_os, const int64_t* d_oe, DcRuns* m, int64_t* d_total,
                    int64_t* d_partial, hipStream_t s);
