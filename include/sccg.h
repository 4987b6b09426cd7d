/*
 * sccg.h -- C ABI of the MI355X-native SCCG hot path (libsccg.so).
 *
 * The reference (Jan-Celin/SCCG-genome-compression) has no library or FFI: its drop-in boundary
 * is the two command lines plus the record-file format.  This header is the
 * seam a host program binds to; the repository's `compression` / `decompression` executables are
 * thin CLIs over it with the reference's argv, output paths, 7z calls and exit codes.
 *
 * Entry point                         replaces (reference file:line)
 * ----------------------------------  -------------------------------------------------------------
 * sccg_compress / _device             compress_genome up to the 7z call  compression.cpp:320-580
 * sccg_compress_files                 the same from FASTA files to the   compression.cpp:181-220,
 *                                     record file                         :320-331
 *   (_ex: with parameter overrides      of its constants                   compression.cpp:373-379)
 *                                     (read_genomes_from_files :181-220, lowercase/N run lines
 *                                     :341-368/:495-555, local loop :372-481, global pass
 *                                     :484-574, delta_encode :222-304)
 * sccg_match                          match_sequences                    compression.cpp:36-179
 * sccg_walk_range / _device           its global walk from a state        compression.cpp:64-161
 *                                     (one chromosome split across GPUs)
 * sccg_reconstruct / _device          decompress_genome after 7z +       decompression.cpp:43-114,
 *                                     reconstruct_genome + file body     :117-279, :316-323
 * sccg_reader_open / _device          reconstruct_genome's parse, kept    decompression.cpp:117-236
 * sccg_reader_fetch / _device         ranges of its `result`             decompression.cpp:241-262
 *   (sccg_reader_close, _length,        (no counterpart: the reference rebuilds the whole file)
 *    _header)
 * sccg_reader_fetch_encoded / _device  the same ranges as base indices or one-hot elements, either
 *   (sccg_fetch_bytes_per_base)         strand (no counterpart)
 * sccg_reference_open / _device       the reference strip alone, kept     decompression.cpp:105-110
 *   (sccg_reference_close,              and shared: sccg_reader_open without the strip and without a
 *    _device_bytes, sccg_reader_open_   private R' (no counterpart: the reference strips per run)
 *    shared / _device, sccg_reader_
 *    device_bytes)
 * sccg_cohort_create / _fetch /       the encoded fetch over many records of one context, each region
 *   _fetch_device (sccg_cohort_close,   naming its record, in one launch (no counterpart)
 *    _samples)
 * sccg_reader_segments / _device,     a region's alignment to the reference, run-length coded: the gapless
 *   sccg_cohort_segments / _device      blocks, literals and N runs the origin fetch spells out per base
 *                                       (no counterpart)
 * sccg_reader_lift / _device,         intervals of the reference onto a sample, run-length coded: what
 *   sccg_cohort_lift / _device          locate spells out per reference base (no counterpart)
 * sccg_reader_find / _device,         where an IUPAC pattern occurs in regions of a sample, either strand
 *   sccg_cohort_find / _device          (no counterpart)
 *   (sccg_find_pattern_masks)
 * sccg_reader_find_approx / _device,  the same within k substitutions, each hit with its mismatch count
 *   sccg_cohort_find_approx / _device   (no counterpart)
 *
 * Conventions: status ints (0 = OK); the library never calls exit(); host buffers it returns are
 * malloc'ed and released with sccg_buf_free.  One context per GPU; a context is not re-entrant;
 * contexts on different GPUs may be driven from different host threads.  Every compute path runs
 * on the GPU -- there is no CPU fallback; without a usable device sccg_ctx_create fails.
 */
#ifndef SCCG_H
#define SCCG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCCG_OK             0
#define SCCG_E_INVALID      1  /* bad argument */
#define SCCG_E_HIP          2  /* HIP runtime error (message in sccg_last_error) */
#define SCCG_E_NOMEM        3  /* device or host allocation failed */
#define SCCG_E_DELTA_STOI   4  /* delta_encode's stoi would throw (compression.cpp:279): the
                                  reference then leaves the un-delta'd text and exits 1; the text
                                  returned is that un-delta'd text */
#define SCCG_E_FORMAT       5  /* record file misses a line (decompression.cpp:68-97) */
#define SCCG_E_RANGE        6  /* token beyond the reference (decompression.cpp:223-229) */
#define SCCG_E_PARSE        7  /* malformed run line / token (decompression.cpp:309-311): text outside
                                  the decoder's grammar -- integers of an optional sign and at most
                                  10 digits within int32; run lines of "(d,l)" and bare "d" items
                                  between ',', starts >= 0, ascending and disjoint, N runs within
                                  the sequence; every record-line byte outside a "(d,l)" token a
                                  literal.  Text std::stoi would still read (blanks, trailing junk,
                                  more digits) and unsorted lowercase runs are reported here too,
                                  never decoded to other bytes.  Reported before SCCG_E_RANGE
                                  whatever the order of the faults in the file */
#define SCCG_E_UNSUPPORTED  8  /* shape outside what sccg_match accepts (see below) */
#define SCCG_E_INTERNAL     9  /* internal consistency check failed */
#define SCCG_E_OPEN_REF    10  /* reference FASTA cannot be opened / read (compression.cpp:187-191) */
#define SCCG_E_OPEN_TGT    11  /* target FASTA cannot be opened / read (compression.cpp:202-206) */
#define SCCG_E_WRITE       12  /* the record file cannot be written (compression.cpp:329-331) */

typedef struct sccg_ctx sccg_ctx;

typedef struct {
    char* data;
    size_t len;
} sccg_buf;

/* match_sequences' vector<Position> as SoA (compression.cpp:20-24): kind 1 = match (pos
 * includes the offset, :153), kind 0 = literal run St[t, t+len). */
typedef struct {
    uint8_t* kind;
    int32_t* pos;
    int32_t* len;
    int64_t* t;
    int64_t n;
} sccg_records;

typedef struct {
    int mode_global;          /* 1 when the local loop switched (compression.cpp:462-473) */
    int64_t switch_segment;   /* last segment of a switch window (compression.cpp:417-473), -1 if it
                                 stayed local: the reference's switch segment (the first window)
                                 with SCCG_OPT_EXACT_SWITCH, otherwise the first window the mode
                                 probe found (>= it; the record file is the same either way) */
    int64_t target_bases;     /* |T| after whitespace strip (compression.cpp:218) */
    int64_t reference_bases;  /* |R| */
    int64_t n_matches;        /* (p,l) tokens on the record line */
    int64_t literal_bases;    /* literal bytes on the record line */
    int64_t walk_rounds;      /* global walk: speculative + fix-up rounds */
    int64_t walk_chunks;      /* global walk: chunks */
    int64_t record_bytes;     /* length of the whole compressed_genome.txt */
    int64_t walk_chains;      /* global walk: frozen chains resolved by the chain kernels */
    int64_t walk_reference_bases; /* |R'|: the reference with every 'N' erased (compression.cpp:556) */
} sccg_stats;

int sccg_ctx_create(int device, sccg_ctx** out);
void sccg_ctx_destroy(sccg_ctx* ctx);
const char* sccg_last_error(const sccg_ctx* ctx);
int sccg_last_stats(const sccg_ctx* ctx, sccg_stats* out);

/* Context options (sccg_ctx_set_option; SCCG_E_INVALID for an unknown option):
 *   SCCG_OPT_EXACT_SWITCH  0 (default): the local/global mode is decided from ANY switch window
 *                          (a few probed runs of segments first), which is enough for the record
 *                          file (compression.cpp:462-473 truncates it and the global pass
 *                          regenerates it); 1: the in-order pass finds the first window, so
 *                          sccg_stats.switch_segment is the reference's switch segment. */
#define SCCG_OPT_EXACT_SWITCH 1
int sccg_ctx_set_option(sccg_ctx* ctx, int option, int64_t value);

/* Whole-file compression up to (excluding) 7z: returns the exact bytes of
 * <out>/compressed_genome.txt for the given reference/target FASTA file contents. */
int sccg_compress(sccg_ctx* ctx, const char* ref_fa, size_t ref_len, const char* tgt_fa,
                  size_t tgt_len, sccg_buf* out_text);

/* Same, HBM-resident: inputs are device pointers, the text is written to d_out (capacity
 * out_cap bytes; sccg_compress_bound gives a safe capacity) and *out_len is set.  `stream` is a
 * hipStream_t (NULL = the context's own stream).  Synchronises before returning. */
int sccg_compress_device(sccg_ctx* ctx, const void* d_ref_fa, size_t ref_len, const void* d_tgt_fa,
                         size_t tgt_len, void* d_out, size_t out_cap, size_t* out_len, void* stream);
size_t sccg_compress_bound(size_t ref_len, size_t tgt_len);

/* compress_genome's algorithm parameters (compression.cpp:373-379, hard-coded there).
 * sccg_params_default() gives the reference's values, with which sccg_compress_ex is
 * sccg_compress.  Other values are NON-PARITY overrides: the reference cannot
 * run them, so their output is pinned against the parameterised CPU oracle only.  Accepted:
 *   local = 1 (start with the local segment controller, :378): k, k2, L, T1, T2 at the reference's
 *             values (the local kernels are built for them), 0 <= m <= 127;
 *   local = 0 (straight to the global pass, as the reference with `local = false`): 1 <= k <= 32,
 *             0 <= m <= 127 (k2, L, T1, T2 unused).
 * Others: SCCG_E_UNSUPPORTED. */
typedef struct {
    int32_t k;       /* 14   primary k-mer length: local pass 1 and the global walk */
    int32_t k2;      /* 10   local pass 2 */
    int32_t L;       /* 1000 segment length */
    int32_t m;       /* 100  global range gate |p - prev_match_end| <= m */
    float T1;        /* 0.5  segment mismatch-ratio threshold */
    int32_t T2;      /* 4    bad segments in a row before the switch to global */
    int32_t local;   /* 1    start with the local controller */
} sccg_params;

void sccg_params_default(sccg_params* p);
int sccg_compress_ex(sccg_ctx* ctx, const sccg_params* params, const char* ref_fa, size_t ref_len,
                     const char* tgt_fa, size_t tgt_len, sccg_buf* out_text);
int sccg_compress_device_ex(sccg_ctx* ctx, const sccg_params* params, const void* d_ref_fa,
                            size_t ref_len, const void* d_tgt_fa, size_t tgt_len, void* d_out,
                            size_t out_cap, size_t* out_len, void* stream);

/* Files in, record file out (compression.cpp:320-580 up to, excluding, the 7z call): reads both
 * FASTA files (host threads, pinned staging, the copies to HBM overlapped with the reading and the
 * reference's GPU work), compresses on the GPU and writes `out_path` (the bytes sccg_compress
 * returns).  params NULL = the reference's constants.  *out_len (optional) = bytes written.
 * SCCG_E_OPEN_REF / _OPEN_TGT when an input cannot be opened (nothing written), SCCG_E_WRITE when
 * the output cannot; SCCG_E_DELTA_STOI writes the un-delta'd text as the reference does. */
int sccg_compress_files(sccg_ctx* ctx, const sccg_params* params, const char* ref_path, const char* tgt_path,
                        const char* out_path, size_t* out_len);

/* match_sequences(Sr, St, k, m, global, offset) on already-uppercased byte strings.  Accepted
 * shapes: global == 0 with |Sr| <= 1000 and |St| <= 1000 (the local-segment kernel), or
 * global == 1 with 0 <= m <= 127 and 1 <= k <= 32 (the windowed global walk).  Others:
 * SCCG_E_UNSUPPORTED.  A global call sets sccg_last_stats' walk fields (n_matches, walk_rounds,
 * walk_chunks, target_bases, walk_reference_bases) as sccg_walk_range does. */
int sccg_match(sccg_ctx* ctx, const uint8_t* sr, size_t nr, const uint8_t* st, size_t nt, int k,
               int m, int global, int64_t offset, sccg_records* out);
void sccg_records_free(sccg_records* r);

/* The global walk of match_sequences(Sr, St, k, m, true) (compression.cpp:64-161) entered at state
 * (index = x0, prev_match_end = P0) and run until the first state with index >= x_end (or until
 * index > |St| - k): its match records (kind 1, pos = p, len = l, t = target index; the literals are
 * the gaps) and that exit state, exit_state[0] = index, exit_state[1] = prev_match_end.  This is the
 * engine of one chromosome's walk split across GPUs (multigpu.split_walk):
 * two walks that reach the same state coincide afterwards.  Sr, St: N-erased, uppercased sequences
 * (R', T' of compression.cpp:556-557).  P0 == -1 (the ungated first step) only with x0 == 0;
 * 0 <= m <= 127, 1 <= k <= 32.  The _device form takes device pointers (stream: hipStream_t or
 * NULL); both return host records (sccg_records_free). */
int sccg_walk_range(sccg_ctx* ctx, const uint8_t* sr, size_t nr, const uint8_t* st, size_t nt, int k, int m,
                    int64_t x0, int64_t P0, int64_t x_end, sccg_records* out, int64_t* exit_state);
int sccg_walk_range_device(sccg_ctx* ctx, const void* d_ref, size_t nr, const void* d_tgt, size_t nt, int k,
                           int m, int64_t x0, int64_t P0, int64_t x_end, sccg_records* out, int64_t* exit_state,
                           void* stream);

/* Decompression after 7z: record text (contents of the extracted compressed_genome.txt) +
 * reference FASTA -> exact bytes of <out>/reconstructed_genome.fa. */
int sccg_reconstruct(sccg_ctx* ctx, const char* ref_fa, size_t ref_len, const char* rec_text,
                     size_t rec_len, sccg_buf* out_fa);
/* HBM-resident form.  With d_out == NULL only *out_len (the exact output size) is computed;
 * with out_cap too small it returns SCCG_E_NOMEM and sets *out_len to the size needed. */
int sccg_reconstruct_device(sccg_ctx* ctx, const void* d_ref_fa, size_t ref_len, const void* d_rec,
                            size_t rec_len, void* d_out, size_t out_cap, size_t* out_len, void* stream);

/* Region reader: ranges of the target read from a record without rebuilding it.  The reference has
 * no counterpart (it writes the whole of reconstructed_genome.fa); the sequence a reader addresses
 * is `result` of decompression.cpp:241-274 after N insertion (:241-249) and lowercasing (:251-262),
 * i.e. the body of reconstructed_genome.fa with its '\n' removed.  Position j of a region is byte j
 * of that string; regions are 0-based and half-open.
 *
 * sccg_reader_open does reconstruct_genome's one-time work once (reference strip :105-110, run
 * lines :126-207, the record line's tokens :210-236 as a block index) and returns exactly the
 * status sccg_reconstruct returns for the same inputs: SCCG_E_FORMAT, _PARSE, _RANGE (every token
 * is checked, :223-229) and the N-beyond-sequence check; on any error *out is NULL.  After an open
 * that succeeds a fetch decodes only valid tokens and re-checks nothing.  The _device form takes
 * device pointers and a hipStream_t (NULL = the context's own stream).
 *
 * A reader owns what it keeps, in device allocations of its own (the context's buffers are reused by
 * its next call): R', the record line, three int64 per 64 record-line bytes, both run lists and the
 * header bytes -- about |R'| + |record line| * 11 / 8 + 16 * N runs + 8 * lowercase runs + 12 KiB.
 * Inputs are not referenced after open returns.  Several readers may be open on one context;
 * sccg_compress / sccg_reconstruct on that context do not disturb them.  A reader uses its context's
 * streams and shares its non-reentrancy (one call at a time per context, readers included); close
 * every reader before sccg_ctx_destroy. */
typedef struct sccg_reader sccg_reader;
typedef struct { int64_t begin, end; } sccg_region;   /* 0-based, half-open, in sequence positions */

int sccg_reader_open(sccg_ctx* ctx, const char* ref_fa, size_t ref_len, const char* rec_text, size_t rec_len,
                     sccg_reader** out);
int sccg_reader_open_device(sccg_ctx* ctx, const void* d_ref_fa, size_t ref_len, const void* d_rec, size_t rec_len,
                            sccg_reader** out, void* stream);
void sccg_reader_close(sccg_reader* reader);                         /* NULL: no-op */
int64_t sccg_reader_length(const sccg_reader* reader);               /* bases in the sequence; -1 for NULL */
const char* sccg_reader_header(const sccg_reader* reader, size_t* len); /* the record's header line ('>'
                                                                        included) without '\n'; len 0 if none */

/* The regions' bases, concatenated in the order given, no separators, no wrapping: region i starts
 * at byte sum_{k<i}(end_k - begin_k).  Regions may overlap, repeat, be empty and come in any order;
 * n == 0 gives an empty output.  One kernel launch and one copy of the region list per call whatever
 * n is; the work follows the bases asked for.  SCCG_E_INVALID for a NULL reader / output, NULL
 * regions with n > 0, or a region outside 0 <= begin <= end <= length (sccg_last_error names the
 * first one; nothing is written).  sccg_reader_fetch returns a malloc'ed buffer (sccg_buf_free).
 * The _device form writes to d_out (capacity out_cap) and sets *out_len; d_out == NULL is a size
 * query, out_cap too small returns SCCG_E_NOMEM with *out_len = the size needed.  Both synchronise
 * before returning. */
#define SCCG_FETCH_UPPER 1u   /* ignore the lowercase runs (decompression.cpp:251-262 skipped) */
int sccg_reader_fetch(sccg_reader* reader, const sccg_region* regions, size_t n, uint32_t flags, sccg_buf* out);
int sccg_reader_fetch_device(sccg_reader* reader, const sccg_region* regions /*host*/, size_t n, uint32_t flags,
                             void* d_out, size_t out_cap, size_t* out_len, void* stream);

/* Encoded fetch: the same regions as ASCII, base indices or one-hot elements, each on either strand.
 * Region i takes bytes_per_base * (end_i - begin_i) bytes at bytes_per_base * sum_{k<i}(end_k -
 * begin_k), no separators; overlapping, repeated, empty and unordered regions and n == 0 as in
 * sccg_reader_fetch.
 *
 *   encoding          dtype   bytes per base   a base's bytes
 *   ----------------  ------  ---------------  -----------------------------------------------------
 *   SCCG_ENC_ASCII    U8       1               the sequence byte (sccg_reader_fetch's)
 *   SCCG_ENC_INDEX    U8       1               A/a 0, C/c 1, G/g 2, T/t 3, every other byte 4
 *   SCCG_ENC_ONEHOT   U8       4               four elements (A, C, G, T): the base's is 1, the others
 *                     F16      8               0; four zeros for a byte that is not ACGTacgt.  1 is
 *                     BF16     8               0x01 / 0x3C00 / 0x3F80 / 0x3F800000
 *                     F32     16
 *
 * Region i is on the reverse strand when strand[i] != 0 (strand: n host bytes, NULL = none) or when
 * SCCG_FETCH_REVCOMP is set (all of them; with both it is still reversed): output base q is sequence
 * position end - 1 - q, complemented.  ASCII complement, case kept: A<->T C<->G R<->Y K<->M B<->V D<->H;
 * S, W, N and every other byte unchanged.  INDEX: 3 - code for codes 0-3, 4 stays; ONEHOT: the same on
 * the channel.  INDEX and ONEHOT are case-blind and never read the lowercase runs; SCCG_FETCH_UPPER
 * acts on ASCII and is accepted and ignored for the others.  ASCII with no strand and no REVCOMP is
 * byte for byte sccg_reader_fetch.
 *
 * SCCG_E_INVALID, nothing written: a NULL reader / format / output, an unknown encoding or dtype, a
 * dtype other than U8 with ASCII or INDEX, an unknown flag bit, reserved != 0, d_out not aligned to
 * the element size, or a bad region (sccg_last_error names the first).  d_out == NULL is a size query;
 * out_cap (bytes) too small returns SCCG_E_NOMEM with *out_len = the bytes needed.  One copy of the
 * region list (the strands in it) and one kernel launch per call whatever n is; both forms
 * synchronise before returning. */
#define SCCG_ENC_ASCII   0u
#define SCCG_ENC_INDEX   1u
#define SCCG_ENC_ONEHOT  2u
#define SCCG_DT_U8   0u
#define SCCG_DT_F16  1u
#define SCCG_DT_BF16 2u
#define SCCG_DT_F32  3u   /* ONEHOT's element type; must be SCCG_DT_U8 for ASCII and INDEX */
#define SCCG_FETCH_REVCOMP 2u   /* every region on the reverse strand */
typedef struct { uint32_t encoding, dtype, flags, reserved /* 0 */; } sccg_fetch_format;

/* Origin fetch: where each base comes from.  The format {SCCG_ENC_ORIGIN, SCCG_DT_I32, flags, 0} is taken
 * by sccg_reader_fetch_encoded[_device] and sccg_cohort_fetch[_device]; a base is one little-endian int32:
 *
 *   r >= 0   a token copied the base from position r of the reference sequence R -- the reference
 *            file's non-header lines joined, whitespace removed (decompression.cpp:53-58), 0-based; for
 *            a one-record FASTA r + 1 is the samtools faidx coordinate.  NOT a position of R' (the
 *            N-erased string the tokens index, decompression.cpp:105-110): the library maps it back.
 *   -1       a literal: the base is carried by the record line itself
 *   -2       a base of one of the target's N runs (inserted from the N line, decompression.cpp:241-249;
 *            it is in neither R' nor the record line)
 *
 * Layout, the region rules (empty, repeated, overlapping, unordered, n == 0), the size query and
 * SCCG_E_NOMEM with the bytes needed are the encoded fetch's, at 4 bytes per base; d_out must be 4-byte
 * aligned (else SCCG_E_INVALID); one copy of the region list and one kernel launch per call.  Output
 * base q of a reversed region is position end - 1 - q and its value is that position's origin,
 * unchanged: a reference position is not complemented.  The encoding is case-blind: SCCG_FETCH_UPPER
 * is accepted and ignored and the lowercase runs are never read.  Every other dtype with ORIGIN, and
 * I32 with any other encoding, is SCCG_E_INVALID.
 *
 * Which readers have reference coordinates (sccg_reader_has_coords): one whose record's N line is ","
 * always (R' is R position for position), private or shared; one whose record indexes the erased
 * form only when it was opened through a sccg_reference whose `forms` carried SCCG_REF_COORDS, which
 * keeps the R' -> R map (below).  An ORIGIN fetch on a reader without them returns SCCG_E_UNSUPPORTED
 * -- the size query too; nothing is written; sccg_last_error says which.  In a cohort, bad regions
 * (SCCG_E_INVALID) and regions of samples without coordinates (SCCG_E_UNSUPPORTED) are found in one
 * pass: the first offending region in list order decides the status and is named.  Format errors come
 * first; the coordinate check is made for ORIGIN only. */
#define SCCG_ENC_ORIGIN 3u   /* where each base comes from; dtype must be SCCG_DT_I32 */
#define SCCG_DT_I32     4u   /* valid with SCCG_ENC_ORIGIN only */
int sccg_reader_has_coords(const sccg_reader* reader);   /* 1 / 0; 0 for NULL */

size_t sccg_fetch_bytes_per_base(const sccg_fetch_format* fmt);   /* 1, 1, 4, 8, 8, 16; ORIGIN 4; 0 = invalid format */
int sccg_reader_fetch_encoded(sccg_reader* reader, const sccg_region* regions, size_t n, const uint8_t* strand,
                              const sccg_fetch_format* fmt, sccg_buf* out);
int sccg_reader_fetch_encoded_device(sccg_reader* reader, const sccg_region* regions /*host*/, size_t n,
                                     const uint8_t* strand, const sccg_fetch_format* fmt, void* d_out,
                                     size_t out_cap /*bytes*/, size_t* out_len /*bytes*/, void* stream);

/* Shared reference: R' -- the stripped, uppercased reference every token of a record indexes -- held
 * once for all the readers opened over it.  A private reader (sccg_reader_open) keeps a copy of its
 * own, by far the largest thing it holds; a hundred samples over one reference would hold a hundred.
 *
 * A record's N line decides which R' its tokens index: with an N-run line the reference's 'N' are
 * erased before uppercasing (decompression.cpp:105-110; a lowercase 'n' stays, as "N"), with the N
 * line "," -- a pair that stayed in local mode -- they are kept.  Neither form can be derived from
 * the other on the device, so a reference holds the forms asked for (`forms`: SCCG_REF_ERASED,
 * SCCG_REF_KEPT or both; 0 = both), each made by the very strip sccg_reader_open runs and kept in a
 * device allocation of the reference's own.  sccg_reference_device_bytes is their sum (0 for NULL).
 *
 * sccg_reader_open_shared does everything sccg_reader_open does except the strip and the copy of R':
 * it returns exactly the status sccg_reader_open returns for the same reference and record
 * (SCCG_E_FORMAT, _PARSE, _RANGE, in that order), and SCCG_E_UNSUPPORTED, with sccg_last_error naming
 * the form, for a record that needs a form the reference was opened without (known once the record's
 * lines are, so after SCCG_E_FORMAT).  On any error *out is NULL.  Every reader call works on a
 * shared reader and returns byte for byte what it returns on a private one.  The reader lives on the
 * reference's context and shares its non-reentrancy.
 *
 * A reference is counted by its readers: sccg_reference_close drops the caller's hold (no further
 * open through it), and the memory goes with the last reader's sccg_reader_close.  All of that
 * happens before sccg_ctx_destroy.  sccg_reader_device_bytes is the reader's own persistent
 * allocation (for a private reader R' included; the staging a fetch grows is not counted); 0 for NULL.
 * The _device forms take device pointers and a hipStream_t (NULL = the context's own stream).
 *
 * `forms` is a mask of forms plus one option, SCCG_REF_COORDS: also keep the R' -> R map the origin
 * fetch needs for the erased form -- the maximal runs of uppercase 'N' in R (a lowercase 'n' is not
 * erased), found on the device at open; 16 bytes per run, counted by sccg_reference_device_bytes.
 * SCCG_REF_COORDS alone is both forms plus the map; with form bits, those forms plus the map (with
 * SCCG_REF_KEPT alone the map is empty: the kept form needs none).  Without the bit every allocation
 * and sccg_reference_device_bytes are what they are without this option.  Any other bit is
 * SCCG_E_INVALID; a reference of 2^31 - 1 bases or more cannot carry the map (SCCG_E_UNSUPPORTED). */
typedef struct sccg_reference sccg_reference;
#define SCCG_REF_ERASED 1u   /* R' as a record with an N-run line needs it (N erased, decompression.cpp:105-110) */
#define SCCG_REF_KEPT   2u   /* R' as a record whose N line is "," needs it (N kept) */
#define SCCG_REF_COORDS 4u   /* option: keep the R' -> R map (reference coordinates for SCCG_ENC_ORIGIN) */
int sccg_reference_open(sccg_ctx* ctx, const char* ref_fa, size_t ref_len, uint32_t forms /*0 = both*/, sccg_reference** out);
int sccg_reference_open_device(sccg_ctx* ctx, const void* d_ref_fa, size_t ref_len, uint32_t forms, sccg_reference** out,
                               void* stream);
void sccg_reference_close(sccg_reference* ref);             /* NULL: no-op */
size_t sccg_reference_device_bytes(const sccg_reference* ref);
int sccg_reader_open_shared(sccg_reference* ref, const char* rec_text, size_t rec_len, sccg_reader** out);
int sccg_reader_open_shared_device(sccg_reference* ref, const void* d_rec, size_t rec_len, sccg_reader** out, void* stream);
size_t sccg_reader_device_bytes(const sccg_reader* reader);

/* Cohort: the encoded fetch over many readers at once, each region naming its sample -- a batch of
 * windows drawn from many individuals costs one copy of the region list, one kernel launch and one
 * synchronise, whatever n and the number of samples touched are.
 *
 * sccg_cohort_create takes n_samples readers, private or shared in any mix; a reader may appear
 * twice.  All of them are on one context: anything else, n_samples == 0 or a NULL entry is
 * SCCG_E_INVALID (*out NULL).  The cohort does NOT own its readers: it keeps a device table of what
 * each reads, written once at create, so close the cohort BEFORE any of its readers, and every cohort
 * before sccg_ctx_destroy.  It owns that table and region staging of its own, so sccg_compress /
 * sccg_reconstruct and the readers' own fetches on the context do not disturb it; it shares the
 * context's non-reentrancy.  sccg_cohort_close(NULL) is a no-op; sccg_cohort_samples(NULL) is 0.
 *
 * sccg_cohort_fetch / _device: region i is [begin, end) of sample `sample`, 0-based and half-open in
 * that sample's sequence positions, on the reverse strand when bit 0 of `flags` is set or when the
 * format carries SCCG_FETCH_REVCOMP (all regions; with both it is still reversed).  Output layout,
 * encodings, dtypes, format flags, the size query (d_out == NULL), SCCG_E_NOMEM with *out_len = the
 * bytes needed, and the alignment rule are exactly sccg_reader_fetch_encoded[_device]'s: region i
 * takes bytes_per_base * (end - begin) bytes at the running offset, no separators; regions may be
 * empty, repeat, overlap and come in any order of positions and samples; n == 0 gives an empty output.
 *
 * SCCG_E_INVALID, nothing written, sccg_last_error naming the first offender: every format error of
 * the encoded fetch, a region with a flag bit other than bit 0, a sample outside [0, n_samples), or a
 * region outside its own sample's 0 <= begin <= end <= length.  Both forms synchronise before
 * returning; stream is a hipStream_t (NULL = the context's own). */
typedef struct sccg_cohort sccg_cohort;
typedef struct { int64_t begin, end; int32_t sample; uint32_t flags; } sccg_cohort_region;  /* flags bit 0: reverse strand; others 0 */
int sccg_cohort_create(sccg_reader* const* readers, size_t n_samples, sccg_cohort** out);
void sccg_cohort_close(sccg_cohort* cohort);                 /* NULL: no-op */
size_t sccg_cohort_samples(const sccg_cohort* cohort);
int sccg_cohort_fetch(sccg_cohort* cohort, const sccg_cohort_region* regions, size_t n, const sccg_fetch_format* fmt, sccg_buf* out);
int sccg_cohort_fetch_device(sccg_cohort* cohort, const sccg_cohort_region* regions /*host*/, size_t n,
                             const sccg_fetch_format* fmt, void* d_out, size_t out_cap /*bytes*/, size_t* out_len /*bytes*/,
                             void* stream);

/* Locate: the inverse of the origin fetch -- where a position of the reference sequence lies in a sample.
 * A cohort over one shared reference is asked "the window at reference position r in each of these
 * samples"; with indels upstream r is another sequence position in every one of them.
 *
 * For a reader with reference coordinates (sccg_reader_has_coords) let origin(j) be what SCCG_ENC_ORIGIN
 * returns for sequence position j.  For a reference position r, 0 <= r < |R|, in the coordinates the
 * origin fetch reports (a position of R, not of R'):
 *
 *   copies   the number of sequence positions j with origin(j) == r: the tokens of nonzero length whose
 *            R' interval holds r
 *   pos      the smallest such j when copies > 0 -- a sequence position as every fetch takes it (after
 *            N insertion); it belongs to the first covering token in record order
 *   pos = SCCG_LOCATE_NONE   no token copies r: the base is deleted in this sample, or the sample
 *            carries it as a literal; copies 0
 *   pos = SCCG_LOCATE_REF_N  r lies in a run of uppercase 'N' that the record's R' has erased; copies
 *            0.  The erased form only: for a record whose N line is "," R' is R and an 'N' is a base
 *            like any other.
 *
 * sccg_reader_enable_locate builds the reader's locate index on the device, once (a second call is a
 * no-op returning SCCG_OK): the tokens by reference position -- every token start and end sorted, the
 * number of tokens over each interval between them, and a segment tree of the first token in record
 * order over each, so a query costs O(log tokens) loads whatever the overlap; at most 44 bytes per
 * token, in a device allocation of the reader's own that sccg_reader_close frees and that
 * sccg_reader_device_bytes counts from then on.  SCCG_E_UNSUPPORTED for a reader without reference
 * coordinates (sccg_last_error says which, as for the origin fetch) or of 2^31 - 1 tokens or R' bases
 * and more; SCCG_E_NOMEM when the index cannot be allocated -- the reader is then as it was.  A reader
 * that never calls it allocates and costs what it did.  sccg_reader_can_locate: 1 after it succeeded.
 *
 * sccg_reader_locate / _device: pos[i] and, when `copies` is given, copies[i] for ref_pos[i], i < n;
 * positions may repeat and come in any order.  One copy of the query list, one kernel launch and one
 * synchronise per call whatever n is; n == 0 is SCCG_OK and writes nothing.  The _device form writes
 * int64 to d_pos and int32 to d_copies (may be NULL) in device memory, on `stream` (a hipStream_t; NULL
 * = the context's own).  SCCG_E_INVALID, nothing written, sccg_last_error naming the first offender: a
 * NULL reader; NULL ref_pos or pos / d_pos with n > 0; d_pos not 8-byte or d_copies not 4-byte aligned;
 * a ref_pos outside [0, |R|).  SCCG_E_UNSUPPORTED on a reader that has not enabled locating.
 *
 * sccg_cohort_locate / _device: locus i is reference position ref_pos of sample `sample`; flags must
 * be 0.  A cohort's device table is written at sccg_cohort_create, so a reader is locatable through a
 * cohort only if it had enabled locating BEFORE the cohort was created; enabling it later serves the
 * reader's own calls and the cohorts created after.  The loci are checked in one pass and the first
 * offender in list order decides the status and is named: SCCG_E_INVALID for a nonzero flags, a sample
 * outside [0, n_samples) or a ref_pos outside that sample's [0, |R|); SCCG_E_UNSUPPORTED for a locus
 * whose sample had not enabled locating.  Everything else as the reader's calls; `copies` / d_copies may
 * be NULL here too. */
#define SCCG_LOCATE_NONE  (-1)
#define SCCG_LOCATE_REF_N (-2)
typedef struct { int64_t ref_pos; int32_t sample; uint32_t flags /* 0 */; } sccg_cohort_locus;
int sccg_reader_enable_locate(sccg_reader* reader);
int sccg_reader_can_locate(const sccg_reader* reader);   /* 1 / 0; 0 for NULL */
int sccg_reader_locate(sccg_reader* reader, const int64_t* ref_pos /*host*/, size_t n, int64_t* pos /*host, n*/,
                       int32_t* copies /*host, n; may be NULL*/);
int sccg_reader_locate_device(sccg_reader* reader, const int64_t* ref_pos /*host*/, size_t n, void* d_pos,
                              void* d_copies /*may be NULL*/, void* stream);
int sccg_cohort_locate(sccg_cohort* cohort, const sccg_cohort_locus* loci, size_t n, int64_t* pos, int32_t* copies);
int sccg_cohort_locate_device(sccg_cohort* cohort, const sccg_cohort_locus* loci /*host*/, size_t n, void* d_pos,
                              void* d_copies, void* stream);

/* Segments: a region's alignment to the reference, run-length coded -- the gapless blocks where the
 * sample follows the reference, and the literals and N runs between them.  What the origin fetch says with
 * 4 bytes per base, this says with 24 bytes per segment, and its work is in proportion to the record-line
 * bytes under the regions, not to their bases.
 *
 * For a reader with reference coordinates (sccg_reader_has_coords) let origin(j) be what SCCG_ENC_ORIGIN
 * returns for sequence position j.  A segment of region [begin, end) is a maximal interval [a, b) inside
 * it such that for every j in [a, b - 1) origin(j) >= 0 and origin(j + 1) == origin(j) + 1, or both are
 * -1, or both are -2; it is reported as {pos = a, len = b - a, ref = origin(a)}.  The segments of a region
 * tile it exactly, in ascending pos; an empty region has none; they are clipped to the region, so ref
 * belongs to the first base inside it.  The definition speaks of bases, never of tokens: a token that
 * starts where the one before it ends, on the reference too, continues its segment (zero-length tokens
 * between them change nothing); a token is split by a target N run put into it, and where its interval of
 * R' crosses an erased run of 'N' in R (the origin jumps there); touching N runs of the target form one
 * -2 segment.
 *
 * The segments of region i are out[off[i], off[i + 1]), off[0] == 0, off[n] the total; regions may be
 * empty, repeat, overlap and come in any order; n == 0 is SCCG_OK with no segments (off[0] = 0).  The
 * host forms return the sccg_segment array in *out (out->len bytes; sccg_buf_free) and, when `off` is
 * given, the n + 1 offsets.  The _device forms write int64 offsets to d_off (may be NULL) and segments
 * to d_seg, device memory, on `stream` (a hipStream_t; NULL = the context's own): d_seg == NULL is a size
 * query that only sets *n_seg; with cap (in segments) too small they return SCCG_E_NOMEM, *n_seg the number
 * needed, the buffers' contents unspecified.  Forward strand only.  Six kernel launches and one host read
 * (the total) per call, whatever n, the region sizes and the samples touched are (four for a size query).
 * The locate index is not needed.
 *
 * SCCG_E_INVALID, nothing written, sccg_last_error naming the first offender: a NULL reader / cohort /
 * out / n_seg; a NULL region list with n > 0; d_off or d_seg not 8-byte aligned; a region outside 0 <=
 * begin <= end <= length; in a cohort a sample outside [0, n_samples) or ANY flag bit set, bit 0 included.
 * SCCG_E_UNSUPPORTED, the size query included: a reader without reference coordinates; in a cohort the
 * regions are checked in one pass and the first offender in list order decides the status.  Both forms
 * synchronise before returning. */
typedef struct { int64_t pos, len, ref; } sccg_segment;   /* ref >= 0, -1 literal, -2 target N run */
int sccg_reader_segments(sccg_reader* reader, const sccg_region* regions, size_t n, int64_t* off /*host, n + 1; may be NULL*/,
                         sccg_buf* out /*sccg_segment[]*/);
int sccg_reader_segments_device(sccg_reader* reader, const sccg_region* regions /*host*/, size_t n,
                                void* d_off /*int64[n + 1] or NULL*/, void* d_seg, size_t cap /*segments*/, size_t* n_seg,
                                void* stream);
int sccg_cohort_segments(sccg_cohort* cohort, const sccg_cohort_region* regions, size_t n, int64_t* off, sccg_buf* out);
int sccg_cohort_segments_device(sccg_cohort* cohort, const sccg_cohort_region* regions /*host*/, size_t n, void* d_off, void* d_seg,
                                size_t cap, size_t* n_seg, void* stream);

/* Lift: intervals of the reference onto a sample, run-length coded -- where an exon, an enhancer, a BED
 * line of the reference lies in the sample, and which parts of it are missing.  What locate says with 12
 * bytes per reference base, this says with 24 bytes per block, and its work is in proportion to the token
 * boundaries and runs under the intervals, not to their bases: segments, mirrored onto the reference axis.
 *
 * For a reader that has enabled locating (sccg_reader_enable_locate) let pos(r) be what sccg_reader_locate
 * returns for reference position r, 0 <= r < |R|.  A block of interval [begin, end) is a maximal interval
 * [a, b) inside it such that for every r in [a, b - 1) pos(r) >= 0 and pos(r + 1) == pos(r) + 1, or both
 * are -1, or both are -2; it is reported as {ref = a, len = b - a, pos = pos(a)}.  The blocks of an
 * interval tile it exactly, in ascending ref; an empty interval has none; they are clipped to the interval,
 * so pos belongs to the first reference base inside it; no two neighbours could merge.  The definition
 * speaks of bases, never of tokens:
 *   - a block goes on where the same first covering token goes on (later tokens over it, nested or
 *     overlapping, change `copies`, not pos), and where another token continues it on both axes: "(100,30)
 *     (130,20)" back to back is one block, zero-length tokens between them change nothing;
 *   - it is cut where a target N run was put into a token (pos jumps there), and where the first covering
 *     token ends and a different one takes over;
 *   - it is cut on both sides of every erased run of 'N' in R: each such run, or its part inside the
 *     interval, is one -2 block.  A record whose N line is "," has no -2 blocks;
 *   - positions before the first token boundary, behind the last one or in an uncovered gap give -1 blocks;
 *     a record without any token gives -1 and -2 blocks only;
 *   - with duplicated reference bases (copies > 1) the lift follows locate: the first covering token in
 *     record order wins.  `copies` is not reported -- it is not constant over a block; locate gives it per
 *     position.
 *
 * The layout is sccg_*_segments*'s: the blocks of interval i are out[off[i], off[i + 1]), off[0] == 0,
 * off[n] the total; intervals may be empty, repeat, overlap and come in any order of positions and samples;
 * n == 0 is SCCG_OK with no blocks (off[0] = 0).  The host forms return the sccg_lift_block array in *out
 * (out->len bytes; sccg_buf_free) and, when `off` is given, the n + 1 offsets.  The _device forms write
 * int64 offsets to d_off (may be NULL) and blocks to d_blk, device memory, on `stream` (a hipStream_t; NULL =
 * the context's own): d_blk == NULL is a size query that only sets *n_blk; with cap (in blocks) too small
 * they return SCCG_E_NOMEM, *n_blk the number needed, the buffers' contents unspecified.  Both forms
 * synchronise before returning.
 *
 * Costs: the locate index is read exactly as it is and gets no new array, so sccg_reader_device_bytes does
 * not change; the scratch lives in the staging the call grows, as for segments.  Six kernel launches, one
 * copy of the interval list and one host read (the total) per call, whatever n, the interval sizes and the
 * samples touched are (four launches for a size query).
 *
 * SCCG_E_INVALID, nothing written, sccg_last_error naming the first offender ("interval k"): a NULL reader /
 * cohort / out / n_blk; a NULL list with n > 0; d_off or d_blk not 8-byte aligned; an interval outside 0 <=
 * begin <= end <= |R| of its own sample; in a cohort a sample outside [0, n_samples) or any flag bit set.
 * SCCG_E_UNSUPPORTED, the size query included: a reader that has not enabled locating; in a cohort an
 * interval whose sample had not enabled locating before sccg_cohort_create.  The intervals are checked in
 * one pass and the first offender in list order decides the status. */
typedef struct { int64_t ref, len, pos; } sccg_lift_block;   /* pos >= 0, -1 no copy, -2 erased N of the reference */
int sccg_reader_lift(sccg_reader* reader, const sccg_region* intervals /*of R, 0-based half-open*/, size_t n,
                     int64_t* off /*host, n + 1; may be NULL*/, sccg_buf* out /*sccg_lift_block[]*/);
int sccg_reader_lift_device(sccg_reader* reader, const sccg_region* intervals /*host*/, size_t n,
                            void* d_off /*int64[n + 1] or NULL*/, void* d_blk, size_t cap /*blocks*/, size_t* n_blk, void* stream);
int sccg_cohort_lift(sccg_cohort* cohort, const sccg_cohort_region* intervals, size_t n, int64_t* off, sccg_buf* out);
int sccg_cohort_lift_device(sccg_cohort* cohort, const sccg_cohort_region* intervals /*host*/, size_t n, void* d_off, void* d_blk,
                            size_t cap, size_t* n_blk, void* stream);

/* Find: where a pattern -- a primer, a restriction site, a guide + PAM, a motif -- occurs in regions of a
 * sample, on either strand.  The first reader call whose answer depends on the bases themselves: the regions
 * are decoded and matched in one pass on the device, and no base is written to memory.
 *
 * The pattern is m letters, 1 <= m <= SCCG_FIND_MAX_PATTERN, of the IUPAC nucleotide alphabet
 * ACGTURYSWKMBDHVN in either case (U means T).  A letter stands for a set of {A, C, G, T}, held as a 4-bit
 * mask (bit 0 A, 1 C, 2 G, 3 T): R = AG, Y = CT, S = CG, W = AT, K = GT, M = AC, B = CGT, D = AGT, H = ACT,
 * V = ACG, N = ACGT.  A sequence position j has code(j), SCCG_ENC_INDEX's: A/a 0, C/c 1, G/g 2, T/t 3, every
 * other byte 4 -- a base of a target N run, a literal 'N' and any other byte alike.  The search is case-blind
 * and never reads the lowercase runs.  CODE 4 MATCHES NO PATTERN LETTER, NOT EVEN 'N': the pattern letter N
 * means "any of A, C, G, T", so a window holding an N base is never a hit.
 *
 * Position j of region [begin, end) is a forward hit iff j + m <= end and mask[t] has bit code(j + t) for
 * every t < m: a window that would match but crosses `end` is no hit of that region.  It is a reverse hit iff
 * the reverse complement of seq[j, j + m) matches the pattern, which is the forward window matching the
 * reverse-complemented pattern (the masks reversed, A <-> T and C <-> G swapped in each); it is reported at
 * the same pos = j, the leftmost forward coordinate, with strand 1.  A palindromic site such as GAATTC is
 * hit on both strands at the same pos and gives two rows.  flags: SCCG_FIND_FWD searches the forward strand,
 * SCCG_FIND_REV the reverse strand, both together both; 0 means forward only.
 *
 * The layout is sccg_*_segments*'s: the hits of region i are out[off[i], off[i + 1]), off[0] == 0, off[n]
 * the total, in ascending pos, forward before reverse at equal pos; regions may be empty, shorter than m (no
 * hits), repeat, overlap and come in any order; n == 0 is SCCG_OK with no hits (off[0] = 0).  The result is
 * deterministic: the same call gives the same bytes.  The host forms return the sccg_hit array in *out
 * (out->len bytes; sccg_buf_free) and, when `off` is given, the n + 1 offsets.  The _device forms write int64
 * offsets to d_off (may be NULL) and hits to d_hit, device memory, on `stream` (a hipStream_t; NULL = the
 * context's own): d_hit == NULL is a size query that only sets *n_hit; with cap (in hits) too small they
 * return SCCG_E_NOMEM, *n_hit the number needed, the buffers' contents unspecified.  Both forms synchronise
 * before returning.
 *
 * Any reader can be searched, private or shared, with or without reference coordinates; the locate index is
 * not needed.  Costs: three kernel launches (two for a size query), one copy of the region list -- the masks
 * travel in the kernel arguments -- and one host read (the total) per call, whatever n, the region sizes and
 * the samples touched are.  The scratch (2 bits per candidate start) lives in the staging the call grows, as
 * for segments; sccg_reader_device_bytes does not change.
 *
 * SCCG_E_INVALID, nothing written, sccg_last_error naming the first offender.  In this order: a NULL reader /
 * cohort / out / n_hit (no message); a NULL pattern, m == 0, m > SCCG_FIND_MAX_PATTERN or a byte outside the
 * alphabet ("pattern byte k"); a flag bit other than SCCG_FIND_FWD | SCCG_FIND_REV; d_off or d_hit not 8-byte
 * aligned; then the regions as for segments: a NULL list with n > 0, a region outside 0 <= begin <= end <=
 * length, in a cohort a sample outside [0, n_samples) or ANY flag bit of a region set, bit 0 included (the
 * strands are the call's, not a region's).
 *
 * sccg_find_pattern_masks is a pure host function, no context: the m masks of a pattern in fwd and of its
 * reverse complement in rev (either may be NULL), what the kernels are launched with; SCCG_E_INVALID as
 * above. */
#define SCCG_FIND_MAX_PATTERN 64
#define SCCG_FIND_FWD 1u
#define SCCG_FIND_REV 2u
typedef struct { int64_t pos, strand; } sccg_hit;   /* strand 0 forward, 1 reverse */
int sccg_find_pattern_masks(const char* pattern, size_t m, uint8_t* fwd /*m*/, uint8_t* rev /*m*/);
int sccg_reader_find(sccg_reader* reader, const char* pattern, size_t m, const sccg_region* regions, size_t n, uint32_t flags,
                     int64_t* off /*host, n + 1; may be NULL*/, sccg_buf* out /*sccg_hit[]*/);
int sccg_reader_find_device(sccg_reader* reader, const char* pattern, size_t m, const sccg_region* regions /*host*/, size_t n,
                            uint32_t flags, void* d_off /*int64[n + 1] or NULL*/, void* d_hit, size_t cap /*hits*/, size_t* n_hit,
                            void* stream);
int sccg_cohort_find(sccg_cohort* cohort, const char* pattern, size_t m, const sccg_cohort_region* regions, size_t n, uint32_t flags,
                     int64_t* off, sccg_buf* out);
int sccg_cohort_find_device(sccg_cohort* cohort, const char* pattern, size_t m, const sccg_cohort_region* regions /*host*/, size_t n,
                            uint32_t flags, void* d_off, void* d_hit, size_t cap, size_t* n_hit, void* stream);

/* Find with mismatches: where the pattern occurs within max_mismatches substitutions (Hamming distance; no
 * gaps) -- the off-target sites of a guide + PAM, the places a primer still binds.  Find's alphabet, masks,
 * reverse-complement rule, codes, flags and layout; what differs is said here.
 *
 * For a candidate start j of a region, a strand s (0 forward, 1 reverse) and that strand's masks (the
 * pattern's; the reverse-complemented pattern's), d(j, s) is the number of t < m where mask_s[t] lacks bit
 * code(j + t).  CODE 4 -- a base of a target N run, a literal 'N', any other byte -- IS A MISMATCH AGAINST
 * EVERY LETTER, 'N' INCLUDED.  (j, s) is a hit iff j + m <= end and d(j, s) <= K = max_mismatches: a window
 * never crosses its region's end, whatever K is.  Rows are sccg_hit_mm {pos, strand, mismatches = d(j, s)},
 * 24 bytes, in Find's order: out[off[i], off[i + 1]) region i's, ascending pos, forward before reverse at
 * equal pos -- where the two strands may carry different mismatches.  K = 0 gives exactly Find's rows with a
 * third column of zeros.  Limits: 0 <= K <= SCCG_FIND_MAX_MISMATCHES and K < m; a pattern all of whose
 * letters may mismatch says nothing and would return every window.
 *
 * The host and _device forms, the size query (d_hit == NULL), cap (in hits) / SCCG_E_NOMEM with *n_hit set,
 * the 8-byte alignment of d_off / d_hit, `stream` and the synchronise before returning are Find's.  Costs:
 * three kernel launches (two for a size query), one copy of the region list -- the masks and K travel in the
 * kernel arguments -- and one host read (the total) per call.  The scratch, 2 bits and two 4-bit distances
 * per candidate start (34 + 128 words of 8 bytes per 960 candidates, 1.35 bytes a candidate), lives in the
 * staging the call grows; sccg_reader_device_bytes does not change.
 *
 * SCCG_E_INVALID, nothing written, sccg_last_error naming the first offender, in this order: NULL handles,
 * out or n_hit (no message); the pattern, as Find; unknown flag bits; max_mismatches >
 * SCCG_FIND_MAX_MISMATCHES or >= m (the message holds the word "mismatches" and the number); alignment;
 * the regions, exactly as Find. */
#define SCCG_FIND_MAX_MISMATCHES 15
typedef struct { int64_t pos, strand, mismatches; } sccg_hit_mm;   /* strand 0 forward, 1 reverse */
int sccg_reader_find_approx(sccg_reader* reader, const char* pattern, size_t m, const sccg_region* regions, size_t n, uint32_t flags,
                            uint32_t max_mismatches, int64_t* off /*host, n + 1; may be NULL*/, sccg_buf* out /*sccg_hit_mm[]*/);
int sccg_reader_find_approx_device(sccg_reader* reader, const char* pattern, size_t m, const sccg_region* regions /*host*/, size_t n,
                                   uint32_t flags, uint32_t max_mismatches, void* d_off /*int64[n + 1] or NULL*/, void* d_hit,
                                   size_t cap /*hits*/, size_t* n_hit, void* stream);
int sccg_cohort_find_approx(sccg_cohort* cohort, const char* pattern, size_t m, const sccg_cohort_region* regions, size_t n,
                            uint32_t flags, uint32_t max_mismatches, int64_t* off, sccg_buf* out);
int sccg_cohort_find_approx_device(sccg_cohort* cohort, const char* pattern, size_t m, const sccg_cohort_region* regions /*host*/,
                                   size_t n, uint32_t flags, uint32_t max_mismatches, void* d_off, void* d_hit, size_t cap,
                                   size_t* n_hit, void* stream);

void sccg_buf_free(sccg_buf* b);

/* Per-kernel device timing with HIP events recorded on the launching stream (process-wide).
 * sccg_profile(ctx, 1) resets and enables it for every family, 0 disables it (enable > 1: a bit
 * mask as below, kept for old callers -- it cannot select family 0 alone).  sccg_profile_mask
 * resets and enables it for the families of `mask` (bit i = sccg_profile_name(i); 0 disables).
 * sccg_profile_get returns the summed duration and launch count of one kernel family by name
 * (sccg_profile_name(i), i = 0.. until NULL). */
int sccg_profile(sccg_ctx* ctx, int enable);
int sccg_profile_mask(sccg_ctx* ctx, uint32_t mask);
int sccg_profile_get(sccg_ctx* ctx, const char* kernel, double* total_ms, int64_t* launches);
const char* sccg_profile_name(int i);

#ifdef __cplusplus
}
#endif
#endif
