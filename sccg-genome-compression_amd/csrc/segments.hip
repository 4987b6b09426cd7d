// segments.hip -- origin segments: a region's alignment to the reference, run-length coded.
//
// With origin(j) what the origin fetch (decomp.hip: k_fetch_origin) returns for sequence position j, a
// segment of region [j0, j1) is a maximal interval whose bases continue each other: reference positions
// ascending by one, or all literals (-1), or all bases of the target's N runs (-2).  The decoder knows
// every boundary while it parses tokens; this file keeps them, and does work in proportion to the
// record-line bytes under the regions -- never to their bases:
//   k_sg_regions   a region per lane: positions -> decoded offsets [d0, d1) over the N runs -> its first
//                  record block and block count over boff (fetch_decode_span's front), whether its first
//                  and its last base are N.  Region i gets nb[i] + 1 work items: its record blocks, then
//                  a tail item (the N run a region ends in; it also closes an empty region).
//   k_sg_scan      one block: the exclusive prefix of the items (the flat work space), later of the
//                  waves' counts.
//   k_sg_blocks    W waves share the flat space in equal consecutive chunks.  A wave parses a block as
//                  k_tok_fill2 does and every base-producing element, clipped to [d0, d1), counts its
//                  segment starts: a literal byte one if the base before it is no literal; a token one if
//                  it does not continue the base before it, one wherever a run of 'N' that R' has erased
//                  is crossed (the origin jumps) and two for every group of touching target N runs put
//                  into it (the N segment, and the token going on behind it) -- by a search of the run
//                  keys (start - cum, as map_seek's) and a walk of the runs found, not of bases.  <false>
//                  leaves the wave's count, <true> runs again from the scanned counts and stores
//                  {pos, ref} of the k-th start at slot k, and the regions' offsets.
//   k_sg_len       a segment per lane: len = the next start of the same region, or the region's end,
//                  minus pos (k_refn_write's k-th start pairs with the k-th end: O(1) stores a segment).
// The base before a block: a block's first element must know the origin of the last base produced
// before the block, which zero-length tokens and straddling token text put any number of blocks back.
// A wave carries it along its consecutive blocks; for the first block of its chunk it searches boff for
// the block that holds decoded byte boff[b] - 1 and parses that one.  Nothing walks backwards, every
// loop is bounded by a data size, no wave waits for another.
#include "internal.h"
#include "recparse.h"
#include "segments.h"

namespace {

constexpr int WPB = SCCG_BLOCK / 64;
constexpr int TK_B = 64;           // record bytes per block (decomp.hip's block index)
constexpr int SG_STEPS = 64;       // bound of every halving search here (< 2^63 entries end sooner)
constexpr int SG_WAVES = 4096;     // the most waves that share the flat space
constexpr int SG_SCAN_PER = 16;    // k_sg_scan: entries per thread and round
constexpr int SG_LEN_BLOCKS = 2048;   // the most blocks of k_sg_len (they stride over the segments)
constexpr int64_t NO_PREV = -3;    // "the base before": unknown / none (never compared: the element starts its region)

__device__ __forceinline__ int64_t readlane64(int64_t v, int l) {
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, l);
    const int hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

__device__ __forceinline__ int64_t run_key(const DcRuns& M, int64_t m) { return (int64_t)M.start[m] - M.cum[m]; }
// the run bases before run m (m == M.n: all of them)
__device__ __forceinline__ int64_t run_cum(const DcRuns& M, int64_t m) { return m < M.n ? M.cum[m] : (M.n ? M.total : 0); }
// first m with key(m) >= v (GT: > v); the keys ascend
template <bool GT>
__device__ __forceinline__ int64_t run_key_first(const DcRuns& M, int64_t v) {
    int64_t a = 0, b = M.n;
    for (int it = 0; it < SG_STEPS && a < b; it++) {
        const int64_t m = (a + b) >> 1;
        const int64_t k = run_key(M, m);
        if (GT ? k > v : k >= v) b = m; else a = m + 1;
    }
    return a;
}
// first run ending after sequence position j
__device__ __forceinline__ int64_t run_end_after(const DcRuns& M, int64_t j) {
    int64_t a = 0, b = M.n;
    for (int it = 0; it < SG_STEPS && a < b; it++) {
        const int64_t m = (a + b) >> 1;
        if ((int64_t)M.start[m] + M.len[m] > j) b = m; else a = m + 1;
    }
    return a;
}
// first m in [a, b) with boff[m] >= d (GT: > d), b if none
template <bool GT>
__device__ __forceinline__ int64_t boff_first(const int64_t* __restrict__ boff, int64_t a, int64_t b, int64_t d) {
    for (int it = 0; it < SG_STEPS && a < b; it++) {
        const int64_t m = (a + b) >> 1;
        if (GT ? boff[m] > d : boff[m] >= d) b = m; else a = m + 1;
    }
    return a;
}
// the position in R of R' position v
__device__ __forceinline__ int64_t ref_pos(const DcRuns& M, int64_t v) {
    return M.n ? v + run_cum(M, run_key_first<true>(M, v)) : v;
}

struct SgArgs {
    DcCohortEntry E;            // the reader's source (!COHORT)
    const DcCohortEntry* tab;   // one entry per sample (COHORT)
    const int64_t* beg;
    const int64_t* end;
    const int32_t* samp;
    int64_t n;
    // per region (k_sg_regions): decoded range, first block, its first base is N, the start of the N run it ends in (-1: none)
    int64_t *rd0, *rd1, *rb0, *rhead, *rtail;
    int64_t *items, *ioff;      // n + 1: work items per region, their exclusive prefix (ioff[n] = all)
    int64_t W;                  // waves of k_sg_blocks
    int64_t *wcnt, *woff;       // W, W + 1: segment starts per wave, their exclusive prefix (woff[W] = all)
    int64_t* off;               // n + 1: the regions' offsets (the write)
    sccg_segment* seg;
    int64_t cap;                // segments seg holds
};

template <bool COHORT>
__device__ __forceinline__ const DcFetchSrc& sg_src(const SgArgs& A, int64_t i) {
    if (COHORT) return A.tab[__builtin_amdgcn_readfirstlane(A.samp[i])].S;
    return A.E.S;
}

template <bool COHORT>
__global__ __launch_bounds__(SCCG_BLOCK) void k_sg_regions(const SgArgs A) {
    const int64_t i = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const DcFetchSrc& S = COHORT ? A.tab[A.samp[i]].S : A.E.S;
    const DcRuns& N = S.nr;
    const int64_t j0 = A.beg[i], j1 = A.end[i];
    int64_t d0 = 0, d1 = 0, b0 = 0, nb = 0, head = 0, tail = -1;
    if (j1 > j0) {
        const int64_t r0 = run_end_after(N, j0), r1 = run_end_after(N, j1), rl = run_end_after(N, j1 - 1);
        head = r0 < N.n && N.start[r0] <= j0;
        d0 = j0 - (r0 < N.n ? N.cum[r0] + (N.start[r0] <= j0 ? j0 - N.start[r0] : 0) : run_cum(N, N.n));
        d1 = j1 - (r1 < N.n ? N.cum[r1] + (N.start[r1] <= j1 ? j1 - N.start[r1] : 0) : run_cum(N, N.n));
        if (rl < N.n && N.start[rl] <= j1 - 1) {   // the touching runs put in at decoded offset d1, clipped
            const int64_t at = d1 + run_cum(N, run_key_first<false>(N, d1));
            tail = at > j0 ? at : j0;
        }
        if (d1 > d0) {   // record blocks holding decoded bytes d0 and d1 - 1 (a block's bytes: [boff[b], boff[b + 1]))
            const int64_t nblk = (S.nrec + TK_B - 1) / TK_B;
            b0 = boff_first<true>(S.boff, 1, nblk, d0) - 1;
            nb = boff_first<false>(S.boff, b0 + 1, nblk, d1) - b0;
        }
    }
    A.rd0[i] = d0;
    A.rd1[i] = d1;
    A.rb0[i] = b0;
    A.rhead[i] = head;
    A.rtail[i] = tail;
    A.items[i] = nb + 1;
}

// out[k] = in[0] + .. + in[k - 1], k <= m: one block, SCCG_BLOCK * SG_SCAN_PER entries a round
__global__ __launch_bounds__(SCCG_BLOCK) void k_sg_scan(const int64_t* __restrict__ in, int64_t* __restrict__ out, int64_t m) {
    __shared__ int64_t tmp[5];
    int64_t carry = 0;
    for (int64_t base = 0; base < m; base += SCCG_BLOCK * SG_SCAN_PER) {
        const int64_t k0 = base + (int64_t)threadIdx.x * SG_SCAN_PER;
        int64_t v[SG_SCAN_PER], s = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < SG_SCAN_PER; q++) {
            v[q] = k0 + q < m ? in[k0 + q] : 0;
            s += v[q];
        }
        int64_t ex = block_excl_add(s, tmp, &tot) + carry;
#pragma unroll
        for (int q = 0; q < SG_SCAN_PER; q++) {
            if (k0 + q < m) out[k0 + q] = ex;
            ex += v[q];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) out[m] = carry;
}

// A lane's element of a record block: decoded offset, running p (a token's R' position), bases produced
struct SgElem {
    int64_t o, p, l;
    bool tok;
};
// k_tok_fill2's parse of block b (st: the wave's 2 * TK_B staging bytes)
__device__ __forceinline__ SgElem sg_parse(const DcFetchSrc& S, int64_t b, uint8_t* st) {
    const int lane = lane_id();
    const uint8_t* __restrict__ rec = S.rec;
    const int64_t n = S.nrec, rb = b * TK_B, ri = rb + lane;
    const uint8_t c = ri < n ? rec[ri] : (uint8_t)',';
    wave_sync();   // (the staged bytes of the block before are no longer read)
    st[lane] = c;
    st[TK_B + lane] = ri + TK_B < n ? rec[ri + TK_B] : (uint8_t)0;
    wave_sync();
    const RlView v{st - RL_BEHIND, rb, n, TK_B};   // v.at(q) = st[q - rb]
    const bool par = ri < n && (c == '(' || c == ')');
    const unsigned long long pm = __ballot(par) & ((1ull << lane) - 1ull);
    const bool inside = pm ? st[63 - __clzll((long long)pm)] == '(' : S.bin[b] != 0;
    int64_t contrib = 0, d = 0;
    bool tok = false;
    if (ri < n) {
        if (c == '(') {
            int64_t comma = -1, close = -1, l = 0;
            for (int64_t q = ri + 1; q < n && q < ri + 32; q++) {
                const uint8_t cq = v.at(q);
                if (cq == ',' && comma < 0) comma = q;
                if (cq == ')') { close = q; break; }
                if (cq == '(') break;
            }
            if (comma > 0 && close > comma && parse_int_v(v, ri + 1, comma, &d) && parse_int_v(v, comma + 1, close, &l) && l >= 0) {
                tok = true;
                contrib = l;
            }
        } else if (c == ')') {
            contrib = inside ? 0 : 1;
        } else if (!inside) {
            contrib = 1;
        }
    }
    const int64_t o = S.boff[b] + wave_incl_add(contrib) - contrib;
    const int64_t p = S.bdsum[b] + wave_incl_add(d);   // running p, this token included
    return SgElem{o, p, contrib, tok};
}
// the origin of an element's last base
__device__ __forceinline__ int64_t sg_last_origin(const DcFetchSrc& S, const SgElem& e) {
    return e.tok && e.l > 0 ? ref_pos(S.rm, e.p + e.l - 1) : -1;
}

// What a region's items share.
struct SgRegion {
    int64_t j0, d0, d1;
    bool head;   // its first base is N
};

// The segment starts of one element clipped to the region's [d0, d1) (not empty), in ascending position;
// prev: the origin of the decoded byte before the element (read only when the element starts behind d0).
// emit(k, pos, ref) takes the k-th; returns their number.  The events of a token are the groups of
// touching target N runs put in at its decoded offsets (key == offset) and the erased reference runs its
// R' interval crosses, merged by offset: the loop stops at those alone.
template <typename Emit>
__device__ __forceinline__ int sg_element(const DcFetchSrc& S, const SgElem& e, const SgRegion& G, int64_t prev, Emit&& emit) {
    const DcRuns& N = S.nr;
    const DcRuns& M = S.rm;
    const int64_t a = e.o > G.d0 ? e.o : G.d0, en = e.o + e.l < G.d1 ? e.o + e.l : G.d1;
    const int64_t va = e.p + (a - e.o);   // a token's R' position at decoded offset a
    int64_t mN = run_key_first<false>(N, a);
    int64_t mr = e.tok && M.n ? run_key_first<true>(M, va) : M.n;
    int cnt = 0;
    bool first = true;
    int64_t x = a;
    for (int64_t it = 0; it <= N.n + M.n && x < en; it++) {
        bool has_n = false;   // a target N run of nonzero length is put in just before decoded offset x
        int64_t gpos = 0;
        while (mN < N.n && run_key(N, mN) <= x) {
            if (N.len[mN] > 0 && !has_n) {
                has_n = true;
                gpos = N.start[mN];
            }
            mN++;
        }
        if (x == G.d0 && !G.head) has_n = false;   // (those runs end before the region)
        const int64_t v = va + (x - a);
        bool cut = false;
        if (e.tok)
            while (mr < M.n && run_key(M, mr) <= v) {
                mr++;
                cut = true;
            }
        const int64_t r = e.tok ? v + (M.n ? run_cum(M, mr) : 0) : -1;
        if (has_n) emit(cnt++, gpos > G.j0 ? gpos : G.j0, (int64_t)-2);
        const bool goes_on = e.tok ? prev >= 0 && r == prev + 1 : prev == -1;
        if (has_n || (first ? x == G.d0 || !goes_on : cut)) emit(cnt++, x + run_cum(N, mN), r);
        first = false;
        int64_t nx = en;
        if (mN < N.n && run_key(N, mN) < nx) nx = run_key(N, mN);
        if (e.tok && mr < M.n && a + (run_key(M, mr) - va) < nx) nx = a + (run_key(M, mr) - va);
        x = nx;
    }
    return cnt;
}

template <bool COHORT, bool WRITE>
__global__ __launch_bounds__(SCCG_BLOCK) void k_sg_blocks(const SgArgs A) {
    __shared__ uint8_t stg[WPB][2 * TK_B];
    const int64_t w = (int64_t)blockIdx.x * WPB + wave_in_block();
    if (w >= A.W) return;
    const int lane = lane_id();
    uint8_t* st = stg[wave_in_block()];
    const int64_t* __restrict__ ioff = A.ioff;
    const int64_t T = ioff[A.n];
    const int64_t per = T > A.W ? (T + A.W - 1) / A.W : 1;
    const int64_t it0 = w * per, it1 = it0 + per < T ? it0 + per : T;
    int64_t slot = WRITE ? A.woff[w] : 0;   // the next segment's slot (the count: from 0)
    if (it0 < it1) {
        // the region of the chunk's first item: the last i with ioff[i] <= it0 (every region has an item)
        int64_t i = boff_first<true>(ioff, 1, A.n + 1, it0) - 1;
        int64_t carry = NO_PREV;   // the origin of the last base produced before the next block
        SgRegion G{0, 0, 0, false};
        int64_t b0 = 0;
        for (int64_t it = it0; it < it1; it++) {
            if (it >= ioff[i + 1]) i++;
            const int64_t k = it - ioff[i], nb = ioff[i + 1] - ioff[i] - 1;
            if (WRITE && k == 0 && lane == 0) A.off[i] = slot;
            if (k == nb) {   // the tail item
                const int64_t tail = A.rtail[i];
                if (tail >= 0) {
                    if (WRITE && lane == 0 && slot < A.cap) {
                        A.seg[slot].pos = tail;
                        A.seg[slot].ref = -2;
                    }
                    slot++;
                }
                if (WRITE && i == A.n - 1 && lane == 0) A.off[A.n] = slot;
                continue;
            }
            const DcFetchSrc& S = sg_src<COHORT>(A, i);
            if (k == 0 || it == it0) {
                G = SgRegion{A.beg[i], A.rd0[i], A.rd1[i], A.rhead[i] != 0};
                b0 = A.rb0[i];
                carry = NO_PREV;
            }
            const int64_t b = b0 + k;
            if (k > 0 && it == it0 && S.boff[b] > G.d0) {
                // the chunk starts inside a region: the block that holds decoded byte boff[b] - 1 (the blocks
                // between it and b produce nothing), which lies at or behind b0 as boff[b0] <= d0
                const int64_t bp = boff_first<false>(S.boff, b0 + 1, b, S.boff[b]) - 1;
                const SgElem q = sg_parse(S, bp, st);
                const int64_t lo = sg_last_origin(S, q);
                const unsigned long long cm = __ballot(q.l > 0);
                if (cm) carry = readlane64(lo, 63 - __clzll((long long)cm));
            }
            const SgElem e = sg_parse(S, b, st);
            const int64_t lo = sg_last_origin(S, e);
            const unsigned long long cm = __ballot(e.l > 0);
            const unsigned long long below = cm & ((1ull << lane) - 1ull);
            const int64_t lo_before = __shfl(lo, below ? 63 - __clzll((long long)below) : lane, 64);
            const int64_t prev = below ? lo_before : carry;
            const bool in = e.l > 0 && e.o < G.d1 && e.o + e.l > G.d0;
            const int cnt = in ? sg_element(S, e, G, prev, [](int, int64_t, int64_t) {}) : 0;
            const int incl = (int)wave_incl_add_dpp((uint32_t)cnt);
            if (WRITE && cnt) {
                const int64_t at = slot + incl - cnt;
                sccg_segment* seg = A.seg;
                const int64_t cap = A.cap;
                sg_element(S, e, G, prev, [=](int q, int64_t pos, int64_t ref) {
                    if (at + q < cap) {
                        seg[at + q].pos = pos;
                        seg[at + q].ref = ref;
                    }
                });
            }
            slot += __builtin_amdgcn_readlane(incl, 63);
            if (cm) carry = readlane64(lo, 63 - __clzll((long long)cm));
        }
    }
    if (!WRITE && lane == 0) A.wcnt[w] = slot;
}

// (the total is read here, not passed: the launch is queued before the host knows it; a total beyond the
// capacity fails the call, and nothing beyond the capacity is read or written)
__global__ __launch_bounds__(SCCG_BLOCK) void k_sg_len(const SgArgs A) {
    const int64_t total = A.woff[A.W], m = total < A.cap ? total : A.cap;
    for (int64_t k = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x; k < m; k += (int64_t)gridDim.x * SCCG_BLOCK) {
        const int64_t i = boff_first<true>(A.off, 1, A.n + 1, k) - 1;   // the last region with off[i] <= k: the one that is not empty
        const int64_t next = k + 1 >= A.off[i + 1] ? A.end[i] : k + 1 < m ? A.seg[k + 1].pos : A.seg[k].pos;
        A.seg[k].len = next - A.seg[k].pos;
    }
}

int64_t sg_waves(const SgCall& c) {
    int64_t w = c.bound_items < 1 ? 1 : c.bound_items > SG_WAVES ? SG_WAVES : c.bound_items;
    return (w + WPB - 1) / WPB * WPB;
}

SgArgs sg_args(const SgCall& c) {
    SgArgs A{};
    if (c.src) A.E = DcCohortEntry{*c.src, c.src->nr.n, c.src->lr.n, c.src->nr.total};
    A.tab = c.d_tab;
    A.beg = c.d_beg;
    A.end = c.d_end;
    A.samp = c.d_samp;
    A.n = c.nreg;
    const int64_t n = c.nreg;
    int64_t* p = c.d_scratch;
    A.rd0 = p; p += n;
    A.rd1 = p; p += n;
    A.rb0 = p; p += n;
    A.rhead = p; p += n;
    A.rtail = p; p += n;
    A.items = p; p += n + 1;
    A.ioff = p; p += n + 1;
    A.off = p; p += n + 1;
    A.W = sg_waves(c);
    A.wcnt = p; p += SG_WAVES;
    A.woff = p; p += SG_WAVES + 1;
    return A;
}

}  // namespace

int64_t sg_scratch_words(int64_t nreg) { return 8 * nreg + 3 + 2 * SG_WAVES + 1; }

const int64_t* sg_total_slot(const SgCall& c) {
    const SgArgs A = sg_args(c);
    return A.woff + A.W;
}

int sg_scan(const int64_t* in, int64_t* out, int64_t m, hipStream_t s) {
    PROF_LAUNCH(PROF_FETCH, s, k_sg_scan, dim3(1), dim3(SCCG_BLOCK), 0, s, in, out, m);
    SCCG_HIP(hipGetLastError());
    return 0;
}

int sg_count(const SgCall& c, hipStream_t s) {
    if (c.nreg <= 0) return SCCG_E_INVALID;
    const SgArgs A = sg_args(c);
    const dim3 blk(SCCG_BLOCK);
    void (*const regions)(SgArgs) = c.src ? k_sg_regions<false> : k_sg_regions<true>;
    void (*const blocks)(SgArgs) = c.src ? k_sg_blocks<false, false> : k_sg_blocks<true, false>;
    PROF_LAUNCH(PROF_FETCH, s, regions, dim3(grid_for(A.n, SCCG_BLOCK)), blk, 0, s, A);
    if (const int rc = sg_scan(A.items, A.ioff, A.n, s)) return rc;
    PROF_LAUNCH(PROF_FETCH, s, blocks, dim3((unsigned)(A.W / WPB)), blk, 0, s, A);
    return sg_scan(A.wcnt, A.woff, A.W, s);
}

int sg_write(const SgCall& c, int64_t cap, int64_t* d_off, sccg_segment* d_seg, hipStream_t s) {
    if (c.nreg <= 0 || cap < 0) return SCCG_E_INVALID;
    SgArgs A = sg_args(c);
    if (d_off) A.off = d_off;
    A.seg = d_seg;
    A.cap = cap;
    const dim3 blk(SCCG_BLOCK);
    void (*const blocks)(SgArgs) = c.src ? k_sg_blocks<false, true> : k_sg_blocks<true, true>;
    PROF_LAUNCH(PROF_FETCH, s, blocks, dim3((unsigned)(A.W / WPB)), blk, 0, s, A);
    const int64_t len_blocks = (cap + SCCG_BLOCK - 1) / SCCG_BLOCK;
    PROF_LAUNCH(PROF_FETCH, s, k_sg_len, dim3((unsigned)(len_blocks < 1 ? 1 : len_blocks > SG_LEN_BLOCKS ? SG_LEN_BLOCKS : len_blocks)), blk,
                0, s, A);
    SCCG_HIP(hipGetLastError());
    return 0;
}
