// locate.hip -- reference position -> sequence position: the inverse of the origin fetch.
//
// "Where does reference position r lie in this sample?"  A token "(dp,l)" of the record line copies
// R' positions [p, p + l) to decoded offsets [o, o + l), so r is in the sample wherever a token's R'
// interval holds r's R' position: `copies` counts those tokens and `pos` is the smallest such
// sequence position, which is the first covering token in record order (decoded offsets ascend
// along the record line).
//
// The index (locate.h: LcIndex) answers both in O(log n) loads whatever the overlap -- a stuck walk
// piles thousands of short tokens onto one reference window, so nothing here walks a
// list of overlapping tokens:
//   tokens       the tokens of nonzero length in record order, by k_tok_fill2's parse of the record
//                blocks (count, scan, write)
//   endpoints    every start and end, radix-sorted (rocPRIM, header-only, this file alone) and
//                deduplicated (flag, scan, write): the elementary intervals
//   cover        +1 at a token's start, -1 at its end, prefix-summed: tokens over each interval
//   tree         implicit segment tree over the intervals; each token atomicMin's its index into the
//                canonical nodes of its leaf range
// A query is one binary search for the leaf, one load of its cover, and the minimum over the leaf's
// ancestors, whose addresses all follow from the leaf (independent loads, one round trip).
#include <rocprim/device/device_radix_sort.hpp>

#include "internal.h"
#include "locate.h"
#include "recparse.h"

namespace {

constexpr int WPB = SCCG_BLOCK / 64;
constexpr int TK_B = 64;          // record bytes per block (decomp.hip's block index)
constexpr int LC_LEVELS = 36;     // bound of the tree nodes read per query: a leaf and its ancestors
constexpr int LC_STEPS = 64;      // bound of every search loop here: a halving search over < 2^63 entries ends sooner

// One wave per record block, k_tok_fill2's parse: the tokens "(d,l)" that start in the block with
// their running p and decoded offset.  WRITE = false: cnt[b] = those with l > 0; WRITE = true: they
// go to slots off[b] .. in record order.
template <bool WRITE>
__global__ __launch_bounds__(SCCG_BLOCK) void k_lc_tokens(const uint8_t* __restrict__ s, int64_t n, const int64_t* __restrict__ bin,
                                                          const int64_t* __restrict__ boff, const int64_t* __restrict__ bdsum,
                                                          int64_t* __restrict__ cnt, const int64_t* __restrict__ off, int64_t nt,
                                                          uint32_t* __restrict__ tp, int32_t* __restrict__ tl,
                                                          int64_t* __restrict__ to) {
    __shared__ uint8_t stg[WPB][2 * TK_B];
    const int64_t b = (int64_t)blockIdx.x * WPB + wave_in_block();
    const int64_t base = b * TK_B;
    if (base >= n) return;
    const int lane = lane_id();
    const int64_t i = base + lane;
    uint8_t* st = stg[wave_in_block()];
    const uint8_t c = i < n ? s[i] : (uint8_t)',';
    st[lane] = c;
    st[TK_B + lane] = i + TK_B < n ? s[i + TK_B] : (uint8_t)0;
    wave_sync();
    const RlView v{st - RL_BEHIND, base, n, TK_B};   // v.at(q) = st[q - base]
    const bool par = i < n && (c == '(' || c == ')');
    const unsigned long long pm = __ballot(par) & ((1ull << lane) - 1ull);
    const bool inside = pm ? st[63 - __clzll((long long)pm)] == '(' : bin[b] != 0;
    int64_t contrib = 0, d = 0;
    bool tok = false;
    if (i < n) {
        if (c == '(') {
            int64_t comma = -1, close = -1, l = 0;
            for (int64_t q = i + 1; q < n && q < i + 32; q++) {
                const uint8_t cq = v.at(q);
                if (cq == ',' && comma < 0) comma = q;
                if (cq == ')') { close = q; break; }
                if (cq == '(') break;
            }
            if (comma > 0 && close > comma && parse_int_v(v, i + 1, comma, &d) && parse_int_v(v, comma + 1, close, &l) && l >= 0) {
                tok = true;
                contrib = l;
            }
        } else if (c == ')') {
            contrib = inside ? 0 : 1;
        } else if (!inside) {
            contrib = 1;
        }
    }
    const int64_t o = boff[b] + wave_incl_add(contrib) - contrib;
    const int64_t p = bdsum[b] + wave_incl_add(d);   // running p, this token included
    const unsigned long long tm = __ballot(tok && contrib > 0);
    if (!WRITE) {
        if (lane == 0) cnt[b] = __popcll(tm);
        return;
    }
    if (tok && contrib > 0) {
        const int64_t at = off[b] + __popcll(tm & ((1ull << lane) - 1ull));
        if (at < nt) {   // (the count and the write parse the same bytes: always)
            tp[at] = (uint32_t)p;
            tl[at] = (int32_t)contrib;
            to[at] = o;
        }
    }
}

__global__ __launch_bounds__(SCCG_BLOCK) void k_lc_keys(const uint32_t* __restrict__ tp, const int32_t* __restrict__ tl, int64_t nt,
                                                        uint32_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x;
    if (i >= nt) return;
    keys[2 * i] = tp[i];
    keys[2 * i + 1] = tp[i] + (uint32_t)tl[i];
}

__global__ __launch_bounds__(SCCG_BLOCK) void k_lc_flag(const uint32_t* __restrict__ sorted, int64_t n, int64_t* __restrict__ flag) {
    const int64_t k = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x;
    if (k < n) flag[k] = k == 0 || sorted[k] != sorted[k - 1];
}

__global__ __launch_bounds__(SCCG_BLOCK) void k_lc_unique(const uint32_t* __restrict__ sorted, const int64_t* __restrict__ rank,
                                                          int64_t n, int64_t ne, uint32_t* __restrict__ ep) {
    const int64_t k = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x;
    if (k >= n || !(k == 0 || sorted[k] != sorted[k - 1])) return;
    const int64_t at = rank[k];
    if (at >= 0 && at < ne) ep[at] = sorted[k];
}

// the entry of ep[0, ne) equal to v (every token start and end is one), ne when there is none
__device__ __forceinline__ int64_t ep_find(const uint32_t* __restrict__ ep, int64_t ne, uint32_t v) {
    int64_t a = 0, b = ne;   // first k with ep[k] >= v
    for (int it = 0; it < LC_STEPS && a < b; it++) {
        const int64_t m = (a + b) >> 1;
        if (ep[m] >= v) b = m; else a = m + 1;
    }
    return a < ne && ep[a] == v ? a : ne;
}

// one token per thread: +1 / -1 at its endpoints, its index onto the canonical nodes of its leaves
__global__ __launch_bounds__(SCCG_BLOCK) void k_lc_insert(const uint32_t* __restrict__ tp, const int32_t* __restrict__ tl, int64_t nt,
                                                          const uint32_t* __restrict__ ep, int64_t ne, int64_t* __restrict__ delta,
                                                          uint32_t* __restrict__ tree) {
    const int64_t i = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x;
    if (i >= nt) return;
    const int64_t a = ep_find(ep, ne, tp[i]), b = ep_find(ep, ne, tp[i] + (uint32_t)tl[i]);
    if (a >= b || b >= ne) return;   // (never: both endpoints are in ep and the end is the larger)
    atomicAdd(reinterpret_cast<unsigned long long*>(delta + a), 1ull);
    atomicAdd(reinterpret_cast<unsigned long long*>(delta + b), ~0ull);   // -1
    int64_t l = a + ne, r = b + ne;   // leaves [a, b): nodes < 2 ne
    for (int it = 0; it < LC_STEPS && l < r; it++, l >>= 1, r >>= 1) {
        if (l & 1) atomicMin(tree + l++, (uint32_t)i);
        if (r & 1) atomicMin(tree + --r, (uint32_t)i);
    }
}

__global__ __launch_bounds__(SCCG_BLOCK) void k_lc_cover(const int64_t* __restrict__ delta, const int64_t* __restrict__ excl, int64_t ne,
                                                         int32_t* __restrict__ cover) {
    const int64_t k = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x;
    if (k < ne) cover[k] = (int32_t)(excl[k] + delta[k]);
}

// first m in [0, M.n) with key(m) > v, key(m) = start[m] - cum[m] (map_seek's search, one lane's)
__device__ __forceinline__ int64_t runs_after(const DcRuns& M, int64_t v) {
    int64_t a = 0, b = M.n;
    for (int it = 0; it < LC_STEPS && a < b; it++) {
        const int64_t m = (a + b) >> 1;
        if ((int64_t)M.start[m] - M.cum[m] > v) b = m; else a = m + 1;
    }
    return a;
}

// One query on one lane: a chain of dependent loads, the next query's in the next lane.
__device__ __forceinline__ void lc_one(const LcSrc& S, int64_t r, int64_t& pos, int32_t& copies) {
    pos = SCCG_LOCATE_NONE;
    copies = 0;
    // 1. R -> R': inside an erased run of N, else minus the N before r
    int64_t v = r;
    if (S.rm.n > 0) {
        int64_t a = 0, b = S.rm.n;   // first run that ends after r
        for (int it = 0; it < LC_STEPS && a < b; it++) {
            const int64_t m = (a + b) >> 1;
            if ((int64_t)S.rm.start[m] + S.rm.len[m] > r) b = m; else a = m + 1;
        }
        if (a < S.rm.n && S.rm.start[a] <= r) {
            pos = SCCG_LOCATE_REF_N;
            return;
        }
        v = r - (a < S.rm.n ? S.rm.cum[a] : S.rm.total);
    }
    // 2. the elementary interval of v, its cover, the first token over it
    const LcIndex& X = S.ix;
    int64_t a = 0, b = X.ne;   // first k with ep[k] > v
    for (int it = 0; it < LC_STEPS && a < b; it++) {
        const int64_t m = (a + b) >> 1;
        if ((int64_t)X.ep[m] > v) b = m; else a = m + 1;
    }
    const int64_t k = a - 1;
    if (k < 0) return;
    const int32_t c = X.cover[k];
    if (c <= 0) return;
    // the leaf and its ancestors, four levels at a time: their addresses all follow from the leaf, so
    // the four loads of a round wait for nothing; past the root the root is read again, which a
    // minimum does not mind.  (A leaf is below 2^33 -- ne <= 2 nt < 2^32 -- so LC_LEVELS bounds it.)
    uint32_t first = 0xffffffffu;
    const int64_t leaf = k + X.ne;
    for (int it = 0; it < LC_LEVELS && (leaf >> it) >= 1; it += 4) {
        uint32_t t[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t x = leaf >> (it + u);
            t[u] = X.tree[x ? x : 1];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) first = t[u] < first ? t[u] : first;
    }
    if ((int64_t)first >= X.nt) return;   // (never with cover > 0)
    // 3. inside the token, then decoded offset -> sequence position over the target's N runs
    const int64_t in = v - (int64_t)X.tp[first];
    if (in < 0) return;
    const int64_t d = X.to[first] + in;
    const int64_t m = runs_after(S.nr, d);
    pos = d + (m < S.nr.n ? S.nr.cum[m] : S.nr.total);
    copies = c;
}

struct LcArgs {
    LcSrc S;
    const LcSrc* tab;
    const int64_t* q;
    const int32_t* samp;
    int64_t n;
    int64_t* pos;
    int32_t* copies;
};

template <bool COHORT>
__global__ __launch_bounds__(SCCG_BLOCK) void k_locate(const LcArgs A) {
    const int64_t i = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    int64_t pos;
    int32_t copies;
    if (COHORT) lc_one(A.tab[A.samp[i]], A.q[i], pos, copies);
    else lc_one(A.S, A.q[i], pos, copies);
    A.pos[i] = pos;
    if (A.copies) A.copies[i] = copies;
}

}  // namespace

int lc_count_tokens(const DcFetchSrc& S, int64_t* d_cnt, int64_t* d_off, int64_t* d_nt, int64_t* d_partial, hipStream_t s) {
    const int64_t nblk = (S.nrec + TK_B - 1) / TK_B;
    if (nblk > 0) {
        hipLaunchKernelGGL(k_lc_tokens<false>, dim3(grid_for(nblk, WPB)), dim3(SCCG_BLOCK), 0, s, S.rec, S.nrec, S.bin, S.boff, S.bdsum,
                           d_cnt, nullptr, 0, nullptr, nullptr, nullptr);
        SCCG_HIP(hipGetLastError());
    }
    return dev_excl_sum(d_cnt, d_off, nblk, d_nt, d_partial, s);
}

size_t lc_sort_temp_bytes(int64_t nkeys) {
    size_t bytes = 0;
    const uint32_t* in = nullptr;
    uint32_t* out = nullptr;
    if (rocprim::radix_sort_keys(nullptr, bytes, in, out, (size_t)nkeys, 0u, 32u, (hipStream_t) nullptr) != hipSuccess) return 0;
    return bytes;
}

int lc_endpoints(const DcFetchSrc& S, const int64_t* d_off, int64_t nt, uint32_t* tp, int32_t* tl, int64_t* to, uint32_t* keys,
                 uint32_t* sorted, void* tmp, size_t tmp_bytes, int64_t* flag, int64_t* rank, int64_t* d_ne, int64_t* d_partial,
                 hipStream_t s) {
    const int64_t nblk = (S.nrec + TK_B - 1) / TK_B, nk = 2 * nt;
    hipLaunchKernelGGL(k_lc_tokens<true>, dim3(grid_for(nblk, WPB)), dim3(SCCG_BLOCK), 0, s, S.rec, S.nrec, S.bin, S.boff, S.bdsum,
                       nullptr, d_off, nt, tp, tl, to);
    hipLaunchKernelGGL(k_lc_keys, dim3(grid_for(nt, SCCG_BLOCK)), dim3(SCCG_BLOCK), 0, s, tp, tl, nt, keys);
    SCCG_HIP(hipGetLastError());
    SCCG_HIP(rocprim::radix_sort_keys(tmp, tmp_bytes, (const uint32_t*)keys, sorted, (size_t)nk, 0u, 32u, s));
    hipLaunchKernelGGL(k_lc_flag, dim3(grid_for(nk, SCCG_BLOCK)), dim3(SCCG_BLOCK), 0, s, sorted, nk, flag);
    SCCG_HIP(hipGetLastError());
    return dev_excl_sum(flag, rank, nk, d_ne, d_partial, s);
}

int lc_index(const uint32_t* tp, const int32_t* tl, int64_t nt, const uint32_t* sorted, const int64_t* rank, int64_t ne,
             uint32_t* ep, int32_t* cover, uint32_t* tree, int64_t* delta, int64_t* excl, int64_t* d_partial, hipStream_t s) {
    hipLaunchKernelGGL(k_lc_unique, dim3(grid_for(2 * nt, SCCG_BLOCK)), dim3(SCCG_BLOCK), 0, s, sorted, rank, 2 * nt, ne, ep);
    SCCG_HIP(hipGetLastError());
    // (delta may be the flags and excl the ranks the launch above has read: stream order)
    SCCG_HIP(hipMemsetAsync(delta, 0, (size_t)ne * sizeof(int64_t), s));
    SCCG_HIP(hipMemsetAsync(tree, 0xff, (size_t)(2 * ne) * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_lc_insert, dim3(grid_for(nt, SCCG_BLOCK)), dim3(SCCG_BLOCK), 0, s, tp, tl, nt, ep, ne, delta, tree);
    SCCG_HIP(hipGetLastError());
    const int rc = dev_excl_sum(delta, excl, ne, nullptr, d_partial, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_lc_cover, dim3(grid_for(ne, SCCG_BLOCK)), dim3(SCCG_BLOCK), 0, s, delta, excl, ne, cover);
    SCCG_HIP(hipGetLastError());
    return 0;
}

int lc_locate(const LcLocate& c, hipStream_t s) {
    if (c.n <= 0) return 0;
    LcArgs A{};
    if (c.src) A.S = *c.src;
    A.tab = c.d_tab;
    A.q = c.d_q;
    A.samp = c.d_samp;
    A.n = c.n;
    A.pos = c.d_pos;
    A.copies = c.d_copies;
    void (*const kernel)(LcArgs) = c.src ? k_locate<false> : k_locate<true>;
    PROF_LAUNCH(PROF_FETCH, s, kernel, dim3(grid_for(c.n, SCCG_BLOCK)), dim3(SCCG_BLOCK), 0, s, A);
    SCCG_HIP(hipGetLastError());
    return 0;
}
