// lift.hip -- reference intervals onto a sample, run-length coded: the segments call mirrored onto the
// reference axis.
//
// With pos(r) what locate (locate.hip: lc_one) returns for reference position r, a block of interval
// [r0, r1) is a maximal stretch whose bases continue each other: sequence positions ascending by one, or
// all without a copy (-1), or all of one erased run of 'N' (-2).  Inside one elementary interval of the
// locate index the first covering token is constant, so pos is linear there but for the target's N runs
// put into that token; an erased run of R lies between two R' positions.  The work is in proportion to
// the elementary intervals and runs under the query -- never to its bases:
//   k_lf_intervals  an interval per lane: both ends R -> R' over the erased runs ([v0, v1), whether the
//                   first base lies in one), the first and last elementary interval by two searches of
//                   ep.  Interval i gets leaves + 1 work items: its elementary intervals (the pseudo-leaf
//                   before ep[0] is leaf -1), then a tail item (the erased run the interval ends in; it
//                   also closes an interval without leaves).
//   sg_scan         (segments.hip) the exclusive prefix of the items: the flat work space; later of the
//                   waves' counts.
//   k_lf_items      W waves share the flat space in equal consecutive chunks, an item per lane.  An item
//                   is one leaf clipped to [v0, v1): the first token over it from the leaf and its
//                   ancestors (lc_one's independent loads), the same for the leaf before it when the item
//                   starts on the leaf's first base -- the block goes on there if pos does -- and the cuts
//                   inside by one search of the target's run keys and one of the erased runs', then a
//                   merge of the runs found.  An erased run belongs to the item that holds the R' position
//                   behind it, or to the tail item when that is v1.  <false> leaves the wave's count,
//                   <true> runs again from the scanned counts and stores {ref, pos} of the k-th start at
//                   slot k, and the intervals' offsets.
//   k_lf_len        a block per lane: len = the next start of the same interval, or its end, minus ref.
// Nothing walks bases, every loop is bounded by a data size or a fixed step count, no wave waits for
// another, plain vector stores only.
#include "internal.h"
#include "lift.h"
#include "segments.h"

namespace {

constexpr int WPB = SCCG_BLOCK / 64;
constexpr int LF_STEPS = 64;       // bound of every halving search here (< 2^63 entries end sooner)
constexpr int LF_LEVELS = 36;      // tree nodes read per leaf (locate.hip's LC_LEVELS)
constexpr int LF_WAVES = 4096;     // the most waves that share the flat space
constexpr int LF_LEN_BLOCKS = 2048;   // the most blocks of k_lf_len (they stride over the blocks)
constexpr int64_t LF_FAR = INT64_MAX;

__device__ __forceinline__ int64_t run_key(const DcRuns& M, int64_t m) { return (int64_t)M.start[m] - M.cum[m]; }
// the run bases before run m (m == M.n: all of them)
__device__ __forceinline__ int64_t run_cum(const DcRuns& M, int64_t m) { return m < M.n ? M.cum[m] : (M.n ? M.total : 0); }
// first m with key(m) >= v (GT: > v); the keys ascend
template <bool GT>
__device__ __forceinline__ int64_t run_key_first(const DcRuns& M, int64_t v) {
    int64_t a = 0, b = M.n;
    for (int it = 0; it < LF_STEPS && a < b; it++) {
        const int64_t m = (a + b) >> 1;
        const int64_t k = run_key(M, m);
        if (GT ? k > v : k >= v) b = m; else a = m + 1;
    }
    return a;
}
// first run ending after position r (of the runs' own axis)
__device__ __forceinline__ int64_t run_end_after(const DcRuns& M, int64_t r) {
    int64_t a = 0, b = M.n;
    for (int it = 0; it < LF_STEPS && a < b; it++) {
        const int64_t m = (a + b) >> 1;
        if ((int64_t)M.start[m] + M.len[m] > r) b = m; else a = m + 1;
    }
    return a;
}
// first k in [0, ne) with ep[k] >= v (GT: > v), ne if none
template <bool GT>
__device__ __forceinline__ int64_t ep_first(const LcIndex& X, int64_t v) {
    int64_t a = 0, b = X.ne;
    for (int it = 0; it < LF_STEPS && a < b; it++) {
        const int64_t m = (a + b) >> 1;
        if (GT ? (int64_t)X.ep[m] > v : (int64_t)X.ep[m] >= v) b = m; else a = m + 1;
    }
    return a;
}
// first m in [a, b) with p[m] > d, b if none
__device__ __forceinline__ int64_t i64_after(const int64_t* __restrict__ p, int64_t a, int64_t b, int64_t d) {
    for (int it = 0; it < LF_STEPS && a < b; it++) {
        const int64_t m = (a + b) >> 1;
        if (p[m] > d) b = m; else a = m + 1;
    }
    return a;
}

struct LfArgs {
    LcSrc S;             // the reader's source (!COHORT)
    const LcSrc* tab;    // one entry per sample (COHORT)
    const int64_t* beg;
    const int64_t* end;
    const int32_t* samp;
    int64_t n;
    // per interval (k_lf_intervals): its R' range, its first leaf (-1: the pseudo-leaf), its first base lies in an erased run
    int64_t *rv0, *rv1, *rk0, *rhead;
    int64_t *items, *ioff;      // n + 1: work items per interval, their exclusive prefix (ioff[n] = all)
    int64_t W;                  // waves of k_lf_items
    int64_t *wcnt, *woff;       // W, W + 1: block starts per wave, their exclusive prefix (woff[W] = all)
    int64_t* off;               // n + 1: the intervals' offsets (the write)
    sccg_lift_block* blk;
    int64_t cap;                // blocks blk holds
};

// the non-erased positions of R before x: x's place in R' (an x inside an erased run: the run's)
__device__ __forceinline__ int64_t lf_rprime(const DcRuns& M, int64_t x, bool* inside) {
    const int64_t a = run_end_after(M, x);
    const bool in = a < M.n && (int64_t)M.start[a] <= x;
    *inside = in;
    return (in ? (int64_t)M.start[a] : x) - run_cum(M, a);
}

template <bool COHORT>
__global__ __launch_bounds__(SCCG_BLOCK) void k_lf_intervals(const LfArgs A) {
    const int64_t i = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const LcSrc& S = COHORT ? A.tab[A.samp[i]] : A.S;
    const int64_t r0 = A.beg[i], r1 = A.end[i];
    int64_t v0 = 0, v1 = 0, k0 = 0, nl = 0;
    bool head = false, at_end = false;
    if (r1 > r0) {
        v0 = lf_rprime(S.rm, r0, &head);
        v1 = lf_rprime(S.rm, r1, &at_end);
        if (v1 > v0) {   // leaves holding R' positions v0 and v1 - 1 (leaf k: [ep[k], ep[k + 1]))
            k0 = ep_first<true>(S.ix, v0) - 1;
            nl = ep_first<false>(S.ix, v1) - k0;
        }
    }
    A.rv0[i] = v0;
    A.rv1[i] = v1;
    A.rk0[i] = k0;
    A.rhead[i] = head;
    A.items[i] = nl + 1;
}

// The first token in record order over leaf k: its R' start and decoded offset; false when nothing covers it.
__device__ __forceinline__ bool lf_first_token(const LcIndex& X, int64_t k, int64_t* tp, int64_t* to) {
    if (k < 0 || k >= X.ne || X.cover[k] <= 0) return false;
    uint32_t first = 0xffffffffu;
    const int64_t leaf = k + X.ne;
    for (int it = 0; it < LF_LEVELS && (leaf >> it) >= 1; it += 4) {   // (lc_one's four independent loads a round)
        uint32_t t[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t x = leaf >> (it + u);
            t[u] = X.tree[x ? x : 1];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) first = t[u] < first ? t[u] : first;
    }
    if ((int64_t)first >= X.nt) return false;   // (never with cover > 0)
    *tp = X.tp[first];
    *to = X.to[first];
    return true;
}

// What an interval's items share.
struct LfInterval {
    int64_t r0, r1, v0, v1;
    bool head;   // r0 lies in an erased run
};

// The block starts of leaf k clipped to [v0, v1) (not empty there), in ascending reference position;
// emit(q, ref, pos) takes the q-th; returns their number.  The events inside the leaf are the erased runs
// of R before its R' positions (key == position) and the groups of target N runs put into its first
// token (key == decoded offset), merged by R' position: the loop stops at those alone.
template <typename Emit>
__device__ __forceinline__ int lf_leaf(const LcSrc& S, const LfInterval& G, int64_t k, Emit&& emit) {
    const LcIndex& X = S.ix;
    const DcRuns& N = S.nr;
    const DcRuns& M = S.rm;
    const int64_t lo = k >= 0 ? (int64_t)X.ep[k] : 0, hi = k + 1 < X.ne ? (int64_t)X.ep[k + 1] : LF_FAR;
    const int64_t a = lo > G.v0 ? lo : G.v0, b = hi < G.v1 ? hi : G.v1;
    int64_t tp = 0, to = 0;
    const bool cov = lf_first_token(X, k, &tp, &to);
    const int64_t da = to + (a - tp);   // the decoded offset of R' position a
    int64_t mN = cov ? run_key_first<true>(N, da) : N.n;
    int64_t mr = run_key_first<false>(M, a);
    bool starts = true;   // a opens a block: the interval's first base, or pos does not go on from a - 1
    if (a > G.v0) {
        int64_t ptp = 0, pto = 0;
        int64_t pp = -1;
        if (lf_first_token(X, k - 1, &ptp, &pto)) {
            const int64_t pd = pto + (a - 1 - ptp);
            pp = pd + run_cum(N, run_key_first<true>(N, pd));
        }
        const int64_t p = cov ? da + run_cum(N, mN) : -1;
        starts = pp >= 0 ? p != pp + 1 : p != -1;
    } else if (!G.head && mr < M.n && run_key(M, mr) == a) {
        mr++;   // (that run ends before the interval)
    }
    int cnt = 0;
    int64_t x = a;
    for (int64_t it = 0; it <= N.n + M.n && x < b; it++) {
        const bool erased = mr < M.n && run_key(M, mr) == x;
        if (erased) {
            const int64_t at = M.start[mr];
            emit(cnt++, at > G.r0 ? at : G.r0, (int64_t)-2);
            mr++;
        }
        bool put_in = false;   // target N of nonzero length is put in just before x's copy
        if (cov && x > a)
            while (mN < N.n && run_key(N, mN) <= da + (x - a)) {
                put_in = put_in || N.len[mN] > 0;
                mN++;
            }
        if (erased || (x == a ? starts : put_in)) emit(cnt++, x + run_cum(M, mr), cov ? da + (x - a) + run_cum(N, mN) : (int64_t)-1);
        int64_t nx = b;
        if (mr < M.n && run_key(M, mr) < nx) nx = run_key(M, mr);
        if (cov && mN < N.n && run_key(N, mN) - da < nx - a) nx = a + (run_key(N, mN) - da);
        x = nx;
    }
    return cnt;
}

// The tail item: the erased run the interval ends in (the R' position behind it is v1, in no leaf of
// the interval), clipped.
template <typename Emit>
__device__ __forceinline__ int lf_tail(const LcSrc& S, const LfInterval& G, Emit&& emit) {
    const DcRuns& M = S.rm;
    if (G.r1 <= G.r0) return 0;
    const int64_t m = run_key_first<false>(M, G.v1);
    if (m >= M.n || run_key(M, m) != G.v1) return 0;
    const int64_t at = M.start[m];
    if (at >= G.r1 || at + M.len[m] <= G.r0) return 0;
    emit(0, at > G.r0 ? at : G.r0, (int64_t)-2);
    return 1;
}

template <bool COHORT, bool WRITE>
__global__ __launch_bounds__(SCCG_BLOCK) void k_lf_items(const LfArgs A) {
    const int64_t w = (int64_t)blockIdx.x * WPB + wave_in_block();
    if (w >= A.W) return;
    const int lane = lane_id();
    const int64_t* __restrict__ ioff = A.ioff;
    const int64_t T = ioff[A.n];
    const int64_t per = ((T + A.W - 1) / A.W + 63) / 64 * 64;   // whole rounds of 64 lanes
    const int64_t it0 = w * per, it1 = it0 + per < T ? it0 + per : T;
    int64_t slot = WRITE ? A.woff[w] : 0;   // the next block's slot (the count: from 0)
    for (int64_t base = it0; base < it1; base += 64) {
        const int64_t it = base + lane;
        const bool active = it < it1;
        int64_t i = 0, k = 0, nl = 0;
        LfInterval G{0, 0, 0, 0, false};
        int cnt = 0;
        if (active) {
            i = i64_after(ioff, 1, A.n + 1, it) - 1;   // the last i with ioff[i] <= it (every interval has an item)
            k = it - ioff[i];
            nl = ioff[i + 1] - ioff[i] - 1;
            G = LfInterval{A.beg[i], A.end[i], A.rv0[i], A.rv1[i], A.rhead[i] != 0};
            const LcSrc& S = COHORT ? A.tab[A.samp[i]] : A.S;
            const auto none = [](int, int64_t, int64_t) {};
            cnt = k == nl ? lf_tail(S, G, none) : lf_leaf(S, G, A.rk0[i] + k, none);
        }
        const int incl = (int)wave_incl_add_dpp((uint32_t)cnt);
        if (WRITE && active) {
            const int64_t at = slot + incl - cnt;
            if (k == 0) A.off[i] = at;
            if (k == nl && i == A.n - 1) A.off[A.n] = at + cnt;
            if (cnt) {
                const LcSrc& S = COHORT ? A.tab[A.samp[i]] : A.S;
                sccg_lift_block* blk = A.blk;
                const int64_t cap = A.cap;
                const auto store = [=](int q, int64_t ref, int64_t pos) {
                    if (at + q < cap) {
                        blk[at + q].ref = ref;
                        blk[at + q].pos = pos;
                    }
                };
                if (k == nl) lf_tail(S, G, store); else lf_leaf(S, G, A.rk0[i] + k, store);
            }
        }
        slot += __builtin_amdgcn_readlane(incl, 63);
    }
    if (!WRITE && lane == 0) A.wcnt[w] = slot;
}

// (the total is read here, not passed: the launch is queued before the host knows it; a total beyond the
// capacity fails the call, and nothing beyond the capacity is read or written)
__global__ __launch_bounds__(SCCG_BLOCK) void k_lf_len(const LfArgs A) {
    const int64_t total = A.woff[A.W], m = total < A.cap ? total : A.cap;
    for (int64_t k = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x; k < m; k += (int64_t)gridDim.x * SCCG_BLOCK) {
        const int64_t i = i64_after(A.off, 1, A.n + 1, k) - 1;   // the last interval with off[i] <= k: the one that is not empty
        const int64_t next = k + 1 >= A.off[i + 1] ? A.end[i] : k + 1 < m ? A.blk[k + 1].ref : A.blk[k].ref;
        A.blk[k].len = next - A.blk[k].ref;
    }
}

int64_t lf_waves(const LfCall& c) {
    const int64_t rounds = (c.bound_items + 63) / 64;
    const int64_t w = rounds < 1 ? 1 : rounds > LF_WAVES ? LF_WAVES : rounds;
    return (w + WPB - 1) / WPB * WPB;
}

LfArgs lf_args(const LfCall& c) {
    LfArgs A{};
    if (c.src) A.S = *c.src;
    A.tab = c.d_tab;
    A.beg = c.d_beg;
    A.end = c.d_end;
    A.samp = c.d_samp;
    A.n = c.nreg;
    const int64_t n = c.nreg;
    int64_t* p = c.d_scratch;
    A.rv0 = p; p += n;
    A.rv1 = p; p += n;
    A.rk0 = p; p += n;
    A.rhead = p; p += n;
    A.items = p; p += n + 1;
    A.ioff = p; p += n + 1;
    A.off = p; p += n + 1;
    A.W = lf_waves(c);
    A.wcnt = p; p += LF_WAVES;
    A.woff = p; p += LF_WAVES + 1;
    return A;
}

}  // namespace

int64_t lf_scratch_words(int64_t nreg) { return 7 * nreg + 3 + 2 * LF_WAVES + 1; }

const int64_t* lf_total_slot(const LfCall& c) {
    const LfArgs A = lf_args(c);
    return A.woff + A.W;
}

int lf_count(const LfCall& c, hipStream_t s) {
    if (c.nreg <= 0) return SCCG_E_INVALID;
    const LfArgs A = lf_args(c);
    const dim3 blk(SCCG_BLOCK);
    void (*const intervals)(LfArgs) = c.src ? k_lf_intervals<false> : k_lf_intervals<true>;
    void (*const items)(LfArgs) = c.src ? k_lf_items<false, false> : k_lf_items<true, false>;
    PROF_LAUNCH(PROF_FETCH, s, intervals, dim3(grid_for(A.n, SCCG_BLOCK)), blk, 0, s, A);
    if (const int rc = sg_scan(A.items, A.ioff, A.n, s)) return rc;
    PROF_LAUNCH(PROF_FETCH, s, items, dim3((unsigned)(A.W / WPB)), blk, 0, s, A);
    return sg_scan(A.wcnt, A.woff, A.W, s);
}

int lf_write(const LfCall& c, int64_t cap, int64_t* d_off, sccg_lift_block* d_blk, hipStream_t s) {
    if (c.nreg <= 0 || cap < 0) return SCCG_E_INVALID;
    LfArgs A = lf_args(c);
    if (d_off) A.off = d_off;
    A.blk = d_blk;
    A.cap = cap;
    const dim3 blk(SCCG_BLOCK);
    void (*const items)(LfArgs) = c.src ? k_lf_items<false, true> : k_lf_items<true, true>;
    PROF_LAUNCH(PROF_FETCH, s, items, dim3((unsigned)(A.W / WPB)), blk, 0, s, A);
    const int64_t len_blocks = (cap + SCCG_BLOCK - 1) / SCCG_BLOCK;
    PROF_LAUNCH(PROF_FETCH, s, k_lf_len, dim3((unsigned)(len_blocks < 1 ? 1 : len_blocks > LF_LEN_BLOCKS ? LF_LEN_BLOCKS : len_blocks)), blk,
                0, s, A);
    SCCG_HIP(hipGetLastError());
    return 0;
}
