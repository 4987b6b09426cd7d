// decomp.hip -- reconstruction of the target FASTA from the record text (decompression.cpp).
//
//   line split                  decompression.cpp:66-101
//   run-line parse              decompression.cpp:126-207 ("(d,len)" / "d," items, running start)
//   token decode                decompression.cpp:210-236 ("(dp,l)" -> ref[p, p+l), literals)
//   N insertion, lowercase      decompression.cpp:241-262
//   50-column output            decompression.cpp:266-274, :322
//
// All of it is data-parallel: item starts are found with a scan of "last parenthesis" positions,
// numbers are parsed one item per thread, running starts / absolute p are prefix sums, output
// offsets are prefix sums, and the final FASTA is written position-by-position with N and
// lowercase membership found by binary search over the (sorted, disjoint) run lists.
// Inputs the reference's own compressor can produce are handled exactly; text outside that
// grammar is reported as SCCG_E_PARSE instead of reproducing the reference's undefined paths.
//
// The grammar (tests/recgen.py states it in full and builds records at each of its edges):
//   integer      an optional sign and 1 to 10 digits, within int32 (std::stoi also takes leading
//                blanks, trailing junk and more digits: those are SCCG_E_PARSE here)
//   run line     "(d,l)" items of at most 25 bytes, l >= 0, a ',' after ')' consumed, and bare "d"
//                items (runs of one) followed by ',' or the line's end; any number of ',' between,
//                before and after them; starts (running sums of d) >= 0, ascending and disjoint,
//                ends within int32; the last N run ends within the sequence, lowercase runs may
//                pass its end (decompression.cpp:255-262 drops the part beyond)
//   record line  "(d,l)" tokens; every byte outside one is a literal, ',' digits and ')' included;
//                p (running sum of d) < 0 or p + l > |R'| is SCCG_E_RANGE
// Three classes of input follow: inside the grammar the result is the reference's, byte for byte;
// text the reference defines a result for but the grammar excludes (the stoi leniencies above,
// descending or overlapping lowercase runs, which it sorts) is SCCG_E_PARSE, never other bytes;
// what the reference fails on fails here with FORMAT, PARSE or RANGE -- PARSE from any line before
// RANGE, where the reference reports the first failure in reading order.
#include <cstdlib>

#include "internal.h"
#include "decomp.h"
#include "find.h"
#include "recparse.h"
#include "segments.h"

namespace {

__device__ __forceinline__ bool is_num(uint8_t c) { return (c >= '0' && c <= '9') || c == '-' || c == '+'; }

// stoi on [s, e): optional sign then digits, all of [s,e) consumed; returns false otherwise
__device__ __forceinline__ bool parse_int(const uint8_t* s, int64_t n, int64_t a, int64_t e, int64_t* v) {
    if (a >= e) return false;
    bool neg = false;
    if (s[a] == '-' || s[a] == '+') { neg = s[a] == '-'; a++; }
    if (a >= e || e - a > 10) return false;
    int64_t x = 0;
    for (int64_t i = a; i < e; i++) {
        const uint8_t c = s[i];
        if (c < '0' || c > '9') return false;
        x = x * 10 + (c - '0');
    }
    x = neg ? -x : x;
    if (x > INT32_MAX || x < INT32_MIN) return false;
    *v = x;
    (void)n;
    return true;
}

// every '\n' of the record text into nl[0, NL_CAP) in any order, their count in *cnt (a record
// file holds 2-3 of them; the caller falls back to ordered searches when there are more)
__global__ void k_newlines(const uint8_t* __restrict__ s, int64_t n, unsigned long long* __restrict__ cnt,
                           int64_t* __restrict__ nl) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (s[i] == '\n') {
            const unsigned long long k = atomicAdd(cnt, 1ull);
            if (k < (unsigned long long)DC_NL_CAP) nl[k] = i;
        }
}

// positions of '(' / ')' -> value i, else -1 (for a max-scan: last parenthesis at or before i)
__global__ void k_paren_pos(const uint8_t* __restrict__ s, int64_t n, int64_t* __restrict__ v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        v[i] = (s[i] == '(' || s[i] == ')') ? i : -1;
}

// ---------------------------------------------------------------------------------------------
// run lines: item start flags (exclusive max-scan `lp` = last paren strictly before i)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool run_item_start(const uint8_t* s, int64_t i, int64_t lp_excl) {
    const uint8_t c = s[i];
    if (c == '(') return true;
    if (!is_num(c)) return false;
    const bool inside = lp_excl >= 0 && s[lp_excl] == '(';
    return !inside && (i == 0 || !is_num(s[i - 1]));
}

__global__ void k_run_items_flag(const uint8_t* __restrict__ s, int64_t n, const int64_t* __restrict__ lp,
                                 int64_t* __restrict__ flag, int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bool st = run_item_start(s, i, lp[i]);
        flag[i] = st;
        // bytes outside any item must be ',' (a ')' closes a tuple)
        const uint8_t c = s[i];
        const bool inside = (lp[i] >= 0 && s[lp[i]] == '(') || c == '(' || c == ')';
        if (!inside && !is_num(c) && c != ',') atomicOr(err, 1);
    }
}

__global__ void k_run_items_parse(const uint8_t* __restrict__ s, int64_t n, const int64_t* __restrict__ lp,
                                  const int64_t* __restrict__ rank, int64_t* __restrict__ dlt,
                                  int32_t* __restrict__ len, int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!run_item_start(s, i, lp[i])) continue;
        const int64_t r = rank[i];
        int64_t d = 0, l = 1;
        bool ok;
        if (s[i] == '(') {
            int64_t comma = -1, close = -1;
            for (int64_t q = i + 1; q < n && q < i + 32; q++) {
                if (s[q] == ',' && comma < 0) comma = q;
                if (s[q] == ')') { close = q; break; }
                if (s[q] == '(') break;
            }
            ok = comma > 0 && close > comma && parse_int(s, n, i + 1, comma, &d) && parse_int(s, n, comma + 1, close, &l);
            // a ',' right after ')' is consumed by the reference parser (decompression.cpp:143-144)
        } else {
            int64_t e = i;
            while (e < n && is_num(s[e])) e++;
            ok = (e == n || s[e] == ',') && parse_int(s, n, i, e, &d);
        }
        // (a line of n bytes inside the grammar holds at most n / 2 + 1 items: dc_run_cap; text with
        // more item starts than that, "((((", is malformed and must not write past the lists)
        if (!ok || l < 0 || r >= n / 2 + 2) { atomicOr(err, 1); continue; }
        dlt[r] = d;
        len[r] = (int32_t)l;
    }
}

// ---------------------------------------------------------------------------------------------
// run lines, tiled: one wave per 1 KiB tile, 16 bytes per lane, the tile staged in LDS with the 32
// bytes before it and the 64 after it (every byte read of the parse is an LDS read; coalesced HBM
// loads once per pass).  A run line's parentheses only open "(d,len)" items of at most 25 bytes, so
// the "inside an item" state at a lane's first byte follows from the last parenthesis before it:
// in the lanes before it (a wave max-scan), else in the 32 bytes before the tile (text outside the
// compressor's grammar is flagged by the item parses either way).  Three launches per line instead
// of a parenthesis max-scan, an item-rank scan and three prefix sums (decompression.cpp:126-207 per
// item, running start, sorted).
// ---------------------------------------------------------------------------------------------
constexpr int RL_LANE = 8;   // (16: ~5 us slower on the chr1 reconstruction, more serial bytes per lane)
constexpr int RL_TILE = 64 * RL_LANE;   // (RL_BEHIND, RL_AHEAD, RlView, parse_int_v: recparse.h)
constexpr int RL_STAGE = RL_BEHIND + RL_TILE + RL_AHEAD;

template <int TILE>
__device__ __forceinline__ RlView rl_stage(const uint8_t* __restrict__ s, int64_t n, int64_t t0, uint8_t* st) {
    for (int k = lane_id(); k < RL_BEHIND + TILE + RL_AHEAD; k += 64) {
        const int64_t g = t0 - RL_BEHIND + k;
        st[k] = (g >= 0 && g < n) ? s[g] : (uint8_t)0;
    }
    wave_sync();
    return RlView{st, t0, n, TILE};
}

// one item at i (inside the tile): "(d,l)" or a bare "d" followed by ',' or the end
// (decompression.cpp:126-164); a bare number running past the staged bytes is not the compressor's
__device__ __forceinline__ bool rl_item(const RlView& v, int64_t i, int64_t* d, int64_t* l) {
    const int64_t n = v.n, lim = v.lim();
    *l = 1;
    if (v.at(i) == '(') {
        int64_t comma = -1, close = -1;
        for (int64_t q = i + 1; q < n && q < i + 32; q++) {
            const uint8_t c = v.at(q);
            if (c == ',' && comma < 0) comma = q;
            if (c == ')') { close = q; break; }
            if (c == '(') break;
        }
        return comma > 0 && close > comma && parse_int_v(v, i + 1, comma, d) && parse_int_v(v, comma + 1, close, l) &&
               *l >= 0;
    }
    int64_t e = i;
    while (e < n && e < lim && is_num(v.at(e))) e++;
    if (e == lim && e < n) return false;
    return (e == n || v.at(e) == ',') && parse_int_v(v, i, e, d);
}

// the "inside an item" state at the first byte a of this lane's `per` bytes
__device__ __forceinline__ bool rl_lane_inside(const RlView& v, int64_t a, int per) {
    const int lane = lane_id();
    int64_t last = -1;   // this lane's last parenthesis (2 * position + open), -1: none
    for (int64_t i = a; i < a + per && i < v.n; i++) {
        const uint8_t c = v.at(i);
        if (c == '(' || c == ')') last = 2 * i + (c == '(');
    }
    int64_t ex = __shfl_up(last, 1, 64);
    if (lane == 0) ex = -1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {   // exclusive max-scan over the lanes before
        const int64_t o = __shfl_up(ex, d, 64);
        if (lane >= d && o > ex) ex = o;
    }
    // before the tile: the last parenthesis among its RL_BEHIND preceding bytes
    const int64_t b = v.t0 - RL_BEHIND + (lane & (RL_BEHIND - 1));
    const bool par = lane < RL_BEHIND && b >= 0 && (v.at(b) == '(' || v.at(b) == ')');
    const unsigned long long pm = __ballot(par);
    bool tile_in = false;
    if (pm) tile_in = v.at(v.t0 - RL_BEHIND + (63 - __clzll((long long)pm))) == '(';
    return ex >= 0 ? (ex & 1) != 0 : tile_in;
}

struct RlLane {
    int64_t cnt, dsum, lsum, lastlen;   // items starting in the lane, their deltas, lengths, the last length (-1)
};

// walk the lane's bytes: item starts (in order) to f(i, d, l); byte-class errors to err
template <typename F>
__device__ __forceinline__ RlLane rl_lane(const RlView& v, int64_t a, bool inside, int32_t* err, F&& f) {
    RlLane r{0, 0, 0, -1};
    bool bad = false;
    uint8_t prev = a > 0 ? v.at(a - 1) : (uint8_t)',';
    for (int64_t i = a; i < a + RL_LANE && i < v.n; i++) {
        const uint8_t c = v.at(i);
        bool start = false;
        if (c == '(') { start = true; inside = true; }
        else if (c == ')') { inside = false; }
        else if (!inside) {
            if (is_num(c)) start = !(i > 0 && is_num(prev));
            else if (c != ',') bad = true;
        }
        if (start) {
            int64_t d = 0, l = 1;
            if (!rl_item(v, i, &d, &l)) bad = true;
            f(i, d, l, r);
            r.cnt++;
            r.dsum += d;
            r.lsum += l;
            r.lastlen = l;
        }
        prev = c;
    }
    if (bad && err) atomicOr(err, 1);
    return r;
}

// One launch set parses both run lines: tiles [0, j0.ntiles) are line 0's, the rest line 1's.
struct RlJob {
    const uint8_t* s;
    int64_t n, ntiles;
    int64_t* tsum;      // 4 per tile: pass-1 summaries, then their exclusive prefixes
    int32_t* start;
    int32_t* len;
    int64_t* cum;
    int64_t* d_count;   // [0] items, [1] total length
};
__device__ __forceinline__ const RlJob& rl_job(const RlJob& j0, const RlJob& j1, int64_t& t) {
    if (t < j0.ntiles) return j0;
    t -= j0.ntiles;
    return j1;
}

// pass 1: per tile (count, delta sum, length sum, last length) -> tsum[4 * t]
__global__ __launch_bounds__(256) void k_rl_tiles(RlJob j0, RlJob j1, int32_t* __restrict__ err) {
    __shared__ uint8_t stage[4][RL_STAGE];
    int64_t t = (int64_t)blockIdx.x * 4 + wave_in_block();
    if (t >= j0.ntiles + j1.ntiles) return;
    const RlJob& J = rl_job(j0, j1, t);
    const int64_t t0 = t * RL_TILE, n = J.n;
    const int lane = lane_id();
    const RlView v = rl_stage<RL_TILE>(J.s, n, t0, stage[wave_in_block()]);
    const int64_t a = t0 + (int64_t)lane * RL_LANE;
    const bool inside = rl_lane_inside(v, a, RL_LANE);
    const RlLane r = rl_lane(v, a, inside, err, [](int64_t, int64_t, int64_t, const RlLane&) {});
    const int64_t c = wave_sum(r.cnt), d = wave_sum(r.dsum), l = wave_sum(r.lsum);
    const unsigned long long hm = __ballot(r.cnt > 0);
    const int64_t last = hm ? __shfl(r.lastlen, 63 - __clzll((long long)hm), 64) : -1;
    int64_t* tsum = J.tsum;
    if (lane == 0) { tsum[4 * t] = c; tsum[4 * t + 1] = d; tsum[4 * t + 2] = l; tsum[4 * t + 3] = last; }
    // the lane's own totals for the write pass (after the 4 * ntiles summaries)
    int64_t* ld = tsum + 4 * J.ntiles + (t * 64 + lane) * 4;
    ld[0] = r.cnt; ld[1] = r.dsum; ld[2] = r.lsum; ld[3] = r.lastlen;
}

// pass 2 (one block): exclusive prefix over tiles of (count, deltas, lengths) and the last item
// length before each tile (-1: none); the totals -> d_count[0..1]
constexpr int RL_SCAN_T = 256;   // (a 1024-thread block waits for a whole CU beside a running strip)
constexpr int RL_SCAN_B = 8;     // tile summaries per batch of loads
__device__ __forceinline__ int64_t i64_of(int lo, int hi) { return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo); }
__global__ __launch_bounds__(RL_SCAN_T) void k_rl_scan(RlJob j0, RlJob j1) {   // block b: line b
    constexpr int NW = RL_SCAN_T / 64;
    __shared__ int64_t wc[NW], wd[NW], wl[NW], wlast[NW];
    const RlJob& J = blockIdx.x == 0 ? j0 : j1;
    const int64_t ntiles = J.ntiles;
    int64_t* tsum = J.tsum;
    int64_t* d_count = J.d_count;
    if (ntiles <= 0) {
        if (threadIdx.x == 0 && d_count) { d_count[0] = 0; d_count[1] = 0; }
        return;
    }
    const int tid = (int)threadIdx.x, lane = lane_id(), w = wave_in_block();
    const int64_t per = (ntiles + RL_SCAN_T - 1) / RL_SCAN_T, b0 = tid * per;
    const int64_t b1 = b0 + per < ntiles ? b0 + per : ntiles;
    // (RL_SCAN_B tiles' summaries loaded together: one tile at a time made this single-block pass
    // a chain of dependent HBM round trips, ~30 us on the chr1 reconstruction's critical path)
    int64_t c = 0, d = 0, l = 0, last = -1;
    for (int64_t t0 = b0; t0 < b1; t0 += RL_SCAN_B) {
        int4 q[RL_SCAN_B][2];
#pragma unroll
        for (int u = 0; u < RL_SCAN_B; u++)
            if (t0 + u < b1) {
                const int4* p4 = reinterpret_cast<const int4*>(tsum + 4 * (t0 + u));
                q[u][0] = p4[0];
                q[u][1] = p4[1];
            }
#pragma unroll
        for (int u = 0; u < RL_SCAN_B; u++)
            if (t0 + u < b1) {
                c += i64_of(q[u][0].x, q[u][0].y); d += i64_of(q[u][0].z, q[u][0].w); l += i64_of(q[u][1].x, q[u][1].y);
                const int64_t tl = i64_of(q[u][1].z, q[u][1].w);
                if (tl >= 0) last = tl;
            }
    }
    int64_t ic = c, id = d, il = l, ilast = last;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t xc = __shfl_up(ic, o, 64), xd = __shfl_up(id, o, 64), xl = __shfl_up(il, o, 64),
                      xlast = __shfl_up(ilast, o, 64);
        if (lane >= o) { ic += xc; id += xd; il += xl; if (ilast < 0) ilast = xlast; }
    }
    if (lane == 63) { wc[w] = ic; wd[w] = id; wl[w] = il; wlast[w] = ilast; }
    __syncthreads();
    int64_t pc = 0, pd = 0, pl = 0, plast = -1;
    for (int i = 0; i < w; i++) { pc += wc[i]; pd += wd[i]; pl += wl[i]; if (wlast[i] >= 0) plast = wlast[i]; }
    int64_t ec = pc + ic - c, ed = pd + id - d, el = pl + il - l;
    int64_t elast = __shfl_up(ilast, 1, 64);
    if (lane == 0 || elast < 0) elast = lane == 0 ? plast : (elast < 0 ? plast : elast);
    for (int64_t t0 = b0; t0 < b1; t0 += RL_SCAN_B) {
        int4 q[RL_SCAN_B][2];
#pragma unroll
        for (int u = 0; u < RL_SCAN_B; u++)
            if (t0 + u < b1) {
                const int4* p4 = reinterpret_cast<const int4*>(tsum + 4 * (t0 + u));
                q[u][0] = p4[0];
                q[u][1] = p4[1];
            }
#pragma unroll
        for (int u = 0; u < RL_SCAN_B; u++)
            if (t0 + u < b1) {
                const int64_t t = t0 + u;
                const int64_t tc = i64_of(q[u][0].x, q[u][0].y), td = i64_of(q[u][0].z, q[u][0].w);
                const int64_t tl = i64_of(q[u][1].x, q[u][1].y), tlast = i64_of(q[u][1].z, q[u][1].w);
                tsum[4 * t] = ec; tsum[4 * t + 1] = ed; tsum[4 * t + 2] = el; tsum[4 * t + 3] = elast;
                ec += tc; ed += td; el += tl;
                if (tlast >= 0) elast = tlast;
            }
    }
    if (tid == RL_SCAN_T - 1 && d_count) { d_count[0] = ec; d_count[1] = el; }
}

// pass 3: every item's start (running sum of deltas), length and the exclusive prefix of lengths;
// starts must be >= 0, ascending and disjoint, and end within int32 (k_run_finish's checks)
__global__ __launch_bounds__(256) void k_rl_write(RlJob j0, RlJob j1, int32_t* __restrict__ err) {
    __shared__ uint8_t stage[4][RL_STAGE];
    int64_t t = (int64_t)blockIdx.x * 4 + wave_in_block();
    if (t >= j0.ntiles + j1.ntiles) return;
    const RlJob& J = rl_job(j0, j1, t);
    const int64_t t0 = t * RL_TILE, n = J.n;
    const int64_t* tsum = J.tsum;
    int32_t* start = J.start;
    int32_t* len = J.len;
    int64_t* cum = J.cum;
    const int lane = lane_id();
    const RlView v = rl_stage<RL_TILE>(J.s, n, t0, stage[wave_in_block()]);
    const int64_t a = t0 + (int64_t)lane * RL_LANE;
    const bool inside = rl_lane_inside(v, a, RL_LANE);
    // the lane's totals (pass 1 kept them), then its exclusive prefixes over the wave
    const int64_t* ld = tsum + 4 * J.ntiles + (t * 64 + lane) * 4;
    const RlLane tot{ld[0], ld[1], ld[2], ld[3]};
    const int64_t ic = wave_incl_add(tot.cnt), id = wave_incl_add(tot.dsum), il = wave_incl_add(tot.lsum);
    // the last item length before this lane (in earlier lanes, else before the tile)
    const unsigned long long hm = __ballot(tot.cnt > 0) & ((1ull << lane) - 1ull);
    const int64_t prevlen = hm ? __shfl(tot.lastlen, 63 - __clzll((long long)hm), 64) : tsum[4 * t + 3];
    const int64_t rank0 = tsum[4 * t] + ic - tot.cnt;
    int64_t run_start = tsum[4 * t + 1] + id - tot.dsum;   // start of the last item before this lane's first
    int64_t run_cum = tsum[4 * t + 2] + il - tot.lsum;
    int64_t prev_end = rank0 > 0 ? run_start + (prevlen >= 0 ? prevlen : 0) : INT64_MIN;
    bool bad = false;
    // (the lists hold dc_run_cap(n) = n / 2 + 2 runs, more than a line inside the grammar can have;
    // every '(' counts as an item start, so malformed text such as "((((" has more: flagged by
    // pass 1, and nothing is written past the lists)
    const int64_t cap = n / 2 + 2;
    rl_lane(v, a, inside, nullptr, [&](int64_t, int64_t d, int64_t l, const RlLane& r) {
        const int64_t rank = rank0 + r.cnt;
        const int64_t st = run_start + d;
        if (st < 0 || st + l > INT32_MAX || (rank > 0 && st < prev_end) || rank >= cap) bad = true;
        if (rank < cap) {
            start[rank] = (int32_t)st;
            len[rank] = (int32_t)l;
            cum[rank] = run_cum;
        }
        run_start = st;
        run_cum += l;
        prev_end = st + l;
    });
    if (bad) atomicOr(err, 1);
}

// starts = inclusive prefix of deltas (exclusive scan + own delta); runs must be ascending & disjoint.
// Also the run lengths as int64 for the N-count prefix, 0 past the *d_nr parsed runs (the scans run
// to the capacity, so the host never waits for the count).
__global__ void k_run_finish(const int64_t* __restrict__ dex, const int64_t* __restrict__ dlt, const int32_t* __restrict__ len,
                             int64_t cap, const int64_t* __restrict__ d_nr, int32_t* __restrict__ start,
                             int64_t* __restrict__ len64, int32_t* __restrict__ err) {
    const int64_t nr = *d_nr;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < cap; r += (int64_t)gridDim.x * blockDim.x) {
        if (r >= nr) { len64[r] = 0; continue; }
        const int64_t st = dex[r] + dlt[r];
        const int64_t pst = r ? dex[r - 1] + dlt[r - 1] : INT64_MIN;
        const int64_t pend = r ? pst + len[r - 1] : 0;
        // (the formatter keeps run ends in int32: a run must also END within int32)
        if (st < 0 || st + (int64_t)len[r] > INT32_MAX || (r && st < pend)) atomicOr(err, 1);
        start[r] = (int32_t)st;
        len64[r] = len[r];
    }
}

// the last N run must end within the sequence: decoded length (*d_D) + N count (d_ncnt[1])
__global__ void k_n_check(const int32_t* __restrict__ ns, const int32_t* __restrict__ nl, const int64_t* __restrict__ d_ncnt,
                          const int64_t* __restrict__ d_D, int32_t* __restrict__ err) {
    const int64_t n = d_ncnt[0];
    // (a line that failed its parse may count more item starts than the lists hold: PARSE is
    // reported before this check's bit either way)
    if (*err & 1) return;
    if (threadIdx.x == 0 && n > 0 && (int64_t)ns[n - 1] + nl[n - 1] > *d_D + d_ncnt[1]) atomicOr(err, 4);
}

// ---------------------------------------------------------------------------------------------
// record line
// ---------------------------------------------------------------------------------------------
constexpr int WPB = 4;
// 16 bytes from any byte address: one global_load_dwordx4 (gfx950 runs in unaligned access mode)
__device__ __forceinline__ uint4 load16u(const uint8_t* __restrict__ p) {
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
// dst[0, l) = src[0, l) by one wave: bytes up to dst's next 16-byte boundary and after its last one
// one per lane, the rest 16 bytes per lane as aligned stores of (unaligned) 16-byte source loads.
// The source may be read up to 19 bytes past src + l (the reference buffers carry 64 bytes of slack).
constexpr int WC_DEPTH = 2;
__device__ __forceinline__ void wave_copy_body(uint4* __restrict__ d, const uint8_t* __restrict__ s0, int64_t nb, int64_t from,
                                               int lane);
__device__ __forceinline__ int64_t readlane64(int64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)(v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ void wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int64_t l, int lane) {
    const int64_t h = ((16 - ((uintptr_t)dst & 15)) & 15) < l ? ((16 - ((uintptr_t)dst & 15)) & 15) : l;
    const int64_t nb = (l - h) >> 4;
    const int64_t t0 = h + (nb << 4);
    if (lane < h) dst[lane] = src[lane];
    if (lane < l - t0) dst[t0 + lane] = src[t0 + lane];
    wave_copy_body(reinterpret_cast<uint4*>(dst + h), src + h, nb, 0, lane);
}

// 16-byte chunks [from, nb) of d = s0 (d 16-byte aligned)
__device__ __forceinline__ void wave_copy_body(uint4* __restrict__ d, const uint8_t* __restrict__ s0, int64_t nb, int64_t from,
                                               int lane) {
    // WC_DEPTH KiB of loads in flight per wave before the stores (one 1 KiB step at a time left the
    // fill bound by the bytes in flight: ~3 TB/s)
    for (int64_t c0 = from + lane; c0 < nb; c0 += 64 * WC_DEPTH) {
        uint4 v[WC_DEPTH];
#pragma unroll
        for (int u = 0; u < WC_DEPTH; u++) {
            const int64_t c = c0 + 64 * u;
            if (c < nb) v[u] = load16u(s0 + 16 * c);
        }
#pragma unroll
        for (int u = 0; u < WC_DEPTH; u++) {
            const int64_t c = c0 + 64 * u;
            if (c < nb) d[c] = v[u];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// record line, per 64-byte block (the usual path).  A token "(dp,l)" is at most 25 bytes, so the
// "inside a token" state at a block's first byte follows from the last parenthesis before it (the
// lanes before it in the 1 KiB tile, else the 32 bytes before the tile; rl_lane_inside).  Pass 1
// stores per block its state and its sums of output bytes (literal 1, token l) and token deltas;
// two exclusive scans over the blocks give every block's output offset and running p; the fill
// recomputes a block's bytes from those (decompression.cpp:210-236), with the range check of
// :223-229 (d_err bit 2) in the same pass.  (The per-byte arrays of the scan-based path -- last
// parenthesis, contribution, delta, their prefix sums: 40 B per record byte -- are gone.)
// ---------------------------------------------------------------------------------------------
constexpr int TK_B = 64;   // record bytes per block (one lane in pass 1, one wave in the fill)

__global__ __launch_bounds__(256) void k_tok_blocks(const uint8_t* __restrict__ s, int64_t n, int64_t* __restrict__ bin,
                                                    int64_t* __restrict__ bcontrib, int64_t* __restrict__ bdelta,
                                                    int32_t* __restrict__ err) {
    // one wave per 1 KiB tile (16 bytes per lane, staged in LDS); 4 lanes make one 64-byte block
    constexpr int TL = 16, TT = 64 * TL;
    __shared__ uint8_t stage[4][RL_BEHIND + TT + RL_AHEAD];
    const int64_t t = (int64_t)blockIdx.x * 4 + wave_in_block();
    const int64_t t0 = t * TT;
    if (t0 >= n) return;
    const int lane = lane_id();
    const RlView v = rl_stage<TT>(s, n, t0, stage[wave_in_block()]);
    const int64_t a = t0 + (int64_t)lane * TL;
    bool inside = rl_lane_inside(v, a, TL);
    const bool in0 = inside;
    int64_t cs = 0, ds = 0;
    bool bad = false;
    for (int64_t i = a; i < a + TL && i < n; i++) {
        const uint8_t c = v.at(i);
        if (c == '(') {
            int64_t comma = -1, close = -1, d = 0, l = 0;
            for (int64_t q = i + 1; q < n && q < i + 32; q++) {
                const uint8_t cq = v.at(q);
                if (cq == ',' && comma < 0) comma = q;
                if (cq == ')') { close = q; break; }
                if (cq == '(') break;
            }
            if (!(comma > 0 && close > comma && parse_int_v(v, i + 1, comma, &d) && parse_int_v(v, comma + 1, close, &l)) ||
                l < 0)
                bad = true;
            cs += l;
            ds += d;
            inside = true;
        } else if (c == ')') {
            cs += inside ? 0 : 1;   // a ')' outside a token is a literal (decompression.cpp:231-234)
            inside = false;
        } else if (!inside) {
            cs += 1;
        }
    }
    if (bad) atomicOr(err, 1);
    cs += __shfl_xor(cs, 1, 64);
    cs += __shfl_xor(cs, 2, 64);
    ds += __shfl_xor(ds, 1, 64);
    ds += __shfl_xor(ds, 2, 64);
    static_assert(4 * TL == TK_B, "four lanes per block");
    const int64_t b = t * (TT / TK_B) + (lane >> 2);
    if ((lane & 3) == 0 && b * TK_B < n) {
        bin[b] = in0;
        bcontrib[b] = cs;
        bdelta[b] = ds;
    }
}

// one wave per block: literals and token copies into dec at the block's offsets; tokens beyond
// the reference (p < 0 or p + l > |R'|, decompression.cpp:223-229) set d_err bit 2 and copy nothing.
// WRITE = false: the range check alone (no dec; a size query or an early error must report
// SCCG_E_RANGE exactly as the full decode would)
template <bool WRITE>
__global__ __launch_bounds__(SCCG_BLOCK) void k_tok_fill2(const uint8_t* __restrict__ s, int64_t n,
                                                          const int64_t* __restrict__ bin, const int64_t* __restrict__ boff,
                                                          const int64_t* __restrict__ bdsum, const int64_t* __restrict__ d_nref,
                                                          const uint8_t* __restrict__ R, uint8_t* __restrict__ dec,
                                                          int32_t* __restrict__ err, int64_t dcap) {
    __shared__ uint8_t stg[WPB][2 * TK_B];
    const int64_t b = (int64_t)blockIdx.x * WPB + wave_in_block();
    const int64_t base = b * TK_B;
    if (base >= n) return;
    const int lane = lane_id();
    const int64_t i = base + lane;
    // the block's 64 bytes and the 64 after them (a token starting in the block ends within 32) in
    // LDS: the token parses below read LDS, not one dependent HBM byte after the other
    uint8_t* st = stg[wave_in_block()];
    const uint8_t c = i < n ? s[i] : (uint8_t)',';
    st[lane] = c;
    st[TK_B + lane] = i + TK_B < n ? s[i + TK_B] : (uint8_t)0;
    wave_sync();
    const RlView v{st - RL_BEHIND, base, n, TK_B};   // v.at(q) = st[q - base]
    const bool par = i < n && (c == '(' || c == ')');
    // the last parenthesis strictly before this byte inside the block, else the block's state
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
    const int64_t nref = *d_nref;
    if (tok && (p < 0 || p + contrib > nref)) {
        atomicOr(err, 2);
        tok = false;
    }
    if (!WRITE) return;
    // (dcap: dec's capacity -- a fill queued before the decoded length is known writes nothing past
    // it; only a call that then fails its output-capacity check can reach it)
    if (!tok && contrib == 1 && c != '(' && o < dcap) dec[o] = c;   // literals, a stray ')' included
    unsigned long long tm = __ballot(tok);
    while (tm) {
        const int j = __ffsll((long long)tm) - 1;   // (wave-uniform: the token's fields by readlane)
        tm &= tm - 1;
        const int64_t pj = readlane64(p, j), oj = readlane64(o, j);
        int64_t lj = readlane64(contrib, j);
        if (lj > dcap - oj) lj = dcap - oj > 0 ? dcap - oj : 0;
        wave_copy(dec + oj, R + pj, lj, lane);
    }
}

// ---------------------------------------------------------------------------------------------
// output: header '\n' then result wrapped at 50 columns + final '\n'
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t first_run_ending_after(const int32_t* st, const int32_t* ln, int64_t nr, int64_t j,
                                                          int64_t a = 0) {
    int64_t b = nr;   // first r >= a with st[r] + ln[r] > j (runs sorted and disjoint)
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if ((int64_t)st[m] + ln[m] > j) b = m; else a = m + 1;
    }
    return a;
}

// N positions before j (j inside an N run: those of the run before j included), given
// r = first_run_ending_after(ns, nl, nn, j)
__device__ __forceinline__ int64_t n_before_at(const int32_t* ns, const int32_t* nl, const int64_t* ncum, int64_t nn,
                                               int64_t r, int64_t j) {
    if (r < nn) return ncum[r] + (ns[r] <= j ? j - ns[r] : 0);
    return nn ? ncum[nn - 1] + nl[nn - 1] : 0;
}

// Run-list view for format_out16: starts, ends and (N runs) the N count before each run, read
// from the block's LDS copies (GlobalRunsAt: from the global lists).
struct LdsRuns {
    const int32_t* s;
    const int32_t* e;
    const int64_t* b;
    __device__ int64_t st(int64_t r) const { return s[r]; }
    __device__ int64_t en(int64_t r) const { return e[r]; }
    __device__ int64_t nb(int64_t r) const { return b[r]; }
};

// first r in [a, b) with V::en(r) > j, ends ascending
template <typename V>
__device__ __forceinline__ int64_t first_end_after(const V& v, int64_t a, int64_t b, int64_t j) {
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (v.en(m) > j) b = m; else a = m + 1;
    }
    return a;
}

// ---------------------------------------------------------------------------------------------
// Output-centric formatter (the usual path).  A block owns OB = 4096 bytes of the OUTPUT, aligned
// to 16 bytes in memory; every thread builds 16 output bytes in registers and stores them with one
// 16-byte store (head and tail threads byte by byte).  Output byte o is the '\n' after a line when
// o % 51 == 50, else position j = o - o / 51; its byte is 'N' inside an N run, else the decoded
// byte at j minus the N positions before j, lowercased inside a lowercase run
// (decompression.cpp:241-274).  The block's decoded bytes and the runs it touches are staged in
// LDS (runs from the global lists when they are more than OFRUNS); a thread finds its first runs by
// binary search in LDS and then walks them.
// ---------------------------------------------------------------------------------------------
constexpr int OPT = 16, OB = 256 * OPT, OFRUNS = 384;   // (a block with more runs takes the global-runs path)
constexpr int TW = 5;      // k_out_index entries per block boundary (the fifth is a spare: no one reads it)
constexpr int FMT_U = 4;   // (U = 1 / 2 / 4 on one box, chr1: 0.638-0.647 / 0.634-0.639 / 0.624-0.626 ms;
                           //  round 6, U = 8: 42 KiB of LDS per block, 0.677-0.682 against 0.614-0.638)

// Block boundaries: output offset o_b = o_first + b * ob clamped to [0, total]; its position
// j_b = o - o / 51; per boundary [decoded offset d_b of j_b, first N run and first lowercase run
// ending after j_b, j_b].  One thread per (boundary, run list).
__global__ void k_out_index(int64_t nres, int64_t total, int64_t o_first, int64_t nblk, int64_t ob, const int32_t* __restrict__ ns,
                            const int32_t* __restrict__ nl, const int64_t* __restrict__ ncum, int64_t nn,
                            const int32_t* __restrict__ ls, const int32_t* __restrict__ ll, int64_t nlr,
                            int64_t* __restrict__ tab) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * (nblk + 1); i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i >> 1;
        int64_t o = o_first + b * ob;
        o = o < 0 ? 0 : (o > total ? total : o);
        const int64_t J = o - o / 51;
        if (i & 1) {
            tab[TW * b + 2] = first_run_ending_after(ls, ll, nlr, J);
        } else {
            const int64_t r = first_run_ending_after(ns, nl, nn, J);
            const int64_t d = J - n_before_at(ns, nl, ncum, nn, r, J);
            tab[TW * b + 0] = d;
            tab[TW * b + 1] = r;
            tab[TW * b + 3] = J;
        }
    }
}

__device__ __forceinline__ void store16(uint8_t* p, uint64_t lo, uint64_t hi) {
    *reinterpret_cast<uint4*>(p) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

// format_out16 with the position (j, col of oc = max(o0, 0)) and the first N / lowercase runs
// ending after j (rn, rl) given by the caller
template <typename V>
__device__ __forceinline__ void format_out16_at(int64_t o0, int64_t total, const uint8_t* sdec, int64_t dbase, const V& N,
                                                int64_t cn, int64_t ntot, const V& L, int64_t cl, uint8_t* out, int64_t j,
                                                int col, int64_t rn, int64_t rl) {
    const int64_t oc = o0 < 0 ? 0 : o0;
    int64_t n_s = INT64_MAX, n_e = INT64_MAX, n_b = ntot, l_s = INT64_MAX, l_e = INT64_MAX;
    if (rn < cn) { n_s = N.st(rn); n_e = N.en(rn); n_b = N.nb(rn); }
    if (rl < cl) { l_s = L.st(rl); l_e = L.en(rl); }
    uint64_t lo = 0, hi = 0;
    const int k0 = (int)(oc - o0), k1 = total - o0 < OPT ? (int)(total - o0) : OPT;
    if (k0 == 0 && k1 == OPT) {
        // Fast path: the thread's 16 output bytes are at most one '\n' (at knl) and 15-16 sequence
        // bytes j .. jl-1.  Lowercase runs (any number) and at most one N run inside them become
        // byte masks: the sequence bytes are the decoded bytes from j's decoded offset, those after
        // an N run inside the group from an offset shifted back by the run's length, N inside the
        // run, tolower where lowercase -- SWAR on four words, then a byte shift for the '\n'.  (A
        // per-byte loop with run bookkeeping ran whenever any lane of a wave met a run boundary:
        // with soft-masked runs every ~650 bases, nearly every wave; 620-680 VALU per wave.)
        const int knl = 50 - col;   // col in [0, 50]: the line's '\n' is output byte knl (if < 16)
        const int nseq = knl < OPT ? OPT - 1 : OPT;
        const int64_t jl = j + nseq;
        // N runs meeting [j, jl): one at most for this path
        int na = OPT, nbnd = OPT, nin = 0;   // N bytes [na, nbnd) of the group (relative)
        int64_t r = rn;
        int64_t nbj;                          // N bases before j
        if (rn < cn && n_s < j) nbj = n_b + (j - n_s);
        else nbj = rn < cn ? n_b : ntot;
        while (r < cn && (r == rn ? n_s : N.st(r)) < jl) {
            const int64_t rs = r == rn ? n_s : N.st(r), re = r == rn ? n_e : N.en(r);
            na = (int)((rs > j ? rs : j) - j);
            nbnd = (int)((re < jl ? re : jl) - j);
            nin++;
            r++;
        }
        const int64_t at1 = j - nbj - dbase;             // decoded offset of byte 0 (bytes before the N run)
        const int64_t at2 = at1 - (nbnd - na);            // (bytes after it: byte p at at2 + p)
        const uint32_t nm = nin ? (((1u << nbnd) - 1u) & ~((1u << na) - 1u)) : 0u;
        const uint32_t after = nin ? (~((1u << nbnd) - 1u) & 0xffffu) : 0u;   // bytes from the shifted window
        const bool use1 = (~after & ~nm & 0xffffu) != 0, use2 = after != 0;
        if (nin <= 1 && (!use1 || at1 >= 0) && (!use2 || at2 >= 0)) {
            // lowercase byte mask (bit per byte)
            uint32_t lm = 0;
            for (int64_t q = rl; q < cl; q++) {
                const int64_t ls = q == rl ? l_s : L.st(q);
                if (ls >= jl) break;
                const int64_t le = q == rl ? l_e : L.en(q);
                const int s0 = (int)((ls > j ? ls : j) - j), e0 = (int)((le < jl ? le : jl) - j);
                if (e0 > s0) lm |= ((1u << e0) - 1u) & ~((1u << s0) - 1u);
            }
            uint32_t w1[4] = {0, 0, 0, 0}, w2[4] = {0, 0, 0, 0};
            auto load16 = [&](int64_t at, uint32_t (&w)[4]) {
                const uint4 v = load16u(reinterpret_cast<const uint8_t*>(sdec) + at);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            };
            if (use1) load16(at1, w1);
            if (use2) load16(at2, w2);
            uint32_t w[4];
#pragma unroll
            for (int qq = 0; qq < 4; qq++) {
                // bit masks -> byte masks for bytes 4qq .. 4qq+3
                const uint32_t nb4 = (nm >> (4 * qq)) & 0xfu, ab4 = (after >> (4 * qq)) & 0xfu, lb4 = (lm >> (4 * qq)) & 0xfu;
                const uint32_t nB = (nb4 * 0x00204081u & 0x01010101u) * 0xffu;   // bit i -> byte i = 0xff
                const uint32_t aB = (ab4 * 0x00204081u & 0x01010101u) * 0xffu;
                const uint32_t lB = (lb4 * 0x00204081u & 0x01010101u) * 0xffu;
                uint32_t x = (w1[qq] & ~aB) | (w2[qq] & aB);
                x = (x & ~nB) | (0x4E4E4E4Eu & nB);                               // 'N'
                const uint32_t ge_a = ((x | 0x80808080u) - 0x41414141u) & 0x80808080u;   // byte >= 'A' (7-bit)
                const uint32_t gt_z = ((x | 0x80808080u) - 0x5B5B5B5Bu) & 0x80808080u;   // byte >= 'Z' + 1
                const uint32_t up = ge_a & ~gt_z & ~x & lB;                       // tolower where lowercase
                w[qq] = x + (up >> 2);
            }
            uint64_t slo = (uint64_t)w[0] | ((uint64_t)w[1] << 32), shi = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
            if (knl < OPT) {   // bytes from knl on move up by one; '\n' at knl
                const uint64_t ulo = slo << 8, uhi = (shi << 8) | (slo >> 56);
                const uint64_t mlo = knl >= 8 ? ~0ull : (knl ? (1ull << (8 * knl)) - 1ull : 0ull);
                const uint64_t mhi = knl <= 8 ? 0ull : (1ull << (8 * (knl - 8))) - 1ull;
                slo = (slo & mlo) | (ulo & ~mlo);
                shi = (shi & mhi) | (uhi & ~mhi);
                if (knl < 8) slo = (slo & ~(0xffull << (8 * knl))) | ((uint64_t)'\n' << (8 * knl));
                else shi = (shi & ~(0xffull << (8 * (knl - 8)))) | ((uint64_t)'\n' << (8 * (knl - 8)));
            }
            store16(out + o0, slo, shi);
            return;
        }
    }
    for (int k = k0; k < k1; k++) {
        uint32_t c;
        if (col == 50) {
            c = '\n';
            col = 0;
        } else {
            while (j >= n_e) {
                rn++;
                if (rn < cn) { n_s = N.st(rn); n_e = N.en(rn); n_b = N.nb(rn); }
                else { n_s = n_e = INT64_MAX; n_b = ntot; }
            }
            while (j >= l_e) {
                rl++;
                if (rl < cl) { l_s = L.st(rl); l_e = L.en(rl); }
                else l_s = l_e = INT64_MAX;
            }
            c = j >= n_s ? (uint32_t)'N' : (uint32_t)sdec[j - n_b - dbase];
            if (j >= l_s) c = c_tolower((uint8_t)c);
            j++;
            col++;
        }
        if (k < 8) lo |= (uint64_t)c << (8 * k);
        else hi |= (uint64_t)c << (8 * (k - 8));
    }
    if (k0 == 0 && k1 == OPT) {
        store16(out + o0, lo, hi);
    } else {
        for (int k = k0; k < k1; k++) out[o0 + k] = (uint8_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xff);
    }
}

template <typename V>
__device__ __forceinline__ void format_out16(int64_t o0, int64_t total, int64_t nres, const uint8_t* sdec, int64_t dbase,
                                             const V& N, int64_t cn, int64_t ntot, const V& L, int64_t cl, uint8_t* out) {
    (void)nres;
    const int64_t oc = o0 < 0 ? 0 : o0;
    if (oc >= total || o0 + OPT <= 0) return;
    const int64_t j = oc - oc / 51;
    const int col = (int)(oc % 51);
    format_out16_at(o0, total, sdec, dbase, N, cn, ntot, L, cl, out, j, col, first_end_after(N, 0, cn, j),
                    first_end_after(L, 0, cl, j));
}

// first r in [0, c) with e[r] > j over an LDS run list: short lists (a tile holds a few runs) by a
// linear pass, long ones by bisection
__device__ __forceinline__ int32_t lds_first_end_after(const int32_t* e, int32_t c, int32_t j) {
    if (c <= 16) {
        int32_t r = 0;
        while (r < c && e[r] <= j) r++;
        return r;
    }
    int32_t a = 0, b = c;
    while (a < b) {
        const int32_t m = (a + b) >> 1;
        if (e[m] > j) b = m; else a = m + 1;
    }
    return a;
}

// runs of the global lists from index a on, as views starting at 0 (format_out16's fallback)
struct GlobalRunsAt {
    const int32_t* s;
    const int32_t* l;
    const int64_t* b;
    int64_t a;
    __device__ int64_t st(int64_t r) const { return s[a + r]; }
    __device__ int64_t en(int64_t r) const { return (int64_t)s[a + r] + l[a + r]; }
    __device__ int64_t nb(int64_t r) const { return b ? b[a + r] : 0; }
};

// U: 16-byte outputs per thread (a block owns U * OB output bytes: fewer, larger dependent load
// phases per byte)
__global__ __launch_bounds__(256) void k_format_out(const uint8_t* __restrict__ dec, int64_t nres, int64_t total, int64_t o_first,
                                                    const int32_t* __restrict__ ns, const int32_t* __restrict__ nl,
                                                    const int64_t* __restrict__ ncum, int64_t nn,
                                                    const int32_t* __restrict__ ls, const int32_t* __restrict__ ll,
                                                    int64_t nlr, const int64_t* __restrict__ tab, uint8_t* __restrict__ out) {
    // the tile's decoded bytes from a 16-byte-aligned base, 16 bytes per thread and load, with
    // 16 bytes of slack for format_out16's unaligned 16-byte reads (dec holds >= 64 bytes of slack)
    constexpr int U = FMT_U;
    __shared__ uint4 sdec4[(U * OB + 64) / 16];
    __shared__ int32_t s_ns[OFRUNS], s_ne[OFRUNS], s_ls[OFRUNS], s_le[OFRUNS];
    __shared__ int64_t s_nb[OFRUNS];
    __shared__ int64_t st[2 * TW];
    uint32_t* sdec_w = reinterpret_cast<uint32_t*>(sdec4);
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;   // (a grid-stride loop over blocks: 0.35-0.43 ms instead of 0.27)
    if (tid < 2 * TW) st[tid] = tab[TW * b + tid];
    __syncthreads();
    const int64_t d0 = st[0], d1 = st[TW];
    const int64_t n_lo = st[1], n_hi = st[TW + 1] < nn ? st[TW + 1] + 1 : nn;
    const int64_t l_lo = st[2], l_hi = st[TW + 2] < nlr ? st[TW + 2] + 1 : nlr;
    const int64_t ntot = nn ? ncum[nn - 1] + nl[nn - 1] : 0;
    const bool lds_runs = n_hi - n_lo <= OFRUNS && l_hi - l_lo <= OFRUNS;
    const int64_t a0 = d0 & ~(int64_t)15;
    const int64_t n16 = (d1 - a0 + 16 + 15) >> 4;   // <= (U * OB + 46) / 16
    const uint4* dec4 = reinterpret_cast<const uint4*>(dec + a0);
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t i = tid + 256 * u;
        if (i < n16) sdec4[i] = dec4[i];
    }
    if (U * 256 + tid < n16) sdec4[U * 256 + tid] = dec4[U * 256 + tid];
    if (lds_runs) {
        for (int64_t r = n_lo + tid; r < n_hi; r += 256) {
            const int32_t x = ns[r];
            s_ns[r - n_lo] = x;
            s_ne[r - n_lo] = x + nl[r];
            s_nb[r - n_lo] = ncum[r];
        }
        for (int64_t r = l_lo + tid; r < l_hi; r += 256) {
            const int32_t x = ls[r];
            s_ls[r - l_lo] = x;
            s_le[r - l_lo] = x + ll[r];
        }
    }
    __syncthreads();
    const uint8_t* sdec = reinterpret_cast<const uint8_t*>(sdec_w);
    // the block's first output offset (clamped) and its (j, col): a thread's (j, col) follow in 32-bit
    // arithmetic from its offset inside the block (no 64-bit division per thread)
    const int64_t ob = o_first + b * (U * OB), obc = ob < 0 ? 0 : ob;
    const int64_t Jb = st[3];   // obc - obc / 51 (k_out_index)
    const int32_t colb = (int32_t)(obc - 51 * (obc - Jb));
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t o0 = ob + (int64_t)(u * 256 + tid) * OPT;
        if (lds_runs) {
            const int64_t oc = o0 < 0 ? 0 : o0;
            if (oc >= total || o0 + OPT <= 0) continue;
            const int32_t q = colb + (int32_t)(oc - obc);
            const int32_t nl51 = q / 51;
            const int64_t j = Jb + (oc - obc) - nl51;
            const int col = q - 51 * nl51;
            const int32_t jr = (int32_t)j;   // (positions are int32 in the run lists)
            const LdsRuns N{s_ns, s_ne, s_nb}, L{s_ls, s_le, nullptr};
            format_out16_at(o0, total, sdec, a0, N, n_hi - n_lo, ntot, L, l_hi - l_lo, out, j, col,
                            lds_first_end_after(s_ne, (int32_t)(n_hi - n_lo), jr),
                            lds_first_end_after(s_le, (int32_t)(l_hi - l_lo), jr));
        } else {
            const GlobalRunsAt N{ns, nl, ncum, n_lo}, L{ls, ll, nullptr, l_lo};
            format_out16(o0, total, nres, sdec, a0, N, n_hi - n_lo, ntot, L, l_hi - l_lo, out);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Region fetch (sccg_reader_fetch*, sccg_cohort_fetch*): bases [begin, end) of the sequence -- result
// of decompression.cpp:241-262, N inserted and lowercased, no '\n' -- for a batch of regions,
// concatenated in the order given, from the state a reader keeps (DcFetchSrc).  One launch for the
// whole batch.  The flat space of output bases is tiled as in the formatter: a block owns OB of
// them, a wave FT_W = 1,024, a lane 16, 16-byte pieces aligned in memory.  The parts, in this order:
//   fetch_decode_span  a span's decode: positions [j0, j1) -> decoded offsets [d0, d1) over the N
//                      runs -> record blocks [b0, b1] over boff -> the k_tok_fill2 parse of just those
//                      blocks, every literal and token copy clipped to [d0, d1), into the wave's LDS
//                      tile (a long token is entered at R' + p + (d0 - o)); ORIGIN keeps where a byte
//                      comes from instead of the byte
//   NCursor, LCursor   a lane's cursors over the N and the lowercase runs for the formatter's
//                      per-base walk over that tile
//   fetch_spans        the loop every kernel sits on: the wave's first region in the prefix of region
//                      lengths, then its spans one after the other, each with its source and strand
//   k_fetch_enc        bytes, codes or one-hot elements; k_fetch_origin: reference positions
//   dc_fetch           the one launcher
// Every search is a wave-wide 64-ary one (64 probes per step); nothing is swept end to end, no scratch
// beyond LDS.  The reader's open has checked every token and run: nothing is re-checked here.
// ---------------------------------------------------------------------------------------------
constexpr int FT_W = 64 * OPT;
static_assert(FT_W * WPB == OB, "a block of WPB waves owns OB output bytes");

// first m in [a, b) with pred(m), b if none; pred monotone (false .. true), a and b wave-uniform
template <typename P>
__device__ __forceinline__ int64_t wave_first(int64_t a, int64_t b, P&& pred) {
    const int lane = lane_id();
    while (b - a > 64) {
        const int64_t step = (b - a + 63) >> 6;
        const int64_t m = a + (int64_t)lane * step + step - 1;   // the last entry of this lane's chunk
        const unsigned long long t = __ballot(m >= b || pred(m));
        if (!t) return b;   // (the last chunk ends exactly at b - 1 and is false there)
        const int c = __ffsll((long long)t) - 1;
        const int64_t mc = a + (int64_t)c * step + step - 1;
        a += (int64_t)c * step;
        b = mc < b ? mc : b;   // pred(mc) holds (or mc is past the end): the answer is in [a, mc]
    }
    const unsigned long long t = __ballot(a + lane < b && pred(a + lane));
    return t ? a + (__ffsll((long long)t) - 1) : b;
}

// A span's decode, shared by the fetch kernels: sequence positions [j0, j1) (j1 - j0 <= FT_W) ->
// decoded offsets [d0, d1) over the N runs -> record blocks [b0, b1] over boff -> k_tok_fill2's parse
// of those blocks with every copy clipped to [d0, d1) into the wave's tile sdec (decoded byte d at
// sdec[d - d0]; st: the wave's 2 * TK_B staging bytes).  Returns the first N run ending after j0
// and d0; the tile is complete (wave_sync) on return.
struct FetchSpan {
    int64_t rn0, d0;
};
// The ORIGIN arm keeps where a byte comes from instead of the byte: its tile is FO_TILE int32, decoded
// offset d at org[opad(d - d0)] -- a literal -1, byte (a - oj) + k of the token at R' position pj the
// position in the reference sequence R of R' position v = pj + (a - oj) + k.  R' is not read.  (opad:
// a lane's 16 consecutive entries start 17 words after its neighbour's, so the per-lane walks of the
// epilogue meet no LDS bank twice.)
// R' -> R: S.rm lists the runs of 'N' in R that R' has erased; run m is crossed from R' position
// key(m) = start[m] - cum[m] on, the keys ascend strictly, and v lies at v + (the N of every run with
// key <= v).  The search is the wave's, once per token piece and not per base: a 64-ary wave_first
// for the piece's first position v0 gives the bracket [lo, hi) of keys around it and the N count
// `add` that holds inside; a piece that ends inside the bracket -- nearly every one: a piece is at most
// 1,024 bases, a reference's runs are far apart -- is v0 + k + add for all its lanes.  The bracket is
// kept (MapCur, wave-uniform) across tokens and spans of one map: the tokens of a span are neighbours
// on the reference, so the next one usually loads nothing of the map.  A piece that crosses runs
// bounds them with a second wave_first and each lane searches those few for its positions.
constexpr int FO_TILE = FT_W + FT_W / 16;
__device__ __forceinline__ int opad(int i) { return i + (i >> 4); }
struct MapCur {
    int64_t mi, lo, hi, add;   // keys [lo, hi) = [key(mi - 1), key(mi)): add N lie before such a position
};
__device__ __forceinline__ int64_t map_key(const DcRuns& M, int64_t m) { return (int64_t)M.start[m] - M.cum[m]; }
// The bracket around R' position v: wave_first's 64-ary narrowing over the keys, whose last step has
// the bracket's own entries in the lanes -- key and cum of up to 64 candidates, the upper bound
// included, loaded in one round and handed over by readlane -- so a map of up to 63 runs (a
// chromosome's) costs one round of loads, where a search and then a read of its result cost two.
__device__ __forceinline__ void map_seek(const DcRuns& M, int64_t v, MapCur& c) {
    const int lane = lane_id();
    int64_t a = 0, b = M.n;   // the first m with key(m) > v is in [a, b]; key(b) > v, or b == M.n
    while (b - a > 63) {
        const int64_t step = (b - a + 63) >> 6;
        const int64_t m = a + (int64_t)lane * step + step - 1;   // the last entry of this lane's chunk
        const unsigned long long t = __ballot(m >= b || map_key(M, m) > v);
        if (!t) { a = b; break; }
        const int h = __ffsll((long long)t) - 1;
        const int64_t mh = a + (int64_t)h * step + step - 1;
        a += (int64_t)h * step;
        b = mh < b ? mh : b;
    }
    const int64_t m = a + lane;   // lanes 0 .. b - a hold entries a .. b
    const bool in = m <= b && m < M.n;
    const int64_t cu = in ? M.cum[m] : M.total, ky = in ? (int64_t)M.start[m] - cu : INT64_MAX;
    const int h = __ffsll((long long)__ballot(m <= b && ky > v)) - 1;   // (lane b - a always qualifies)
    c.mi = a + h;
    c.hi = readlane64(ky, h);
    c.add = readlane64(cu, h);
    c.lo = h > 0 ? readlane64(ky, h - 1) : c.mi > 0 ? map_key(M, c.mi - 1) : INT64_MIN;
}
// org[opad(at + k)] = the R position of R' position v0 + k, k < cnt (the whole wave calls it)
__device__ __forceinline__ void origin_piece(const DcRuns& M, int64_t v0, int cnt, int32_t* org, int at, MapCur& c) {
    const int lane = lane_id();
    if (!M.n) {   // R' is R
        for (int k = lane; k < cnt; k += 64) org[opad(at + k)] = (int32_t)(v0 + k);
        return;
    }
    if (v0 < c.lo || v0 >= c.hi) map_seek(M, v0, c);
    if (v0 + cnt <= c.hi) {
        const int32_t r0 = (int32_t)(v0 + c.add);
        for (int k = lane; k < cnt; k += 64) org[opad(at + k)] = r0 + k;
        return;
    }
    // runs [c.mi, m1) are crossed inside the piece
    const int64_t vend = v0 + cnt, m1 = wave_first(c.mi + 1, M.n, [&](int64_t m) { return map_key(M, m) >= vend; });
    for (int k = lane; k < cnt; k += 64) {
        const int64_t v = v0 + k;
        int64_t a = c.mi, b = m1;   // first m with key(m) > v
        while (a < b) {
            const int64_t m = (a + b) >> 1;
            if (map_key(M, m) > v) b = m; else a = m + 1;
        }
        org[opad(at + k)] = (int32_t)(v + (a < M.n ? M.cum[a] : M.total));
    }
}
template <bool ORIGIN = false>
__device__ __forceinline__ FetchSpan fetch_decode_span(const DcFetchSrc& S, int64_t j0, int64_t j1, uint8_t* sdec, uint8_t* st,
                                                       MapCur* mc = nullptr) {
    int32_t* org = reinterpret_cast<int32_t*>(sdec);   // (ORIGIN: the tile is the wave's int32 one)
    const int lane = lane_id();
    const uint8_t* __restrict__ rec = S.rec;
    const int64_t n = S.nrec, nblk = (n + TK_B - 1) / TK_B;
    const int64_t* __restrict__ boff = S.boff;
    const int32_t* __restrict__ ns = S.nr.start;
    const int32_t* __restrict__ nl = S.nr.len;
    const int64_t* __restrict__ ncum = S.nr.cum;
    const int64_t nn = S.nr.n;
    // positions -> decoded offsets: the N positions before j0 and before j1
    const int64_t rn0 = wave_first(0, nn, [&](int64_t m) { return (int64_t)ns[m] + nl[m] > j0; });
    const int64_t rn1 = wave_first(rn0, nn, [&](int64_t m) { return (int64_t)ns[m] + nl[m] > j1; });
    const int64_t d0 = j0 - n_before_at(ns, nl, ncum, nn, rn0, j0), d1 = j1 - n_before_at(ns, nl, ncum, nn, rn1, j1);
    if (d1 > d0) {
        // record blocks holding decoded bytes d0 and d1 - 1 (a block's bytes: [boff[b], boff[b + 1]))
        const int64_t b0 = wave_first(1, nblk, [&](int64_t m) { return boff[m] > d0; }) - 1;
        const int64_t b1 = wave_first(b0 + 1, nblk, [&](int64_t m) { return boff[m] >= d1; }) - 1;
        for (int64_t b = b0; b <= b1; b++) {
            // k_tok_fill2's parse of block b
            const int64_t rb = b * TK_B, ri = rb + lane;
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
                    if (comma > 0 && close > comma && parse_int_v(v, ri + 1, comma, &d) &&
                        parse_int_v(v, comma + 1, close, &l) && l >= 0) {
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
            const int64_t p = S.bdsum[b] + wave_incl_add(d);   // running p, this token included
            if (!tok && contrib == 1 && c != '(' && o >= d0 && o < d1) {
                if (ORIGIN) org[opad((int)(o - d0))] = -1;
                else sdec[o - d0] = c;
            }
            unsigned long long tm = __ballot(tok && o < d1 && o + contrib > d0);
            while (tm) {
                const int j = __ffsll((long long)tm) - 1;   // (wave-uniform: the token's fields by readlane)
                tm &= tm - 1;
                const int64_t pj = readlane64(p, j), oj = readlane64(o, j), lj = readlane64(contrib, j);
                const int64_t a = oj > d0 ? oj : d0, e = oj + lj < d1 ? oj + lj : d1;
                if (ORIGIN) {   // (the open's range check: pj + lj <= |R'| <= |R| < 2^31)
                    origin_piece(S.rm, pj + (a - oj), (int)(e - a), org, (int)(a - d0), *mc);
                    continue;
                }
                const uint8_t* __restrict__ src = S.R + pj + (a - oj);   // not walked there from the token's start
                uint8_t* dst = sdec + (a - d0);
                const int cnt = (int)(e - a), k = lane * OPT;   // cnt <= FT_W: one 16-byte load per lane
                if (k < cnt) {
                    const uint4 x = load16u(src + k);   // (up to 15 bytes past the token: R' carries the slack)
                    const uint32_t w4[4] = {x.x, x.y, x.z, x.w};
                    const int m = cnt - k < OPT ? cnt - k : OPT;
#pragma unroll
                    for (int q = 0; q < OPT; q++)
                        if (q < m) dst[k + q] = (uint8_t)(w4[q >> 2] >> (8 * (q & 3)));
                }
            }
        }
        wave_sync();
    }
    return FetchSpan{rn0, d0};
}

// A lane's cursor over the N runs while its positions j ascend: run r is [s, e) with b N bases before
// it; past the last run s = e = INT64_MAX and b = ntot.  (The run pointers stay plain: __restrict__
// here cost the ASCII kernel 4 VGPRs.)
struct NCursor {
    const int32_t* ns;
    const int32_t* nl;
    const int64_t* ncum;
    int64_t nn, ntot, r, s, e, b;
    __device__ __forceinline__ NCursor(const DcCohortEntry& E, int64_t r0)
        : ns(E.S.nr.start), nl(E.S.nr.len), ncum(E.S.nr.cum), nn(E.nn), ntot(E.ntot), r(r0) {
        load();
    }
    __device__ __forceinline__ void load() {   // (the sentinel first: as an else arm it put ntot on the stack)
        s = e = INT64_MAX;
        b = ntot;
        if (r < nn) { s = ns[r]; e = s + nl[r]; b = ncum[r]; }
    }
    __device__ __forceinline__ void seek(int64_t j) {   // the first run ending after j
        while (j >= e) {
            r++;
            load();
        }
    }
};
// The same over the first nlr lowercase runs (nlr == 0: case is not looked at).
struct LCursor {
    const int32_t* ls;
    const int32_t* ll;
    int64_t nlr, r, s, e;
    __device__ __forceinline__ LCursor(const DcCohortEntry& E, int64_t nlr_, int64_t r0)
        : ls(E.S.lr.start), ll(E.S.lr.len), nlr(nlr_), r(r0) {
        load();
    }
    __device__ __forceinline__ void load() {
        s = e = INT64_MAX;
        if (r < nlr) { s = ls[r]; e = s + ll[r]; }
    }
    __device__ __forceinline__ void seek(int64_t j) {
        while (j >= e) {
            r++;
            load();
        }
    }
};
// the first lowercase run (of the nlr looked at) ending after j0: the LCursor's start, wave-wide
__device__ __forceinline__ int64_t first_lower_run(const DcCohortEntry& E, int64_t nlr, int64_t j0) {
    const int32_t* __restrict__ ls = E.S.lr.start;
    const int32_t* __restrict__ ll = E.S.lr.len;
    return wave_first(0, nlr, [&](int64_t m) { return (int64_t)ls[m] + ll[m] > j0; });
}

// What every fetch kernel is launched with (dc_fetch fills it).  The flat space is counted in bases:
// block 0's first base is o_first <= 0, so that a wave's 16-byte pieces are aligned in memory.
struct FetchArgs {
    DcCohortEntry E;            // the reader's source (!COHORT)
    const DcCohortEntry* tab;   // one entry per sample (COHORT)
    const int64_t* pre;         // nreg + 1: exclusive prefix of the region lengths, pre[nreg] = F
    const int64_t* beg;         // nreg: region begins, bit 63 set = reverse strand
    const int32_t* samp;        // nreg: region samples (COHORT)
    int64_t nreg, F, o_first;
    uint32_t all_rev, elemwise, upper;   // elemwise: out is not on a base boundary; upper: no lowercase runs
    void* out;
};

// A table entry through a wave-uniform index, read as constant memory (nothing writes the table
// after sccg_cohort_create): with both, the loads are scalar and the entry lands in SGPRs, as the
// reader's entry in the kernel arguments does.
typedef const int64_t __attribute__((address_space(4))) * ConstWords;
__device__ __forceinline__ DcCohortEntry cohort_entry(const DcCohortEntry* tab, int sm) {
    constexpr int NW = (int)(sizeof(DcCohortEntry) / sizeof(int64_t));
    static_assert(sizeof(DcCohortEntry) == NW * sizeof(int64_t), "an entry is whole 8-byte words");
    const ConstWords w = (ConstWords)(uintptr_t)(tab + sm);
    int64_t v[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) v[k] = w[k];
    DcCohortEntry E;
    __builtin_memcpy(&E, v, sizeof E);
    return E;
}

// The wave's tile of the flat space: bases [base, base + FT_W), of which [w0, fend) are this launch's
// (none when w0 >= fend); lane l owns the OPT bases from base + l * OPT.
struct FetchTile {
    int64_t base, w0, fend;
};
__device__ __forceinline__ FetchTile fetch_tile(const FetchArgs& A) {
    const int64_t base = A.o_first + ((int64_t)blockIdx.x * WPB + wave_in_block()) * FT_W;
    return FetchTile{base, base < 0 ? 0 : base, base + FT_W < A.F ? base + FT_W : A.F};
}

// The loop of every fetch kernel: the spans of the wave's tile one after the other.  It finds the
// region holding the tile's first base in the prefix (the last i with pre[i] <= f; an empty region
// never is), steps to the next region that is not empty, takes the span's sample entry -- COHORT:
// samp[i] made provably uniform (readfirstlane) and, when it differs from the sample held, its table
// entry; else the entry of the arguments -- and maps the span [f, fe) to the forward positions
// [j0, j1) it covers (j1 - j0 <= FT_W): a region is reversed by bit 63 of its begin or all_rev, and
// flat base g of a reversed region is position end - 1 - (g - pre[i]).  The whole wave then calls
//     body(entry, j0, j1, rev, j, k0, k1)
// where the lane's bases of the span are its k0-th to k1-th (none: k0 >= k1) and j is the lowest of
// their positions: the lane walks j ascending and places result t at k0 + t, or k1 - 1 - t when rev.
// What the body read of the wave's tiles is synchronised before the next span, and once more after
// the last.
template <bool COHORT, typename Body>
__device__ __forceinline__ void fetch_spans(const FetchArgs& A, const FetchTile& T, Body&& body) {
    const int64_t g0 = T.base + (int64_t)lane_id() * OPT;
    const int64_t* __restrict__ pre = A.pre;
    DcCohortEntry E = A.E;
    int cur = -1;   // the sample E holds (COHORT)
    int64_t f = T.w0;
    int64_t i = wave_first(1, A.nreg + 1, [&](int64_t m) { return pre[m] > f; }) - 1;
    while (f < T.fend) {
        if (pre[i + 1] <= f) {   // usually i + 1 is not empty, else searched for
            i++;
            if (pre[i + 1] <= f) i = wave_first(i + 1, A.nreg + 1, [&](int64_t m) { return pre[m] > f; }) - 1;
        }
        if (COHORT) {
            const int sm = __builtin_amdgcn_readfirstlane(A.samp[i]);
            if (sm != cur) {   // (wave-uniform: a scalar branch around scalar loads)
                cur = sm;
                E = cohort_entry(A.tab, sm);
            }
        }
        const int64_t fe = pre[i + 1] < T.fend ? pre[i + 1] : T.fend;
        const int64_t braw = A.beg[i];
        const bool rev = A.all_rev || braw < 0;
        const int64_t bg = braw & INT64_MAX;
        const int64_t j0 = rev ? bg + (pre[i + 1] - fe) : bg + (f - pre[i]), j1 = j0 + (fe - f);
        const int64_t ga = g0 > f ? g0 : f, gb = g0 + OPT < fe ? g0 + OPT : fe;
        body(E, j0, j1, rev, rev ? j0 + (fe - gb) : j0 + (ga - f), (int)(ga - g0), (int)(gb - g0));
        wave_sync();   // (the tile is read before the next span fills it)
        f = fe;
    }
    wave_sync();
}

// ---------------------------------------------------------------------------------------------
// The byte kernels (k_fetch_enc<ENC, DT, COHORT>; sccg_reader_fetch's bytes are ASCII, forward): the
// strand and the encoding are an epilogue on the decode tile.  Each span is decoded forward by
// fetch_decode_span; a lane walks its bases ascending in j and
// writes each final byte (ASCII, complemented when reversed) or code (0-3, 4 = not ACGT; 3 - code
// when reversed) at its OUTPUT place in a second LDS tile, `fin`, one byte per base.  When the
// wave's spans are done it streams fin out in 16-byte pieces, piece q to lane q % 64, so every
// store instruction of the wave writes 1 KiB contiguous whatever the regions' lengths are: a
// piece holds 16 / 4 / 2 / 1 bases at 1 / 4 / 8 / 16 bytes per base, expanded from the codes in
// registers.  Pieces cut by the tile's ends [max(base, 0), fend), and every piece when d_out is
// not aligned to a whole base (elemwise), are stored element by element.  INDEX and ONEHOT are
// case-blind: their nlr is 0 and they never look at the lowercase runs.
// ---------------------------------------------------------------------------------------------
constexpr int FE_ASCII = 0, FE_INDEX = 1, FE_ONEHOT = 2, FE_ORIGIN = 3;      // SCCG_ENC_*
constexpr int FD_U8 = 0, FD_F16 = 1, FD_BF16 = 2, FD_F32 = 3, FD_I32 = 4;   // SCCG_DT_*

// IUPAC complement of an uppercase letter as its index 0..25, 13 letters x 5 bits per word
// (A<->T C<->G R<->Y K<->M B<->V D<->H; every other letter is its own)
// Thirteen 5-bit entries fill 65 bits: 'Z' (the last of the second word, and its own complement)
// has no entry -- its value would lose bit 64 -- and comp_ascii leaves it alone with the non-letters.
constexpr uint64_t comp_word(int half) {
    const char* from = "ACGTRYKMBVDH";
    const char* to = "TGCAYRMKVBHD";
    uint64_t w = 0;
    for (int i = 0; i < (half ? 12 : 13); i++) {
        const int c = 13 * half + i;
        int r = c;
        for (int k = 0; k < 12; k++)
            if (from[k] - 'A' == c) r = to[k] - 'A';
        w |= (uint64_t)r << (5 * i);
    }
    return w;
}
constexpr uint64_t COMP_LO = comp_word(0), COMP_HI = comp_word(1);
static_assert((COMP_LO & 31) == 'T' - 'A' && ((COMP_HI >> (5 * ('T' - 'N'))) & 31) == 0, "A <-> T");
static_assert(((COMP_LO >> (5 * ('K' - 'A'))) & 31) == 'M' - 'A' && (COMP_HI & 31) == 'N' - 'A', "K -> M, N -> N");
static_assert(((COMP_HI >> (5 * ('Y' - 'N'))) & 31) == 'R' - 'A' && ((COMP_LO >> (5 * ('M' - 'A'))) & 31) == 'K' - 'A',
              "Y -> R, M -> K: each word's last entry");

// the complement of a sequence byte, case kept; a byte that is no letter (and 'Z' / 'z') is unchanged
__device__ __forceinline__ uint32_t comp_ascii(uint32_t c) {
    const uint32_t idx = (c | 0x20u) - 'a';
    if (idx >= 25u) return c;
    const uint64_t w = idx < 13u ? COMP_LO : COMP_HI;
    const uint32_t r = (uint32_t)(w >> (5u * (idx < 13u ? idx : idx - 13u))) & 31u;
    return ('A' + r) | (c & 0x20u);
}

// A/a 0, C/c 1, G/g 2, T/t 3, every other byte 4
__device__ __forceinline__ uint32_t base_code(uint32_t c) {
    const uint32_t u = c & 0xDFu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

// A lane's bases of one span (fetch_spans' j, k0, k1): positions j, j + 1, ... through the N runs
// from rn and the lowercase runs from rl, each final byte or code at its output place in
// mine[k0, k1) -- descending for a reversed span.
template <int ENC>
__device__ __forceinline__ void fetch_enc_walk(const DcCohortEntry& E, int64_t nlr, const uint8_t* sdec, uint8_t* mine, int64_t j,
                                               int64_t rn, int64_t rl, int64_t d0, bool rev, int k0, int k1) {
    NCursor N(E, rn);
    LCursor L(E, nlr, rl);
    for (int t = 0; t < k1 - k0; t++) {
        N.seek(j);
        L.seek(j);
        uint32_t c = j >= N.s ? (uint32_t)'N' : (uint32_t)sdec[j - N.b - d0];
        if (ENC == FE_ASCII) {
            if (j >= L.s) c = c_tolower((uint8_t)c);
            if (rev) c = comp_ascii(c);
        } else {
            c = base_code(c);
            if (rev && c < 4u) c = 3u - c;
        }
        j++;
        mine[rev ? k1 - 1 - t : k0 + t] = (uint8_t)c;
    }
}

// The streamed epilogue, shared likewise: the wave's finished tile fw (one byte per base, flat bases
// [base, base + FT_W), of which [w0, fend) are this launch's) out in 16-byte pieces, piece q to lane
// q % 64; cut pieces, and every piece when elemwise, element by element.
template <int ENC, int DT>
__device__ __forceinline__ void fetch_enc_stream(const uint8_t* fw, int64_t base, int64_t w0, int64_t fend, uint32_t elemwise,
                                                 uint8_t* out, int lane) {
    constexpr int ES = DT == FD_U8 ? 1 : DT == FD_F32 ? 4 : 2;   // element bytes
    constexpr int BPB = ENC == FE_ONEHOT ? 4 * ES : 1;           // bytes per base
    constexpr int PB = 16 / BPB;                                 // bases per 16-byte piece
    constexpr uint32_t ONE = DT == FD_U8 ? 1u : DT == FD_F16 ? 0x3C00u : DT == FD_BF16 ? 0x3F80u : 0x3F800000u;
    for (int it = 0; it < BPB; it++) {
        const int q = it * 64 + lane;
        const int64_t p0 = base + (int64_t)q * PB;   // the piece's first base
        if (p0 >= fend || p0 + PB <= w0) continue;
        const uint8_t* src = fw + q * PB;
        uint8_t* dst = out + p0 * BPB;
        const bool full = !elemwise && p0 >= w0 && p0 + PB <= fend;
        if (BPB == 1) {
            if (full) {
                *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
            } else {
                for (int t = 0; t < PB; t++)
                    if (p0 + t >= w0 && p0 + t < fend) dst[t] = src[t];
            }
        } else {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int t = 0; t < PB; t++) {
                const uint32_t code = src[t];
                if (ES == 1) {
                    w[t] = code < 4u ? ONE << (8u * code) : 0u;
                } else if (ES == 2) {
                    const uint64_t v = code < 4u ? (uint64_t)ONE << (16u * code) : 0ull;
                    w[2 * t] = (uint32_t)v;
                    w[2 * t + 1] = (uint32_t)(v >> 32);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++) w[e] = code == (uint32_t)e ? ONE : 0u;
                }
            }
            if (full) {
                *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int t = 0; t < PB; t++) {
                    if (p0 + t < w0 || p0 + t >= fend) continue;
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int by = (t * 4 + e) * ES;   // the element's byte in the piece
                        const uint32_t x = w[by >> 2] >> (8 * (by & 3));
                        if (ES == 1) dst[by] = (uint8_t)x;
                        else if (ES == 2) *reinterpret_cast<uint16_t*>(dst + by) = (uint16_t)x;
                        else *reinterpret_cast<uint32_t*>(dst + by) = x;
                    }
                }
            }
        }
    }
}

template <int ENC, int DT, bool COHORT>
__global__ __launch_bounds__(SCCG_BLOCK) void k_fetch_enc(const FetchArgs A) {
    static_assert(ENC == FE_ONEHOT || DT == FD_U8, "ASCII and INDEX are bytes");
    __shared__ uint8_t tile[WPB][FT_W];
    __shared__ __attribute__((aligned(16))) uint8_t fin[WPB][FT_W];
    __shared__ uint8_t stg[WPB][2 * TK_B];
    const int lane = lane_id();
    uint8_t* sdec = tile[wave_in_block()];
    uint8_t* fw = fin[wave_in_block()];
    uint8_t* st = stg[wave_in_block()];
    const FetchTile T = fetch_tile(A);
    if (T.w0 >= T.fend) return;
    fetch_spans<COHORT>(A, T, [&](const DcCohortEntry& E, int64_t j0, int64_t j1, bool rev, int64_t j, int k0, int k1) {
        const FetchSpan sp = fetch_decode_span(E.S, j0, j1, sdec, st);
        const int64_t nlr = ENC == FE_ASCII && !A.upper ? E.nlr : 0;
        const int64_t rl0 = first_lower_run(E, nlr, j0);
        if (k0 < k1) fetch_enc_walk<ENC>(E, nlr, sdec, fw + lane * OPT, j, sp.rn0, rl0, sp.d0, rev, k0, k1);
    });
    // fin[w0 - base, fend - base) is complete
    fetch_enc_stream<ENC, DT>(fw, T.base, T.w0, T.fend, A.elemwise, reinterpret_cast<uint8_t*>(A.out), lane);
}

// ---------------------------------------------------------------------------------------------
// Origin fetch (SCCG_ENC_ORIGIN): k_fetch_enc's geometry -- a wave owns FT_W bases -- with one int32
// per base saying where the base comes from: the position in the reference sequence R a token copied
// it from, -1 for a literal of the record line, -2 for a base of one of the target's N runs.
// fetch_decode_span<true> leaves R positions (or -1) in the wave's int32 tile, mapped from R' once per
// token piece (origin_piece); R' itself is never loaded.  A lane walks its bases through the target's
// N runs as fetch_enc_walk does and places each value.  The finished tile streams out as
// k_fetch_enc's does: 16-byte pieces of 4 bases, piece q to lane q % 64, element stores for the
// pieces the tile's ends cut.
// LDS per block: WPB x (2 x FO_TILE x 4 + 2 x TK_B) = 35,328 bytes -> 4 blocks of a CU's 160 KiB,
// 16 waves per CU, 4 per SIMD.
// ---------------------------------------------------------------------------------------------
// A lane's bases of one span: positions j, j + 1, ... through the target's N runs from rn, each
// origin at its output place mine[k0, k1) (opad'ed from the lane's first entry m0) -- descending for
// a reversed span; the value itself is the same on either strand.
__device__ __forceinline__ void fetch_origin_walk(const DcCohortEntry& E, const int32_t* org, int32_t* fw, int m0, int64_t j,
                                                  int64_t rn, int64_t d0, bool rev, int k0, int k1) {
    NCursor N(E, rn);
    for (int t = 0; t < k1 - k0; t++) {
        N.seek(j);
        const int32_t v = j < N.s ? org[opad((int)(j - N.b - d0))] : -2;
        j++;
        fw[opad(m0 + (rev ? k1 - 1 - t : k0 + t))] = v;
    }
}

template <bool COHORT>
__global__ __launch_bounds__(SCCG_BLOCK) void k_fetch_origin(const FetchArgs A) {
    __shared__ int32_t tile[WPB][FO_TILE];
    __shared__ int32_t fin[WPB][FO_TILE];
    __shared__ uint8_t stg[WPB][2 * TK_B];
    const int lane = lane_id();
    int32_t* org = tile[wave_in_block()];
    int32_t* fw = fin[wave_in_block()];
    uint8_t* st = stg[wave_in_block()];
    const FetchTile T = fetch_tile(A);
    const int64_t base = T.base, w0 = T.w0, fend = T.fend;
    if (w0 >= fend) return;
    MapCur mc{0, INT64_MAX, INT64_MAX, 0};   // (no bracket yet: the first piece searches)
    const int32_t* mc_of = nullptr;          // the map mc brackets (the readers of one shared reference have one)
    fetch_spans<COHORT>(A, T, [&](const DcCohortEntry& E, int64_t j0, int64_t j1, bool rev, int64_t j, int k0, int k1) {
        if (E.S.rm.start != mc_of) {
            mc = MapCur{0, INT64_MAX, INT64_MAX, 0};
            mc_of = E.S.rm.start;
        }
        const FetchSpan sp = fetch_decode_span<true>(E.S, j0, j1, reinterpret_cast<uint8_t*>(org), st, &mc);
        if (k0 < k1) fetch_origin_walk(E, org, fw, lane * OPT, j, sp.rn0, sp.d0, rev, k0, k1);
    });
    // fin[w0 - base, fend - base) is complete
    int32_t* out = reinterpret_cast<int32_t*>(A.out);
    for (int it = 0; it < 4 * (FT_W / 256); it++) {
        const int q = it * 64 + lane;
        const int64_t p0 = base + (int64_t)q * 4;   // the piece's first base
        if (p0 >= fend || p0 + 4 <= w0) continue;
        int32_t w[4];
#pragma unroll
        for (int t = 0; t < 4; t++) w[t] = fw[opad(q * 4 + t)];
        int32_t* dst = out + p0;
        if (p0 >= w0 && p0 + 4 <= fend) {
            *reinterpret_cast<int4*>(dst) = make_int4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (p0 + t >= w0 && p0 + t < fend) dst[t] = w[t];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Find (sccg_*_find*): where an IUPAC pattern of m <= 64 letters occurs in the regions, on either
// strand.  The fetch kernels' front with another flat space and another epilogue: the flat space is
// counted in candidate starts -- region i owns max(0, len_i - m + 1) of them, so a window never
// crosses its region's end -- and a wave owns FD_TILE = 960 consecutive ones, a lane 16, as
// fetch_spans hands them out.  For each span of starts [j0, j1) the wave decodes the window
// [j0, j1 + m - 1), at most FD_TILE + 63 <= FT_W positions, through fetch_decode_span into its LDS
// tile; nothing of it goes to memory.
//   pack    lane l walks positions j0 + 16 l .. + 15 through the target's N runs (NCursor) and packs
//           their one-hot nibbles -- A 1, C 2, G 4, T 8, every other byte and every N 0 -- into one
//           64-bit word of the wave's LDS, position j0 + s at nibble s % 16 of word s / 16.
//   match   the pattern is up to four words of mask nibbles per strand (the reverse strand's: the
//           masks reversed and complemented, so a reverse hit is a forward match of that pattern at
//           the same position), in the kernel arguments.  A lane loads the six words around its
//           first start, shifts them to that start, and for each of its starts r shifts by r more
//           nibbles (constant shifts): a stretch of 16 letters matches iff no nibble of `seq & mask`
//           is zero among the pattern's letters -- one AND, three shift-ORs and a compare a word.
//           A lane's hits are two bits per start: forward at bit k, reverse at bit 16 + k of one
//           32-bit word for its 16 flat slots, kept in a register across the tile's spans.
//   k_find_count  leaves that word per lane (256 bytes a tile: 2 bits per candidate, against the
//           byte per base an index fetch writes) and the tile's hit count; sg_scan makes the counts
//           offsets; k_find_write expands the words -- the spans again for the positions, no decode
//           -- into rows {pos, strand} in flat order, which is the order asked for: ascending pos
//           within a region, forward before reverse.  off[i] = the hits before the region's first
//           candidate, read from the same words by a thread per region, so regions that own no
//           candidate (empty, shorter than m) get theirs like every other: the hits before flat
//           position pre[i], or the total when pre[i] is the end of the space.
// LDS per block: WPB x (FT_W + FD_WORDS x 8 + 2 x TK_B) = 6,912 bytes; k_find_count's 88 VGPRs, not
// LDS, set its occupancy: 5 waves per SIMD.  Every loop is bounded by a data size; no wave waits for another.
// ---------------------------------------------------------------------------------------------
constexpr int FD_MAXM = SCCG_FIND_MAX_PATTERN;
constexpr int FD_TILE = (FT_W - (FD_MAXM - 1)) / OPT * OPT;   // candidate starts of a wave: whole lanes of OPT
constexpr int FD_WORDS = FT_W / 16 + 8;                       // packed words of a window, and the six a lane loads past its own
static_assert(OPT == 16, "a lane's starts are one 16-bit mask a strand, its bases one 64-bit word");
static_assert(FD_TILE + FD_MAXM - 1 <= FT_W, "a span's window fits fetch_decode_span's bound and the LDS tile");
static_assert(FD_TILE / 16 + 6 <= FD_WORDS, "the words a lane loads exist");

struct FindArgs {
    FetchArgs F;                        // pre: the prefix of the regions' candidates, F.F all of them; forward, no out
    uint64_t pf[4], pr[4], lm[4];       // mask nibbles of the pattern, of its reverse complement; 1 per letter
    int32_t m, nw;                      // letters, words holding them
    uint32_t fwd, rev;                  // strands searched
    int64_t W;                          // tiles (>= 1)
    uint32_t* bits;                     // W * 64: a lane's hits
    int64_t* wcnt;                      // W: hits per tile (the count)
    int64_t* woff;                      // W + 1: their exclusive prefix (the scan's output, the write's input)
    int64_t* off;                       // nreg + 1 or null
    sccg_hit* hit;
    int64_t cap;
};

// nibbles [nib, nib + 16) of hi:lo
__device__ __forceinline__ uint64_t nib_shr(uint64_t lo, uint64_t hi, int nib) {
    return nib ? (lo >> (4 * nib)) | (hi << (64 - 4 * nib)) : lo;
}
// bit 0 of every nibble that is not zero
__device__ __forceinline__ uint64_t nib_any(uint64_t x) {
    x |= x >> 1;
    x |= x >> 2;
    return x & 0x1111111111111111ull;
}

__device__ __forceinline__ FetchTile find_tile(const FindArgs& A, int64_t w) {
    const int64_t base = w * FD_TILE;
    return FetchTile{base, base, base + FD_TILE < A.F.F ? base + FD_TILE : A.F.F};
}

template <bool COHORT>
__global__ __launch_bounds__(SCCG_BLOCK) void k_find_count(const FindArgs A) {
    __shared__ uint8_t tile[WPB][FT_W];
    __shared__ uint64_t pack[WPB][FD_WORDS];
    __shared__ uint8_t stg[WPB][2 * TK_B];
    const int64_t w = (int64_t)blockIdx.x * WPB + wave_in_block();
    if (w >= A.W) return;
    const int lane = lane_id();
    uint8_t* sdec = tile[wave_in_block()];
    uint64_t* pk = pack[wave_in_block()];
    uint8_t* st = stg[wave_in_block()];
    const FetchTile T = find_tile(A, w);
    if (lane < FD_WORDS - 64) pk[64 + lane] = 0;   // (read by the last lanes, masked by the pattern's end)
    uint32_t bits = 0;
    if (T.w0 < T.fend)
        fetch_spans<COHORT>(A.F, T, [&](const DcCohortEntry& E, int64_t j0, int64_t j1, bool, int64_t j, int k0, int k1) {
            const int64_t je = j1 + (A.m - 1);   // <= the region's end: j1 - 1 is a candidate
            const FetchSpan sp = fetch_decode_span(E.S, j0, je, sdec, st);
            int64_t q = j0 + (int64_t)lane * 16;
            uint64_t word = 0;
            if (q < je) {
                NCursor N(E, sp.rn0);
                const int cnt = je - q < 16 ? (int)(je - q) : 16;
                for (int t = 0; t < cnt; t++) {
                    N.seek(q);
                    const uint32_t c = q >= N.s ? 4u : base_code(sdec[q - N.b - sp.d0]);
                    if (c < 4u) word |= (uint64_t)(1u << c) << (4 * t);
                    q++;
                }
            }
            pk[lane] = word;
            wave_sync();
            if (k0 < k1) {
                const int s0 = (int)(j - j0), a = s0 >> 4, sh = s0 & 15, cnt = k1 - k0;
                uint64_t raw[6], v[5];
#pragma unroll
                for (int k = 0; k < 6; k++) raw[k] = pk[a + k];
#pragma unroll
                for (int k = 0; k < 5; k++) v[k] = nib_shr(raw[k], raw[k + 1], sh);
                uint32_t hf = 0, hr = 0;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    bool f = A.fwd != 0, rv = A.rev != 0;
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k < A.nw) {
                            const uint64_t x = nib_shr(v[k], v[k + 1], r);
                            f = f && nib_any(x & A.pf[k]) == A.lm[k];
                            rv = rv && nib_any(x & A.pr[k]) == A.lm[k];
                        }
                    if (r < cnt) {
                        hf |= (uint32_t)f << r;
                        hr |= (uint32_t)rv << r;
                    }
                }
                bits |= (hf << k0) | (hr << (16 + k0));
            }
        });
    A.bits[w * 64 + lane] = bits;
    const int64_t total = wave_sum((int64_t)__popc(bits));
    if (lane == 0) A.wcnt[w] = total;
}

template <bool COHORT>
__global__ __launch_bounds__(SCCG_BLOCK) void k_find_write(const FindArgs A) {
    // the regions' offsets: the hits before flat position pre[i]
    if (A.off) {
        const int64_t total = A.woff[A.W];
        for (int64_t i = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x; i <= A.F.nreg; i += (int64_t)gridDim.x * SCCG_BLOCK) {
            const int64_t f = A.F.pre[i];
            int64_t o = total;
            if (f < A.F.F) {
                const int64_t w = f / FD_TILE;
                const int sl = (int)(f - w * FD_TILE);
                const uint32_t* __restrict__ b = A.bits + w * 64;
                o = A.woff[w];
                for (int l = 0; l < (sl >> 4); l++) o += __popc(b[l]);
                const uint32_t low = (1u << (sl & 15)) - 1u;
                o += __popc(b[sl >> 4] & (low | (low << 16)));
            }
            A.off[i] = o;
        }
    }
    const int64_t w = (int64_t)blockIdx.x * WPB + wave_in_block();
    if (w >= A.W) return;
    const FetchTile T = find_tile(A, w);
    if (T.w0 >= T.fend) return;
    const uint32_t bits = A.bits[w * 64 + lane_id()];
    const uint32_t c = (uint32_t)__popc(bits);
    int64_t o = A.woff[w] + (wave_incl_add_dpp(c) - c);   // the lane's first row
    if (!__ballot(c != 0)) return;
    sccg_hit* __restrict__ hit = A.hit;
    const int64_t cap = A.cap;
    fetch_spans<COHORT>(A.F, T, [&](const DcCohortEntry&, int64_t, int64_t, bool, int64_t j, int k0, int k1) {
        if (k0 >= k1) return;
        uint32_t mk = (bits | (bits >> 16)) & ((1u << k1) - (1u << k0));   // the span's slots with a hit
        while (mk) {
            const int k = __ffs((int)mk) - 1;
            mk &= mk - 1;
            const int64_t pos = j + (k - k0);
            if ((bits >> k) & 1u) {
                if (o < cap) hit[o] = sccg_hit{pos, 0};
                o++;
            }
            if ((bits >> (16 + k)) & 1u) {
                if (o < cap) hit[o] = sccg_hit{pos, 1};
                o++;
            }
        }
    });
}

// ---------------------------------------------------------------------------------------------
// Find with mismatches (sccg_*_find_approx*): the hits within K <= SCCG_FIND_MAX_MISMATCHES substitutions.
// Find's geometry, front and scan with another match and a third column; the exact kernels above are
// left as they are, so what sccg_*_find* launches does not change.
//   match   nib_any(x & mask) has bit 0 of a nibble for every letter that matches and is a subset of
//           lm (a letter's mask is never zero), so the letters that do not are lm ^ that word and a
//           start's distance is its population count summed over the pattern's words: two v_bcnt a word
//           and strand where the exact kernel compares, no branch.  A base of code 4 packs as nibble 0
//           and so mismatches every letter, N included.  So do the zero nibbles beyond a span's window
//           [j0, je), but no start the gate `r < cnt` lets through sees them: a lane's cnt starts are
//           starts of the span, j < j1, and their last letter is at j + m - 1 <= j1 + m - 2 = je - 1.
//   k_find_mm_count  leaves Find's hit word per lane and, beside it, two 64-bit words of 4-bit
//           distances, one per strand, nibble r for the lane's flat slot r; a nibble is the distance
//           where the hit bit is set (d <= K <= 15) and 0 elsewhere.  All three are kept in registers
//           across the tile's spans and stored once.  Scratch: 34 + 128 words of 8 bytes a tile of 960
//           candidates, 1.35 bytes a candidate.
//   k_find_mm_write  k_find_write's walk over the hit word -- no decode -- storing {pos, strand, d};
//           the regions' offsets come from the hit words exactly as there.
// LDS per block: k_find_count's 6,912 bytes.  Every loop is bounded by a data size or a constant; no
// wave waits for another; plain vector stores.
// ---------------------------------------------------------------------------------------------
struct FindMmArgs {
    FindArgs B;        // Find's arguments; B.hit is not used
    uint32_t K;        // mismatches allowed, <= SCCG_FIND_MAX_MISMATCHES
    uint64_t* dist;    // W * 64 * 2: a lane's distances, forward then reverse
    sccg_hit_mm* hit;
};
static_assert(SCCG_FIND_MAX_MISMATCHES <= 15, "a distance is one nibble");

template <bool COHORT>
__global__ __launch_bounds__(SCCG_BLOCK) void k_find_mm_count(const FindMmArgs M) {
    __shared__ uint8_t tile[WPB][FT_W];
    __shared__ uint64_t pack[WPB][FD_WORDS];
    __shared__ uint8_t stg[WPB][2 * TK_B];
    const FindArgs& A = M.B;
    const int64_t w = (int64_t)blockIdx.x * WPB + wave_in_block();
    if (w >= A.W) return;
    const int lane = lane_id();
    uint8_t* sdec = tile[wave_in_block()];
    uint64_t* pk = pack[wave_in_block()];
    uint8_t* st = stg[wave_in_block()];
    const FetchTile T = find_tile(A, w);
    if (lane < FD_WORDS - 64) pk[64 + lane] = 0;   // (read by the last lanes' starts beyond cnt only)
    uint32_t bits = 0;
    uint64_t df = 0, dr = 0;
    if (T.w0 < T.fend)
        fetch_spans<COHORT>(A.F, T, [&](const DcCohortEntry& E, int64_t j0, int64_t j1, bool, int64_t j, int k0, int k1) {
            const int64_t je = j1 + (A.m - 1);   // <= the region's end: j1 - 1 is a candidate
            const FetchSpan sp = fetch_decode_span(E.S, j0, je, sdec, st);
            int64_t q = j0 + (int64_t)lane * 16;
            uint64_t word = 0;
            if (q < je) {
                NCursor N(E, sp.rn0);
                const int cnt = je - q < 16 ? (int)(je - q) : 16;
                for (int t = 0; t < cnt; t++) {
                    N.seek(q);
                    const uint32_t c = q >= N.s ? 4u : base_code(sdec[q - N.b - sp.d0]);
                    if (c < 4u) word |= (uint64_t)(1u << c) << (4 * t);
                    q++;
                }
            }
            pk[lane] = word;
            wave_sync();
            if (k0 < k1) {
                const int s0 = (int)(j - j0), a = s0 >> 4, sh = s0 & 15, cnt = k1 - k0;
                uint64_t raw[6], v[5];
#pragma unroll
                for (int k = 0; k < 6; k++) raw[k] = pk[a + k];
#pragma unroll
                for (int k = 0; k < 5; k++) v[k] = nib_shr(raw[k], raw[k + 1], sh);
                uint32_t hf = 0, hr = 0;
                uint64_t nf = 0, nr = 0;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    uint32_t f = 0, rv = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (k < A.nw) {
                            const uint64_t x = nib_shr(v[k], v[k + 1], r);
                            f += (uint32_t)__popcll(A.lm[k] ^ nib_any(x & A.pf[k]));
                            rv += (uint32_t)__popcll(A.lm[k] ^ nib_any(x & A.pr[k]));
                        }
                    const bool isf = A.fwd != 0 && f <= M.K && r < cnt, isr = A.rev != 0 && rv <= M.K && r < cnt;
                    hf |= (uint32_t)isf << r;
                    hr |= (uint32_t)isr << r;
                    nf |= (uint64_t)(isf ? f : 0u) << (4 * r);
                    nr |= (uint64_t)(isr ? rv : 0u) << (4 * r);
                }
                // slot k0 + r: the nibbles shifted out are those of r >= 16 - k0 >= cnt, all zero
                bits |= (hf << k0) | (hr << (16 + k0));
                df |= nf << (4 * k0);
                dr |= nr << (4 * k0);
            }
        });
    A.bits[w * 64 + lane] = bits;
    reinterpret_cast<ulonglong2*>(M.dist)[w * 64 + lane] = make_ulonglong2(df, dr);
    const int64_t total = wave_sum((int64_t)__popc(bits));
    if (lane == 0) A.wcnt[w] = total;
}

template <bool COHORT>
__global__ __launch_bounds__(SCCG_BLOCK) void k_find_mm_write(const FindMmArgs M) {
    const FindArgs& A = M.B;
    // the regions' offsets: the hits before flat position pre[i]
    if (A.off) {
        const int64_t total = A.woff[A.W];
        for (int64_t i = (int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x; i <= A.F.nreg; i += (int64_t)gridDim.x * SCCG_BLOCK) {
            const int64_t f = A.F.pre[i];
            int64_t o = total;
            if (f < A.F.F) {
                const int64_t w = f / FD_TILE;
                const int sl = (int)(f - w * FD_TILE);
                const uint32_t* __restrict__ b = A.bits + w * 64;
                o = A.woff[w];
                for (int l = 0; l < (sl >> 4); l++) o += __popc(b[l]);
                const uint32_t low = (1u << (sl & 15)) - 1u;
                o += __popc(b[sl >> 4] & (low | (low << 16)));
            }
            A.off[i] = o;
        }
    }
    const int64_t w = (int64_t)blockIdx.x * WPB + wave_in_block();
    if (w >= A.W) return;
    const FetchTile T = find_tile(A, w);
    if (T.w0 >= T.fend) return;
    const uint32_t bits = A.bits[w * 64 + lane_id()];
    const uint32_t c = (uint32_t)__popc(bits);
    int64_t o = A.woff[w] + (wave_incl_add_dpp(c) - c);   // the lane's first row
    if (!__ballot(c != 0)) return;
    const ulonglong2 d = reinterpret_cast<const ulonglong2*>(M.dist)[w * 64 + lane_id()];
    sccg_hit_mm* __restrict__ hit = M.hit;
    const int64_t cap = A.cap;
    fetch_spans<COHORT>(A.F, T, [&](const DcCohortEntry&, int64_t, int64_t, bool, int64_t j, int k0, int k1) {
        if (k0 >= k1) return;
        uint32_t mk = (bits | (bits >> 16)) & ((1u << k1) - (1u << k0));   // the span's slots with a hit
        while (mk) {
            const int k = __ffs((int)mk) - 1;
            mk &= mk - 1;
            const int64_t pos = j + (k - k0);
            if ((bits >> k) & 1u) {
                if (o < cap) hit[o] = sccg_hit_mm{pos, 0, (int64_t)((d.x >> (4 * k)) & 15u)};
                o++;
            }
            if ((bits >> (16 + k)) & 1u) {
                if (o < cap) hit[o] = sccg_hit_mm{pos, 1, (int64_t)((d.y >> (4 * k)) & 15u)};
                o++;
            }
        }
    });
}

// ---------------------------------------------------------------------------------------------
// The R' -> R map of a shared reference: the maximal runs of the byte 'N' (uppercase only: a
// lowercase 'n' survives into R' as "N", decompression.cpp:108 before :110) in the stripped,
// original-case reference R.  A block takes RM_TILE bytes, a thread 16 of them in one load; a run
// starts where an 'N' follows another byte and ends where another byte follows it, so starts and
// ends are counted per tile, ranked by two prefix sums over the tiles and written in a second pass
// (start k pairs with end k), whatever the runs' lengths are.
// ---------------------------------------------------------------------------------------------
constexpr int RM_PER = 16, RM_TILE = SCCG_BLOCK * RM_PER;

// bit k of st / en: byte i0 + k of R starts / ends a run
__device__ __forceinline__ void refn_events(const uint8_t* __restrict__ R, int64_t n, int64_t i0, uint32_t& st, uint32_t& en) {
    st = en = 0;
    if (i0 >= n) return;
    const uint4 x = load16u(R + i0);   // (past n: R carries the slack)
    const uint32_t w4[4] = {x.x, x.y, x.z, x.w};
    uint32_t isn = 0;
#pragma unroll
    for (int k = 0; k < RM_PER; k++)
        if (i0 + k < n && (uint8_t)(w4[k >> 2] >> (8 * (k & 3))) == 'N') isn |= 1u << k;
    const uint32_t prev = i0 > 0 && R[i0 - 1] == 'N', next = i0 + RM_PER < n && R[i0 + RM_PER] == 'N';
    st = isn & ~((isn << 1) | prev);
    en = isn & ~((isn >> 1) | (next << (RM_PER - 1)));
}

__global__ __launch_bounds__(SCCG_BLOCK) void k_refn_count(const uint8_t* __restrict__ R, int64_t n, int64_t* __restrict__ cs,
                                                           int64_t* __restrict__ ce) {
    __shared__ int64_t tmp[5];
    uint32_t st, en;
    refn_events(R, n, ((int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x) * RM_PER, st, en);
    int64_t ts = 0, te = 0;
    block_excl_add<int64_t>(__popc(st), tmp, &ts);
    block_excl_add<int64_t>(__popc(en), tmp, &te);
    if (threadIdx.x == 0) {
        cs[blockIdx.x] = ts;
        ce[blockIdx.x] = te;
    }
}

// start[k] = the k-th run's first byte, end[k] = its last (inclusive); os / oe: the tiles' ranks
__global__ __launch_bounds__(SCCG_BLOCK) void k_refn_write(const uint8_t* __restrict__ R, int64_t n, const int64_t* __restrict__ os,
                                                           const int64_t* __restrict__ oe, int64_t nruns,
                                                           int32_t* __restrict__ start, int32_t* __restrict__ end) {
    __shared__ int64_t tmp[5];
    uint32_t st, en;
    const int64_t i0 = ((int64_t)blockIdx.x * SCCG_BLOCK + threadIdx.x) * RM_PER;
    refn_events(R, n, i0, st, en);
    int64_t rs = os[blockIdx.x] + block_excl_add<int64_t>(__popc(st), tmp, nullptr);
    int64_t re = oe[blockIdx.x] + block_excl_add<int64_t>(__popc(en), tmp, nullptr);
    for (; st; st &= st - 1, rs++)
        if (rs < nruns) start[rs] = (int32_t)(i0 + __ffs((int)st) - 1);
    for (; en; en &= en - 1, re++)
        if (re < nruns) end[re] = (int32_t)(i0 + __ffs((int)en) - 1);
}

// len[k] <- end[k] - start[k] + 1 (len holds the ends on entry), cum[k] <- the same, to be summed
__global__ void k_refn_len(const int32_t* __restrict__ start, int32_t* __restrict__ len, int64_t* __restrict__ cum, int64_t nruns) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nruns; k += (int64_t)gridDim.x * blockDim.x) {
        const int32_t l = len[k] - start[k] + 1;
        len[k] = l;
        cum[k] = l;
    }
}

}  // namespace

// =============================================================================================
int64_t dc_refmap_tiles(int64_t n) { return n > 0 ? (n + RM_TILE - 1) / RM_TILE : 0; }

int dc_refmap_count(const uint8_t* d_R, int64_t n, int64_t* d_cs, int64_t* d_ce, int64_t* d_os, int64_t* d_oe, int64_t* d_nruns,
                    int64_t* d_partial, hipStream_t s) {
    const int64_t nt = dc_refmap_tiles(n);
    if (!nt) {
        SCCG_HIP(hipMemsetAsync(d_nruns, 0, 2 * sizeof(int64_t), s));
        return 0;
    }
    hipLaunchKernelGGL(k_refn_count, dim3((unsigned)nt), dim3(SCCG_BLOCK), 0, s, d_R, n, d_cs, d_ce);
    SCCG_HIP(hipGetLastError());
    return dev_excl_sum2(d_cs, d_os, d_nruns, d_ce, d_oe, d_nruns + 1, nt, d_partial, s);
}

int dc_refmap_write(const uint8_t* d_R, int64_t n, const int64_t* d_os, const int64_t* d_oe, DcRuns* m, int64_t* d_total,
                    int64_t* d_partial, hipStream_t s) {
    if (m->n <= 0) return 0;
    hipLaunchKernelGGL(k_refn_write, dim3((unsigned)dc_refmap_tiles(n)), dim3(SCCG_BLOCK), 0, s, d_R, n, d_os, d_oe, m->n, m->start,
                       m->len);
    const unsigned g = grid_for(m->n, 256) > 4096 ? 4096 : grid_for(m->n, 256);
    hipLaunchKernelGGL(k_refn_len, dim3(g), dim3(256), 0, s, (const int32_t*)m->start, m->len, m->cum, m->n);
    SCCG_HIP(hipGetLastError());
    return dev_excl_sum(m->cum, m->cum, m->n, d_total, d_partial, s);
}

int dc_find_lines(const uint8_t* d_rec, int64_t n, int64_t* d_nl /*8: 4 results + 4 tickets*/, hipStream_t s) {
    for (int i = 0; i < 4; i++) {
        int rc = launch_first_match(d_rec, n, i ? (const int64_t*)(d_nl + i - 1) : nullptr, 1, '\n', d_nl + i, d_nl + 4 + i, s);
        if (rc) return rc;
    }
    return 0;
}

namespace {
__global__ void k_nl_init(int64_t* cnt, int32_t* err) {
    if (threadIdx.x == 0) {
        *cnt = 0;
        if (err) *err = 0;
    }
}
}  // namespace

int dc_newlines(const uint8_t* d_rec, int64_t n, int64_t* d_buf, hipStream_t s, int32_t* d_err) {
    hipLaunchKernelGGL(k_nl_init, dim3(1), dim3(64), 0, s, d_buf, d_err);   // (one launch zeroes both)
    SCCG_HIP(hipGetLastError());
    if (n <= 0) return 0;
    const unsigned g = grid_for(n, 256) > 4096 ? 4096 : grid_for(n, 256);
    hipLaunchKernelGGL(k_newlines, dim3(g), dim3(256), 0, s, d_rec, n, reinterpret_cast<unsigned long long*>(d_buf), d_buf + 1);
    SCCG_HIP(hipGetLastError());
    return 0;
}

int dc_last_paren(const uint8_t* d_s, int64_t n, int64_t* d_lp, int64_t* d_partial, hipStream_t s) {
    if (n <= 0) return 0;
    const unsigned g = grid_for(n, 256) > 8192 ? 8192 : grid_for(n, 256);
    hipLaunchKernelGGL(k_paren_pos, dim3(g), dim3(256), 0, s, d_s, n, d_lp);
    SCCG_HIP(hipGetLastError());
    // exclusive max-scan: last parenthesis strictly before i; the inclusive form is not needed
    return dev_excl_max(d_lp, d_lp, n, nullptr, d_partial, s);
}

int64_t dc_run_cap(int64_t n) { return n / 2 + 2; }

namespace {
bool rl_tiled_ok(int64_t n) { return (n + RL_TILE - 1) / RL_TILE <= 64 * 1024; }

// the scan-based parser of one line (lines of more than 64 Ki tiles)
int parse_runs_scan(const uint8_t* d_s, int64_t n, DcRuns* r, int64_t* d_lp, int64_t* d_flag, int64_t* d_dlt,
                    int64_t* d_partial, int32_t* d_err, int64_t* d_count, hipStream_t s) {
    if (n <= 0) {
        SCCG_HIP(hipMemsetAsync(d_count, 0, 2 * sizeof(int64_t), s));
        return 0;
    }
    const int64_t cap = dc_run_cap(n);
    int rc = dc_last_paren(d_s, n, d_lp, d_partial, s);
    if (rc) return rc;
    SCCG_HIP(hipMemsetAsync(d_dlt, 0, (size_t)cap * sizeof(int64_t), s));   // deltas past the runs scan as 0
    const unsigned g = grid_for(n, 256) > 8192 ? 8192 : grid_for(n, 256);
    hipLaunchKernelGGL(k_run_items_flag, dim3(g), dim3(256), 0, s, d_s, n, (const int64_t*)d_lp, d_flag, d_err);
    rc = dev_excl_sum(d_flag, d_flag, n, d_count, d_partial, s);   // item ranks; d_count[0] = runs
    if (rc) return rc;
    hipLaunchKernelGGL(k_run_items_parse, dim3(g), dim3(256), 0, s, d_s, n, (const int64_t*)d_lp,
                       (const int64_t*)d_flag, d_dlt, r->len, d_err);
    SCCG_HIP(hipGetLastError());
    // exclusive sum of deltas into d_flag (free now), then starts and int64 lengths, then the
    // N-count prefix; d_count[1] = total run length
    rc = dev_excl_sum(d_dlt, d_flag, cap, nullptr, d_partial, s);
    if (rc) return rc;
    const unsigned g2 = grid_for(cap, 256) > 8192 ? 8192 : grid_for(cap, 256);
    hipLaunchKernelGGL(k_run_finish, dim3(g2), dim3(256), 0, s, (const int64_t*)d_flag, (const int64_t*)d_dlt,
                       (const int32_t*)r->len, cap, (const int64_t*)d_count, r->start, r->cum, d_err);
    SCCG_HIP(hipGetLastError());
    return dev_excl_sum(r->cum, r->cum, cap, d_count + 1, d_partial, s);
}

RlJob rl_job_of(const uint8_t* d_s, int64_t n, DcRuns* r, int64_t* tsum, int64_t* d_count) {
    return RlJob{d_s, n > 0 ? n : 0, n > 0 ? (n + RL_TILE - 1) / RL_TILE : 0, tsum, r->start, r->len, r->cum, d_count};
}

int parse_runs_tiled(const RlJob& j0, const RlJob& j1, int32_t* d_err, hipStream_t s) {
    const int64_t nt = j0.ntiles + j1.ntiles;
    if (nt > 0) {
        const unsigned g = (unsigned)((nt + 3) / 4);
        hipLaunchKernelGGL(k_rl_tiles, dim3(g), dim3(256), 0, s, j0, j1, d_err);
        hipLaunchKernelGGL(k_rl_scan, dim3(2), dim3(RL_SCAN_T), 0, s, j0, j1);
        hipLaunchKernelGGL(k_rl_write, dim3(g), dim3(256), 0, s, j0, j1, d_err);
    } else {
        hipLaunchKernelGGL(k_rl_scan, dim3(2), dim3(RL_SCAN_T), 0, s, j0, j1);   // (zero counts)
    }
    SCCG_HIP(hipGetLastError());
    return 0;
}
}  // namespace

int dc_parse_runs(const uint8_t* d_s, int64_t n, DcRuns* r, int64_t* d_lp, int64_t* d_flag, int64_t* d_dlt,
                  int64_t* d_partial, int32_t* d_err, int64_t* d_count, hipStream_t s) {
    if (n > 0 && rl_tiled_ok(n)) {   // tiled: d_flag holds the per-tile summaries (4 per tile)
        DcRuns none{};
        return parse_runs_tiled(rl_job_of(d_s, n, r, d_flag, d_count), rl_job_of(nullptr, 0, &none, nullptr, nullptr), d_err, s);
    }
    return parse_runs_scan(d_s, n, r, d_lp, d_flag, d_dlt, d_partial, d_err, d_count, s);
}

int dc_parse_runs2(const uint8_t* s0, int64_t n0, DcRuns* r0, int64_t* d_count0, const uint8_t* s1, int64_t n1, DcRuns* r1,
                   int64_t* d_count1, int64_t* d_lp, int64_t* d_flag, int64_t* d_dlt, int64_t* d_partial, int32_t* d_err,
                   hipStream_t s) {
    if (rl_tiled_ok(n0) && rl_tiled_ok(n1))   // both lines in one launch set; summaries in d_flag / d_dlt
        return parse_runs_tiled(rl_job_of(s0, n0, r0, d_flag, d_count0), rl_job_of(s1, n1, r1, d_dlt, d_count1), d_err, s);
    int rc = dc_parse_runs(s0, n0, r0, d_lp, d_flag, d_dlt, d_partial, d_err, d_count0, s);
    if (!rc) rc = dc_parse_runs(s1, n1, r1, d_lp, d_flag, d_dlt, d_partial, d_err, d_count1, s);
    return rc;
}

int dc_n_check(const DcRuns& nr, const int64_t* d_ncnt, const int64_t* d_D, int32_t* d_err, hipStream_t s) {
    hipLaunchKernelGGL(k_n_check, dim3(1), dim3(64), 0, s, (const int32_t*)nr.start, (const int32_t*)nr.len, d_ncnt, d_D,
                       d_err);
    SCCG_HIP(hipGetLastError());
    return 0;
}

int dc_decode_prepare(const uint8_t* d_s, int64_t n, int64_t* d_lp, int64_t* d_contrib, int64_t* d_dlt, int64_t* d_off,
                      int64_t* d_dsum, int64_t* d_partial, int32_t* d_err, int64_t* d_total, hipStream_t s) {
    if (n <= 0) {
        SCCG_HIP(hipMemsetAsync(d_total, 0, sizeof(int64_t), s));
        return 0;
    }
    // per 64-byte block: state, output bytes, deltas; their exclusive prefixes -> d_off, d_dsum
    const int64_t nb = (n + TK_B - 1) / TK_B;
    const unsigned g = (unsigned)((n + 4 * 1024 - 1) / (4 * 1024));   // 4 waves of 1 KiB per block
    hipLaunchKernelGGL(k_tok_blocks, dim3(g), dim3(256), 0, s, d_s, n, d_lp, d_contrib, d_dlt, d_err);
    SCCG_HIP(hipGetLastError());
    // (d_partial: scan_partials_needed(n + 1) + 16 >= 2 * scan_partials_needed(nb))
    return dev_excl_sum2(d_contrib, d_off, d_total, d_dlt, d_dsum, nullptr, nb, d_partial, s);
}

int dc_decode_fill(const uint8_t* d_s, int64_t n, const int64_t* d_lp, const int64_t* d_off, const int64_t* d_dsum,
                   const uint8_t* d_R, uint8_t* d_dec, hipStream_t s, const int64_t* d_nref, int32_t* d_err, int64_t dcap) {
    if (n <= 0) return 0;
    PROF_LAUNCH(PROF_DC_DECODE, s, k_tok_fill2<true>, dim3(grid_for((n + TK_B - 1) / TK_B, WPB)), dim3(SCCG_BLOCK), 0, s, d_s, n,
                d_lp, d_off, d_dsum, d_nref, d_R, d_dec, d_err, dcap);
    SCCG_HIP(hipGetLastError());
    return 0;
}

int dc_tok_range(const uint8_t* d_s, int64_t n, const int64_t* d_lp, const int64_t* d_off, const int64_t* d_dsum,
                 const int64_t* d_nref, int32_t* d_err, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_tok_fill2<false>, dim3(grid_for((n + TK_B - 1) / TK_B, WPB)), dim3(SCCG_BLOCK), 0, s, d_s, n, d_lp,
                       d_off, d_dsum, d_nref, (const uint8_t*)nullptr, (uint8_t*)nullptr, d_err, (int64_t)0);
    SCCG_HIP(hipGetLastError());
    return 0;
}

// (one table row per OB output bytes though a block formats FMT_U * OB: the size the workspace has
// always reserved; the output's misalignment adds a block)
int64_t dc_format_index_words(int64_t nres) { return TW * ((nres + nres / 50 + 16) / OB + 3); }

namespace {
struct FmtGeom {
    int64_t total, o_first, nblk;
};
FmtGeom fmt_geom(int64_t nres, const uint8_t* d_out) {
    FmtGeom g;
    g.total = nres + (nres - 1) / 50;   // the final '\n' is the caller's
    g.o_first = -(int64_t)((uintptr_t)d_out & 15);
    g.nblk = (g.total - g.o_first + FMT_U * OB - 1) / (FMT_U * OB);
    return g;
}
}  // namespace

int dc_format_index(int64_t nres, const DcRuns& nr, const DcRuns& lr, int64_t* d_index, uint8_t* d_out, hipStream_t s) {
    if (nres <= 0) return 0;
    const FmtGeom g = fmt_geom(nres, d_out);
    hipLaunchKernelGGL(k_out_index, dim3(grid_for(2 * (g.nblk + 1), 256)), dim3(256), 0, s, nres, g.total, g.o_first, g.nblk,
                       (int64_t)FMT_U * OB, (const int32_t*)nr.start, (const int32_t*)nr.len, (const int64_t*)nr.cum, nr.n,
                       (const int32_t*)lr.start, (const int32_t*)lr.len, lr.n, d_index);
    SCCG_HIP(hipGetLastError());
    return 0;
}

int dc_format(const uint8_t* d_dec, int64_t nres, const DcRuns& nr, const DcRuns& lr, const int64_t* d_index, uint8_t* d_out,
              hipStream_t s, hipEvent_t wait_before) {
    if (wait_before) SCCG_HIP(hipStreamWaitEvent(s, wait_before, 0));
    if (nres <= 0) return 0;
    const FmtGeom g = fmt_geom(nres, d_out);
    PROF_LAUNCH(PROF_DC_FORMAT, s, k_format_out, dim3((unsigned)g.nblk), dim3(256), 0, s, d_dec, nres, g.total, g.o_first,
                (const int32_t*)nr.start, (const int32_t*)nr.len, (const int64_t*)nr.cum, nr.n,
                (const int32_t*)lr.start, (const int32_t*)lr.len, lr.n, d_index, d_out);
    SCCG_HIP(hipGetLastError());
    return 0;
}

namespace {
// the kernel of a format (null: not a valid pair); COHORT: the source of each span from the table
template <bool COHORT>
void (*fetch_kernel(int enc, int dt))(FetchArgs) {
    if (enc == FE_ASCII && dt == FD_U8) return k_fetch_enc<FE_ASCII, FD_U8, COHORT>;
    if (enc == FE_INDEX && dt == FD_U8) return k_fetch_enc<FE_INDEX, FD_U8, COHORT>;
    if (enc == FE_ONEHOT && dt == FD_U8) return k_fetch_enc<FE_ONEHOT, FD_U8, COHORT>;
    if (enc == FE_ONEHOT && dt == FD_F16) return k_fetch_enc<FE_ONEHOT, FD_F16, COHORT>;
    if (enc == FE_ONEHOT && dt == FD_BF16) return k_fetch_enc<FE_ONEHOT, FD_BF16, COHORT>;
    if (enc == FE_ONEHOT && dt == FD_F32) return k_fetch_enc<FE_ONEHOT, FD_F32, COHORT>;
    if (enc == FE_ORIGIN && dt == FD_I32) return k_fetch_origin<COHORT>;
    return nullptr;
}
}  // namespace

int dc_fetch(const DcFetch& c, hipStream_t s) {
    if (c.F <= 0) return 0;
    void (*const kernel)(FetchArgs) = c.src ? fetch_kernel<false>(c.enc, c.dt) : fetch_kernel<true>(c.enc, c.dt);
    if (!kernel) return SCCG_E_INVALID;
    const uintptr_t at = (uintptr_t)c.d_out;
    const uintptr_t es = c.dt == FD_U8 ? 1 : c.dt == FD_F16 || c.dt == FD_BF16 ? 2 : 4;   // element bytes
    const uintptr_t bpb = c.enc == FE_ONEHOT ? 4 * es : c.enc == FE_ORIGIN ? es : 1;      // bytes per base
    if (c.enc == FE_ORIGIN && at % bpb) return SCCG_E_INVALID;
    // whole bases per 16-byte piece need d_out on a base boundary; else every store is an element's
    const bool elemwise = at % bpb != 0;
    FetchArgs A{};
    if (c.src) A.E = DcCohortEntry{*c.src, c.src->nr.n, c.src->lr.n, c.src->nr.total};
    A.tab = c.d_tab;
    A.pre = c.d_pre;
    A.beg = c.d_beg;
    A.samp = c.d_samp;
    A.nreg = c.nreg;
    A.F = c.F;
    A.o_first = elemwise ? 0 : -(int64_t)((at & 15) / bpb);
    A.all_rev = c.all_rev ? 1u : 0u;
    A.elemwise = elemwise ? 1u : 0u;
    A.upper = c.upper ? 1u : 0u;
    A.out = c.d_out;
    const int64_t nblk = (c.F - A.o_first + OB - 1) / OB;
    PROF_LAUNCH(PROF_FETCH, s, kernel, dim3((unsigned)nblk), dim3(SCCG_BLOCK), 0, s, A);
    SCCG_HIP(hipGetLastError());
    return 0;
}

namespace {
int64_t fd_tiles(int64_t F) { return F > 0 ? (F + FD_TILE - 1) / FD_TILE : 1; }

// scratch: W * 64 hit words (32 W int64), W counts, W + 1 offsets
FindArgs fd_args(const FdCall& c) {
    FindArgs A{};
    if (c.src) A.F.E = DcCohortEntry{*c.src, c.src->nr.n, c.src->lr.n, c.src->nr.total};
    A.F.tab = c.d_tab;
    A.F.pre = c.d_pre;
    A.F.beg = c.d_beg;
    A.F.samp = c.d_samp;
    A.F.nreg = c.nreg;
    A.F.F = c.F;
    for (int t = 0; t < c.m; t++) {
        A.pf[t >> 4] |= (uint64_t)(c.fwd[t] & 15) << (4 * (t & 15));
        A.pr[t >> 4] |= (uint64_t)(c.rev[t] & 15) << (4 * (t & 15));
        A.lm[t >> 4] |= 1ull << (4 * (t & 15));
    }
    A.m = c.m;
    A.nw = (c.m + 15) / 16;
    A.fwd = c.want_fwd ? 1u : 0u;
    A.rev = c.want_rev ? 1u : 0u;
    A.W = fd_tiles(c.F);
    int64_t* p = c.d_scratch;
    A.bits = reinterpret_cast<uint32_t*>(p); p += 32 * A.W;
    A.wcnt = p; p += A.W;
    A.woff = p;
    return A;
}
}  // namespace

int64_t fd_candidates(int64_t len, int m) { return len >= m ? len - m + 1 : 0; }
int64_t fd_scratch_words(int64_t F) { return 34 * fd_tiles(F) + 1; }

const int64_t* fd_total_slot(const FdCall& c) {
    const FindArgs A = fd_args(c);
    return A.woff + A.W;
}

int fd_count(const FdCall& c, hipStream_t s) {
    if (c.nreg <= 0 || c.m < 1 || c.m > FD_MAXM || c.F < 0) return SCCG_E_INVALID;
    const FindArgs A = fd_args(c);
    void (*const kernel)(FindArgs) = c.src ? k_find_count<false> : k_find_count<true>;
    PROF_LAUNCH(PROF_FETCH, s, kernel, dim3((unsigned)((A.W + WPB - 1) / WPB)), dim3(SCCG_BLOCK), 0, s, A);
    SCCG_HIP(hipGetLastError());
    return sg_scan(A.wcnt, A.woff, A.W, s);
}

int fd_write(const FdCall& c, int64_t cap, int64_t* d_off, sccg_hit* d_hit, hipStream_t s) {
    if (c.nreg <= 0 || c.m < 1 || c.m > FD_MAXM || c.F < 0 || cap < 0) return SCCG_E_INVALID;
    FindArgs A = fd_args(c);
    A.off = d_off;
    A.hit = d_hit;
    A.cap = cap;
    void (*const kernel)(FindArgs) = c.src ? k_find_write<false> : k_find_write<true>;
    PROF_LAUNCH(PROF_FETCH, s, kernel, dim3((unsigned)((A.W + WPB - 1) / WPB)), dim3(SCCG_BLOCK), 0, s, A);
    SCCG_HIP(hipGetLastError());
    return 0;
}

namespace {
// scratch: Find's 34 W + 1 words, then the W * 64 pairs of distance words on a 16-byte boundary
FindMmArgs fa_args(const FdCall& c) {
    FindMmArgs M{};
    M.B = fd_args(c);
    M.K = (uint32_t)c.K;
    M.dist = reinterpret_cast<uint64_t*>(((uintptr_t)(M.B.woff + M.B.W + 1) + 15) & ~(uintptr_t)15);
    return M;
}
}  // namespace

int64_t fa_scratch_words(int64_t F) { return fd_scratch_words(F) + 128 * fd_tiles(F) + 1; }

int fa_count(const FdCall& c, hipStream_t s) {
    if (c.nreg <= 0 || c.m < 1 || c.m > FD_MAXM || c.F < 0 || c.K < 0 || c.K > SCCG_FIND_MAX_MISMATCHES) return SCCG_E_INVALID;
    const FindMmArgs M = fa_args(c);
    void (*const kernel)(FindMmArgs) = c.src ? k_find_mm_count<false> : k_find_mm_count<true>;
    PROF_LAUNCH(PROF_FETCH, s, kernel, dim3((unsigned)((M.B.W + WPB - 1) / WPB)), dim3(SCCG_BLOCK), 0, s, M);
    SCCG_HIP(hipGetLastError());
    return sg_scan(M.B.wcnt, M.B.woff, M.B.W, s);
}

int fa_write(const FdCall& c, int64_t cap, int64_t* d_off, sccg_hit_mm* d_hit, hipStream_t s) {
    if (c.nreg <= 0 || c.m < 1 || c.m > FD_MAXM || c.F < 0 || cap < 0) return SCCG_E_INVALID;
    FindMmArgs M = fa_args(c);
    M.B.off = d_off;
    M.B.cap = cap;
    M.hit = d_hit;
    void (*const kernel)(FindMmArgs) = c.src ? k_find_mm_write<false> : k_find_mm_write<true>;
    PROF_LAUNCH(PROF_FETCH, s, kernel, dim3((unsigned)((M.B.W + WPB - 1) / WPB)), dim3(SCCG_BLOCK), 0, s, M);
    SCCG_HIP(hipGetLastError());
    return 0;
}
