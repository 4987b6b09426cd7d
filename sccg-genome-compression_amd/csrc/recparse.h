// recparse.h -- the staged-bytes view and the integer grammar every parser of the record text shares
// (decomp.hip: run lines, record line, fetch; locate.hip: the token list of the locate index;
// segments.hip: the segment starts of the record blocks under a region).
#pragma once

#include "common.h"

constexpr int RL_BEHIND = 32, RL_AHEAD = 64;

// the wave's staged bytes: global positions [t0 - RL_BEHIND, t0 + tile + RL_AHEAD), 0 outside [0, n)
struct RlView {
    const uint8_t* b;
    int64_t t0, n, tile;
    __device__ __forceinline__ uint8_t at(int64_t i) const { return b[i - t0 + RL_BEHIND]; }
    __device__ __forceinline__ int64_t lim() const { return t0 + tile + RL_AHEAD; }
};

// stoi on [a, e) of the view: an optional sign, then 1 to 10 digits within int32, all of it consumed
__device__ __forceinline__ bool parse_int_v(const RlView& v, int64_t a, int64_t e, int64_t* out) {
    if (a >= e) return false;
    bool neg = false;
    if (v.at(a) == '-' || v.at(a) == '+') { neg = v.at(a) == '-'; a++; }
    if (a >= e || e - a > 10) return false;
    int64_t x = 0;
    for (int64_t i = a; i < e; i++) {
        const uint8_t c = v.at(i);
        if (c < '0' || c > '9') return false;
        x = x * 10 + (c - '0');
    }
    x = neg ? -x : x;
    if (x > INT32_MAX || x < INT32_MIN) return false;
    *out = x;
    return true;
}
