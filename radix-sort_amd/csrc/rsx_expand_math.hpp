// rsx_expand_math.hpp — the owner rule and the tile-range arithmetic of rsx_segmented_expand, pure: bisections of the offsets on a plain
// array, the part of [off[0], off[S]) that a tile of the absolute 4096-position grid holds, and how that part splits into element stores
// and 16-byte stores for an output that is only element-aligned.  No HIP type in here, so that plain g++ compiles it too
// (host/harness/expand_selftest.cpp runs it on a case file); under hipcc every function is __host__ __device__.  Included by rsx_expand.hpp.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RSX_EXPAND_HD __host__ __device__ __forceinline__
#else
#define RSX_EXPAND_HD inline
#endif

namespace rsx_expand {

constexpr int kTileShift = 12;
constexpr uint32_t kTileSlots = 1u << kTileShift;        // output positions per tile

// first s in [0, nseg] with off[s] >= x, nseg + 1 if there is none (valid offsets are non-decreasing): the number of offsets below x
RSX_EXPAND_HD uint64_t lower_bound(const uint64_t* off, uint64_t nseg, uint64_t x)
{
    uint64_t lo = 0, hi = nseg + 1;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] < x) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// The owner rule, as an id + 1: the number of s in [0, nseg] with off[s] <= i.  0: i lies before off[0].  nseg + 1: i lies at or behind
// off[S].  Else the owner of i is the result - 1, the LARGEST s with off[s] <= i: of several segments that share an offset the last one
// owns the position, so an empty segment owns nothing.
RSX_EXPAND_HD uint64_t owner_plus_one(const uint64_t* off, uint64_t nseg, uint64_t i)
{
    return i == ~0ull ? nseg + 1 : lower_bound(off, nseg, i + 1);
}

// What the split kernel stores for tile boundary t: the number of offsets below 4096 * t.  The starts that fall into tile t are the
// segments [split(t), split(t + 1)); the owner + 1 of the tile's first position, unless one of them starts there, is split(t).
RSX_EXPAND_HD uint64_t tile_split(const uint64_t* off, uint64_t nseg, uint64_t t)
{
    return lower_bound(off, nseg, t << kTileShift);
}

// The part of [lo, hi) = [off[0], off[S]) inside tile t: [a, b), empty if a >= b.
struct Range {
    uint64_t a, b;
};

RSX_EXPAND_HD Range tile_range(uint64_t t, uint64_t lo, uint64_t hi)
{
    const uint64_t ts = t << kTileShift, te = ts + kTileSlots;
    Range r;
    r.a = lo > ts ? lo : ts;
    r.b = hi < te ? hi : te;
    if (r.b < r.a) r.b = r.a;
    return r;
}

// How [a, b) of an output whose element 0 lies at byte address `addr` (a multiple of elem_bytes: 4 or 8) is stored: `head` elements one by
// one up to the first 16-byte boundary, `nvec` stores of 16 bytes, `tail` elements one by one.
struct Stores {
    uint64_t head, nvec, tail;
};

RSX_EXPAND_HD Stores tile_stores(uint64_t addr, uint32_t elem_bytes, uint64_t a, uint64_t b)
{
    const uint64_t per = 16u / elem_bytes;
    const uint64_t mis = (addr / elem_bytes + a) % per;          // elements behind a 16-byte boundary
    Stores s;
    s.head = (per - mis) % per;
    if (s.head > b - a) s.head = b - a;
    s.nvec = (b - a - s.head) / per;
    s.tail = b - a - s.head - s.nvec * per;
    return s;
}

}  // namespace rsx_expand
