// rsx_rank_math.hpp — the arithmetic of rsx_segmented_rank that needs no HIP type, pure: how the three per-tile carries of a sorted segment
// combine across its tiles, and how (run start, run end, distinct keys before, sorted position, method) become a rank and a tie count.
// Plain g++ compiles it too (host/harness/rank_selftest.cpp runs it on case files); under hipcc every function is __host__ __device__.
// Included by rsx_rank.hpp: the kernels' scans (over the lanes, the waves, the threads' tile ranges) use these functions as their operators.
//
//   A sorted segment of L keys lies on T tiles.  A HEAD is a sorted position whose key differs from its predecessor's, or position 0.
//   Positions are relative to the segment.  Per tile an Edge: the number of heads, the first and the last head in it (kNone: the tile
//   holds no head: a run of equal keys passes through it).  Per tile a Carry, what the tile must know of the others:
//     start  the last head before the tile: where the run that enters it began (kNone for the first tile, whose position 0 is a head)
//     next   the first head at or after the tile's end, L if there is none: where the run that leaves it ends
//     dense  the heads before the tile
//   start is a forward scan with "the later head wins", next the same scan backward, dense a sum: each associative, so the kernels may
//   fold them in any grouping; join() is the sequential form.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RSX_RANK_HD __host__ __device__ __forceinline__
#else
#define RSX_RANK_HD inline
#endif

namespace rsx_rank {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kOrdinal = 0, kMin = 1, kMax = 2, kDense = 3, kAverage = 4;      // RSX_RANK_* of include/radixsort_hip.h
constexpr uint32_t kMethods = 5;

struct Edge {
    uint32_t heads, first, last;
};

struct Carry {
    uint32_t start, next, dense;
};

// forward: the last head seen so far, after a piece whose last head is `last`
RSX_RANK_HD uint32_t carry_start(uint32_t start_in, uint32_t last)
{
    return last != kNone ? last : start_in;
}

// backward: the first head from here on, before a piece whose first head is `first`
RSX_RANK_HD uint32_t carry_next(uint32_t next_after, uint32_t first)
{
    return first != kNone ? first : next_after;
}

RSX_RANK_HD uint32_t carry_dense(uint32_t dense_in, uint32_t heads)
{
    return dense_in + heads;
}

// The three scans over the T tiles of a segment of L keys, sequential form: out[t] is what tile t needs.
template <typename EdgeOf>
RSX_RANK_HD void join(EdgeOf edge_of, uint32_t T, uint32_t L, Carry* out)
{
    uint32_t start = kNone, dense = 0;
    for (uint32_t t = 0; t < T; ++t) {
        const Edge e = edge_of(t);
        out[t].start = start;
        out[t].dense = dense;
        start = carry_start(start, e.last);
        dense = carry_dense(dense, e.heads);
    }
    uint32_t next = kNone;
    for (uint32_t t = T; t-- > 0;) {
        out[t].next = next != kNone ? next : L;
        next = carry_next(next, edge_of(t).first);
    }
}

// The run of the key at sorted position q: [start, end), `dense` distinct keys strictly before it.
//   ordinal  q                      min  start                     max  end - 1
//   dense    dense                  average  start + end - 1 = min + max: TWICE the average rank, an exact integer (L <= 2^31)
RSX_RANK_HD uint32_t rank_of(uint32_t method, uint32_t start, uint32_t end, uint32_t dense, uint32_t q)
{
    switch (method) {
    case kOrdinal: return q;
    case kMin: return start;
    case kMax: return end - 1u;
    case kDense: return dense;
    default: return start + (end - 1u);
    }
}

RSX_RANK_HD uint32_t ties_of(uint32_t start, uint32_t end)
{
    return end - start;
}

}  // namespace rsx_rank
