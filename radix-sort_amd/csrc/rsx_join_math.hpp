// rsx_join_math.hpp — the rules of rsx_segmented_join that are no kernel, pure: how many rows an A element emits for its number of partners
// and the kind of join, the two-level row offset R(j) = tbase[j >> 12] + pre[j], its split at a boundary of the 4096-row output grid (the
// expand's tile_split on that two-level function: rsx_expand_math.hpp's bisection over the tile bases, then one over the prefixes of one
// A tile), and the rows of an output tile.  No HIP type in here, so that plain g++ compiles it too (host/harness/join_selftest.cpp runs it
// on a case file); under hipcc every function is __host__ __device__.  Included by rsx_join.hpp.
#pragma once

#include "rsx_expand_math.hpp"

namespace rsx_join {

constexpr uint32_t kInner = 0, kLeft = 1, kSemi = 2, kAnti = 3;      // RSX_JOIN_*
constexpr uint32_t kNone = 0xFFFFFFFFu;                              // the B index of a LEFT row without a partner
constexpr int kTileShift = rsx_expand::kTileShift;                   // A elements per count tile = output rows per write tile = 4096
constexpr uint32_t kTileSlots = rsx_expand::kTileSlots;

// rows that an A element with c partners emits
RSX_EXPAND_HD uint64_t effective_count(uint64_t c, uint32_t op)
{
    return op == kInner ? c : op == kLeft ? (c ? c : 1u) : op == kSemi ? (c ? 1u : 0u) : (c ? 0u : 1u);
}

// what the count pass stores as the first B position of an A element's rows: lb, or kNone for the LEFT row that has no partner (its one
// row has rank 0, so lb + rank is the B index of every row of every kind)
RSX_EXPAND_HD uint32_t first_partner(uint32_t lb, uint64_t c, uint32_t op)
{
    return op == kLeft && c == 0 ? kNone : lb;
}

// R(j): rows before A position j.  tbase has ntiles + 1 entries (the last is P), pre ntiles * 4096 (the padding behind na included).
RSX_EXPAND_HD uint64_t row_offset(const uint64_t* tbase, const uint64_t* pre, uint64_t ntiles, uint64_t j)
{
    return (j >> kTileShift) >= ntiles ? tbase[ntiles] : tbase[j >> kTileShift] + pre[j];
}

// #{ j in [0, ntiles * 4096) : R(j) < x }: the A positions whose rows start before row x.  R is non-decreasing (every count is >= 0).
// Of the tiles those before the last one T with tbase[T] < x lie below x whole (R(j) <= tbase[t + 1] <= tbase[T] for j in tile t < T),
// those behind it not at all; inside T the prefixes are bisected against x - tbase[T].
RSX_EXPAND_HD uint64_t split(const uint64_t* tbase, const uint64_t* pre, uint64_t ntiles, uint64_t x)
{
    const uint64_t k = rsx_expand::lower_bound(tbase, ntiles, x);         // tile bases below x, of ntiles + 1
    if (k == 0) return 0;
    if (k > ntiles) return ntiles << kTileShift;                           // x > P
    const uint64_t T = k - 1, rel = x - tbase[T];
    const uint64_t* p = pre + (T << kTileShift);
    uint64_t lo = 0, hi = kTileSlots;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (p[mid] < rel) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return (T << kTileShift) + lo;
}

// the rows of output tile u that are written: [a, b) = [4096 u, min(4096 (u + 1), P, capacity)), empty if a >= b
RSX_EXPAND_HD rsx_expand::Range tile_rows(uint64_t u, uint64_t total, uint64_t capacity)
{
    return rsx_expand::tile_range(u, 0, total < capacity ? total : capacity);
}

// workgroups' worth of output tiles that a call can need: rows are bounded by the inputs' sizes, whatever the capacity says
RSX_EXPAND_HD uint64_t row_bound(uint64_t na, uint64_t nb, uint32_t op)
{
    return op == kInner ? na * nb : op == kLeft ? na * (nb ? nb : 1u) : na;      // (na, nb <= 2^31: no overflow)
}

}  // namespace rsx_join
