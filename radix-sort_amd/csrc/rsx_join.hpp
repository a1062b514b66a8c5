// rsx_join.hpp — kernels of rsx_segmented_join: the equi-join of sorted segment s of A with sorted segment s of B, four kinds.  For A element
// j with lower bound lb and upper bound ub of its key in B_s, c = ub - lb partners: INNER emits the rows (j, lb + r), r < c; LEFT the same
// and (j, none) where c == 0; SEMI (j, lb) iff c > 0; ANTI (j, -) iff c == 0.  Rows are ordered by segment, A position, B position and
// packed from 0.  Included by rsx_capi.hip (host side: capi_join.inc).
//
//   (unique_reset_kernel + unique_validate_kernel, unchanged, once per offsets array: the first bad segment of either, one word)
//   join_count_kernel    tiles of 4096 A positions of the ABSOLUTE grid over [0, na) (tile t = positions [4096 t, 4096 t + 4096), so that
//                        the 16-byte loads of a whole tile are aligned whatever aoff[0] is); 256 threads, thread q the 16 consecutive
//                        positions 16 q ..; positions outside [aoff[0], aoff[S]) and behind na count 0 rows.  Per element the segment
//                        (search_kernel's rule: the tile's first and last segment by bisection, in between only where they differ), lb by
//                        rsx_search.hpp's lockstep bisection in global memory (its DIRECT path), and ub inside [lb, Lb): a gallop from lb
//                        (probes lb, lb + 1, lb + 3, lb + 7, ...: one probe where there is no partner, two where there is one) and the
//                        same bisection over the window it leaves.  Every index formed lies in [0, Lb), so unsorted input stays inside
//                        its buffers and gives c >= 0 and lb + c <= Lb.  The effective count (rsx_join_math.hpp) goes through a 64-bit
//                        exclusive scan of the workgroup: thread-serial over the 16, block_scan_u64 over the 256.  Stores, each 16 per
//                        thread as 16-byte vectors, padding of the last tile included: first[j] (uint32: lb, or none for LEFT's lone
//                        row), pre[j] (uint64, exclusive in-tile prefix), arel[j] (uint32: j - aoff[s(j)], only with offsets and an A
//                        index output), and tbase[t] = the tile's total.
//   join_scan_kernel     tbase[0 .. ntiles] := its exclusive 64-bit prefix, tbase[ntiles] = P: ONE workgroup of 1024 threads walks the
//                        table 1024 entries a trip with a running carry (at most 2^19 + 1 entries; launch_table_scan is 32-bit).
//   join_offsets_kernel  one thread per s <= S: d_out_offsets[s] = R(aoff[s]), R(j) = tbase[j >> 12] + pre[j]; zeros and the report with a
//                        bad segment.
//   join_split_kernel    one thread per boundary u of the grid of 4096 output rows: split[u] = #{ j : R(j) < 4096 u } (rsx_join_math.hpp).
//   join_write_kernel    per output tile, expand_tile_kernel's scheme with A positions in the role of segments and R in the role of the
//                        offsets.  No start inside the tile: one owner, a pure fill (a constant, b = first + rank).  Else the A positions
//                        [split[u], split[u+1]) mark slot R(j) - 4096 u of a 4096-slot LDS array with j + 1 by an LDS max, A tile by A
//                        tile, 1024 per trip; an A tile whose total is 0 is skipped on its two table entries alone (all its elements share
//                        one offset with the next element that has a row, which wins the max anyway).  A long run of such tiles is walked
//                        one table entry after another: slow but correct.  Then the inclusive max-scan and the ranks behind the marks, and
//                        the three outputs leave through expand_emit: a = arel[owner] (or the owner itself with one segment),
//                        b = first[owner] + rank, key = d_a[owner].
//
// Grids come from na, S and min(out_capacity, the row bound of na and nb) alone; nothing is read back; the only atomics are the LDS max of
// the marks (commutative: the result does not depend on the order of arrival) and the checks' atomicMin on the first-bad-segment word.
#pragma once

#include "rsx_join_math.hpp"
#include "rsx_expand.hpp"
#include "rsx_search.hpp"
#include "rsx_segmented.hpp"

namespace rsx {

constexpr int kJoinThreads = 256, kJoinPerThread = 16;
constexpr int kJoinScanThreads = 1024;
static_assert(kJoinThreads * kJoinPerThread == static_cast<int>(rsx_join::kTileSlots), "one tile is 4096 A positions");
static_assert(kJoinPerThread % kSearchQpt == 0, "the lockstep bisection takes kSearchQpt elements at a time");

// The window of the upper bound behind lb, kSearchQpt in lockstep.  In: base = lb, len = Lb - lb (0: nothing to do).  Out: keys
// [lb, base) are not after q, key base + len (if inside) is; search_bisect(right) over (base, len) finishes.  Probes base + step - 1 <
// base + len only.
template <typename Key, typename At>
__device__ __forceinline__ void join_gallop(At&& at, const Key (&q)[kSearchQpt], uint32_t (&base)[kSearchQpt], uint32_t (&len)[kSearchQpt])
{
    uint32_t step[kSearchQpt], end[kSearchQpt];
    bool open[kSearchQpt];
    bool any = false;
#pragma unroll
    for (int r = 0; r < kSearchQpt; ++r) {
        step[r] = 1;
        end[r] = base[r] + len[r];
        open[r] = len[r] != 0;
        any |= open[r];
    }
    while (any) {
        Key k[kSearchQpt];
#pragma unroll
        for (int r = 0; r < kSearchQpt; ++r) {
            k[r] = open[r] ? at(r, base[r] + step[r] - 1u) : Key{0};
        }
        any = false;
#pragma unroll
        for (int r = 0; r < kSearchQpt; ++r) {
            if (open[r]) {
                const uint32_t pos = base[r] + step[r] - 1u;
                if (k[r] <= q[r]) {
                    base[r] = pos + 1u;
                    step[r] = min(step[r] << 1, end[r] - base[r]);      // (0 at the end)
                    len[r] = end[r] - base[r];
                    open[r] = base[r] < end[r];
                } else {
                    len[r] = pos - base[r];
                    open[r] = false;
                }
            }
            any |= open[r];
        }
    }
}

template <typename T>
__device__ __forceinline__ void join_store16(T* __restrict__ dst, const T (&v)[kJoinPerThread])
{
    constexpr int PER = 16 / sizeof(T);
#pragma unroll
    for (int g = 0; g < kJoinPerThread / PER; ++g) {
        ExpandVec<T> w;
#pragma unroll
        for (int c = 0; c < PER; ++c) {
            w.x[c] = v[g * PER + c];
        }
        *reinterpret_cast<ExpandVec<T>*>(dst + g * PER) = w;
    }
}

// Workgroup b takes the A tiles [b * chunk, (b + 1) * chunk).  first / arel may be null (not needed by the outputs asked for).
template <typename Key>
__global__ __launch_bounds__(kJoinThreads) void join_count_kernel(const Key* __restrict__ ka, uint64_t na, const uint64_t* __restrict__ aoff,
                                                                  const Key* __restrict__ kb, uint64_t nb, const uint64_t* __restrict__ boff,
                                                                  uint64_t nseg, const uint32_t* __restrict__ bad, uint32_t ntiles, uint32_t chunk,
                                                                  uint32_t op, Key ca, Key cm, uint32_t* __restrict__ first,
                                                                  uint64_t* __restrict__ pre, uint32_t* __restrict__ arel, uint64_t* __restrict__ tbase)
{
    __shared__ uint64_t wtot[kJoinThreads / kWave];
    constexpr int VEC = KeyVec<Key>::N;
    const uint32_t tid = threadIdx.x;
    if (*bad != kUniqNoBad) return;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    const uint64_t alo = aoff ? aoff[0] : 0ull, ahi = aoff ? aoff[nseg] : na;
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint64_t tile_start = static_cast<uint64_t>(t) << rsx_join::kTileShift;
        const uint64_t a = max(tile_start, alo), e = min(tile_start + rsx_join::kTileSlots, ahi);
        const uint64_t j0 = tile_start + static_cast<uint64_t>(tid) * kJoinPerThread;
        uint64_t cnt[kJoinPerThread];
        uint32_t fst[kJoinPerThread], rel[kJoinPerThread];
#pragma unroll
        for (int i = 0; i < kJoinPerThread; ++i) {
            cnt[i] = 0;
            fst[i] = 0;
            rel[i] = 0;
        }
        if (a < e) {                                                          // (uniform) a live element in the tile
            uint64_t s_first = 0, s_last = 0;
            if (aoff) {
                s_first = search_segment_of(aoff, 0, nseg - 1, a);
                s_last = search_segment_of(aoff, s_first, nseg - 1, e - 1);
            }
            Key k[kJoinPerThread];
            if (tile_start + rsx_join::kTileSlots <= na) {
#pragma unroll
                for (int g = 0; g < kJoinPerThread / VEC; ++g) {
                    const KeyVec<Key> v = load_keys16(ka + j0 + g * VEC);
#pragma unroll
                    for (int c = 0; c < VEC; ++c) {
                        k[g * VEC + c] = v.k[c];
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < kJoinPerThread; ++i) {
                    k[i] = j0 + i < na ? ka[j0 + i] : Key{0};
                }
            }
#pragma unroll
            for (int g = 0; g < kJoinPerThread / kSearchQpt; ++g) {
                Key q[kSearchQpt];
                const Key* seg[kSearchQpt];
                uint32_t base[kSearchQpt], len[kSearchQpt], lb[kSearchQpt], L[kSearchQpt];
                bool live[kSearchQpt];
#pragma unroll
                for (int r = 0; r < kSearchQpt; ++r) {
                    const int i = g * kSearchQpt + r;
                    const uint64_t j = j0 + i;
                    live[r] = j >= a && j < e;
                    q[r] = codec_encode(k[i], ca, cm);
                    uint64_t s = s_first;
                    if (live[r] && s_first != s_last) {
                        s = search_segment_of(aoff, s_first, s_last, j);
                    }
                    const uint64_t h0 = live[r] ? uniq_off(boff, s, nb) : 0ull;
                    seg[r] = kb + h0;
                    L[r] = live[r] ? static_cast<uint32_t>(uniq_off(boff, s + 1, nb) - h0) : 0u;
                    rel[i] = live[r] ? static_cast<uint32_t>(j - uniq_off(aoff, s, na)) : 0u;
                    base[r] = 0;
                    len[r] = L[r];
                }
                auto at = [&](int r, uint32_t x) { return codec_encode(seg[r][x], ca, cm); };
                search_bisect(at, q, false, base, len);
#pragma unroll
                for (int r = 0; r < kSearchQpt; ++r) {
                    lb[r] = base[r];
                    len[r] = L[r] - base[r];
                }
                join_gallop(at, q, base, len);
                search_bisect(at, q, true, base, len);
#pragma unroll
                for (int r = 0; r < kSearchQpt; ++r) {
                    const int i = g * kSearchQpt + r;
                    const uint64_t c = base[r] - lb[r];
                    cnt[i] = live[r] ? rsx_join::effective_count(c, op) : 0ull;
                    fst[i] = rsx_join::first_partner(lb[r], c, op);
                }
            }
        }
        // the exclusive 64-bit prefix inside the tile
        uint64_t mine[1] = {0}, all[1];
#pragma unroll
        for (int i = 0; i < kJoinPerThread; ++i) {
            const uint64_t c = cnt[i];
            cnt[i] = mine[0];
            mine[0] += c;
        }
        block_scan_u64<kJoinThreads, 1>(mine, all, wtot);
#pragma unroll
        for (int i = 0; i < kJoinPerThread; ++i) {
            cnt[i] += mine[0];
        }
        join_store16(pre + j0, cnt);
        if (first) join_store16(first + j0, fst);
        if (arel) join_store16(arel + j0, rel);
        if (tid == 0) {
            tbase[t] = all[0];
        }
    }
}

// tbase[0 .. n] := exclusive prefix of tbase[0 .. n), tbase[n] = the total.  One workgroup.
__global__ __launch_bounds__(kJoinScanThreads) void join_scan_kernel(uint64_t* __restrict__ tbase, uint32_t n, const uint32_t* __restrict__ bad)
{
    __shared__ uint64_t wtot[kJoinScanThreads / kWave];
    if (*bad != kUniqNoBad) return;
    uint64_t carry = 0;
#pragma unroll 1
    for (uint32_t i0 = 0; i0 < n; i0 += kJoinScanThreads) {
        const uint32_t i = i0 + threadIdx.x;
        uint64_t v[1] = {i < n ? tbase[i] : 0ull}, all[1];
        block_scan_u64<kJoinScanThreads, 1>(v, all, wtot);
        if (i < n) {
            tbase[i] = carry + v[0];
        }
        carry += all[0];
    }
    if (threadIdx.x == 0) {
        tbase[n] = carry;
    }
}

// d_out_offsets; with bad input zeros, and the first bad segment + 1 goes to the mapped host words with the call's id unless an earlier
// report is still pending there (as expand_split_kernel does)
__global__ __launch_bounds__(kExpandSmallThreads) void join_offsets_kernel(const uint64_t* __restrict__ aoff, uint64_t na, uint64_t nseg,
                                                                          const uint32_t* __restrict__ bad, const uint64_t* __restrict__ tbase,
                                                                          const uint64_t* __restrict__ pre, uint32_t ntiles, uint64_t* __restrict__ out,
                                                                          uint32_t* status_host, uint32_t call_id)
{
    const uint32_t b = *bad;
    if (b != kUniqNoBad && blockIdx.x == 0 && threadIdx.x == 0 && __hip_atomic_load(status_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
        __hip_atomic_store(status_host + 1, call_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(status_host, b + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);            // (after the call's id)
    }
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kExpandSmallThreads;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kExpandSmallThreads + threadIdx.x; s <= nseg; s += stride) {
        out[s] = b != kUniqNoBad ? 0ull : rsx_join::row_offset(tbase, pre, ntiles, uniq_off(aoff, s, na));
    }
}

__global__ __launch_bounds__(kExpandSmallThreads) void join_split_kernel(const uint64_t* __restrict__ tbase, const uint64_t* __restrict__ pre, uint32_t ntiles,
                                                                        const uint32_t* __restrict__ bad, uint32_t nout, uint32_t* __restrict__ split)
{
    if (*bad != kUniqNoBad) return;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kExpandSmallThreads;
    for (uint64_t u = static_cast<uint64_t>(blockIdx.x) * kExpandSmallThreads + threadIdx.x; u <= nout; u += stride) {
        split[u] = static_cast<uint32_t>(rsx_join::split(tbase, pre, ntiles, u << rsx_join::kTileShift));      // <= 2^31 + 4095
    }
}

// Workgroup b takes the output tiles [b * chunk, (b + 1) * chunk).  Which outputs exist is an argument (null pointers, uniform).
template <typename Key>
__global__ __launch_bounds__(kJoinThreads) void join_write_kernel(const Key* __restrict__ ka, const uint32_t* __restrict__ bad,
                                                                  const uint64_t* __restrict__ tbase, const uint64_t* __restrict__ pre,
                                                                  const uint32_t* __restrict__ first, const uint32_t* __restrict__ arel, uint32_t ntiles,
                                                                  const uint32_t* __restrict__ split, uint32_t nout, uint32_t chunk, uint64_t capacity,
                                                                  Key* __restrict__ kout, uint32_t* __restrict__ aout, uint32_t* __restrict__ bout)
{
    __shared__ ExpandShared sh;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t u0 = blockIdx.x * chunk, u1 = min(u0 + chunk, nout);
    if (*bad != kUniqNoBad || u0 >= u1) return;
    const uint64_t total = tbase[ntiles];
    const uint32_t npos = ntiles << rsx_join::kTileShift;                       // A positions, padding included (<= 2^31 + 4095)
    const bool need_rank = bout != nullptr;                                     // (uniform)
#pragma unroll 1
    for (uint32_t u = u0; u < u1; ++u) {
        const rsx_expand::Range r = rsx_join::tile_rows(u, total, capacity);
        if (r.a >= r.b) return;                                                 // (uniform) at or past P or the capacity: so are all later tiles
        const uint64_t tile_start = static_cast<uint64_t>(u) << rsx_join::kTileShift;
        const uint32_t s_lo = split[u], s_hi = split[u + 1];                    // (uniform) the A positions whose rows start inside the tile
        if (s_lo == s_hi) {
            // ---- fill path: all of [a, b) are rows of A position s_lo - 1 (r.a < r.b <= P implies s_lo >= 1)
            const uint32_t j = s_lo - 1u;
            const uint64_t base = rsx_join::row_offset(tbase, pre, ntiles, j);
            if (aout) {
                const uint32_t v = arel ? arel[j] : j;
                expand_emit(aout, r.a, r.b, [v](uint64_t) { return v; });
            }
            if (bout) {
                const uint32_t f = first[j];
                expand_emit(bout, r.a, r.b, [f, base](uint64_t p) { return f + static_cast<uint32_t>(p - base); });
            }
            if (kout) {
                const Key v = ka[j];
                expand_emit(kout, r.a, r.b, [v](uint64_t) { return v; });
            }
            continue;
        }
        // ---- general path
        // 1. clear the marks
        {
            uint4* z = reinterpret_cast<uint4*>(sh.own + tid * kJoinPerThread);
#pragma unroll
            for (int i = 0; i < kJoinPerThread / 4; ++i) {
                z[i] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        __syncthreads();
        // 2. the walk, A tile by A tile: every A position of [s_lo, s_hi) marks the slot of its first row with its id + 1; of equal
        //    offsets the largest id stays, which is the one that has a row there
#pragma unroll 1
        for (uint32_t t = s_lo >> rsx_join::kTileShift; t <= (s_hi - 1u) >> rsx_join::kTileShift; ++t) {
            const uint64_t tb = tbase[t];
            if (tbase[t + 1] == tb) continue;                                   // (uniform) no row in this A tile
            const uint32_t lo = max(s_lo, t << rsx_join::kTileShift), hi = min(s_hi, (t + 1u) << rsx_join::kTileShift);
            const uint64_t* __restrict__ p = pre;
#pragma unroll 1
            for (uint32_t j = lo + tid; j < hi; j += 4 * kJoinThreads) {
                uint64_t x[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    x[k] = tb + p[min(j + k * kJoinThreads, hi - 1u)] - tile_start;
                }
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t jk = j + k * kJoinThreads;
                    if (jk < hi && x[k] < rsx_join::kTileSlots) {               // (the second: always)
                        atomicMax(&sh.own[x[k]], jk + 1u);
                    }
                }
            }
        }
        __syncthreads();
        // 3. the inclusive max-scan over the slots; what the tile inherits is s_lo
        uint32_t m[kJoinPerThread];
        {
            const uint4* q = reinterpret_cast<const uint4*>(sh.own + tid * kJoinPerThread);
#pragma unroll
            for (int i = 0; i < kJoinPerThread / 4; ++i) {
                const uint4 w = q[i];
                m[4 * i] = w.x;
                m[4 * i + 1] = w.y;
                m[4 * i + 2] = w.z;
                m[4 * i + 3] = w.w;
            }
        }
        uint32_t mine = 0;
#pragma unroll
        for (int i = 0; i < kJoinPerThread; ++i) {
            mine = max(mine, m[i]);
        }
        const uint32_t incl = wave_inclusive_max(mine);
        if (lane == kWave - 1) {
            sh.wtot[wave] = incl;
        }
        __syncthreads();
        uint32_t run = s_lo;
#pragma unroll
        for (uint32_t w = 0; w < kJoinThreads / kWave; ++w) {
            run = max(run, w < wave ? sh.wtot[w] : 0u);
        }
        const uint32_t left = __shfl_up(incl, 1);
        if (lane != 0) {
            run = max(run, left);
        }
        // run = owner + 1 of the slot before the thread's first.  Its rank comes from R, every later one from the marks.
        uint32_t rk = 0;
        if (need_rank && run >= 1u && run <= npos) {
            rk = static_cast<uint32_t>(tile_start + static_cast<uint64_t>(tid) * kJoinPerThread - rsx_join::row_offset(tbase, pre, ntiles, run - 1u)) - 1u;
        }
        uint32_t rnk[kJoinPerThread];
#pragma unroll
        for (int i = 0; i < kJoinPerThread; ++i) {
            rk = m[i] != 0u ? 0u : rk + 1u;
            run = max(run, m[i]);
            m[i] = run;
            rnk[i] = rk;
        }
        {
            uint4* q = reinterpret_cast<uint4*>(sh.own + tid * kJoinPerThread);
#pragma unroll
            for (int i = 0; i < kJoinPerThread / 4; ++i) {
                q[i] = make_uint4(m[4 * i], m[4 * i + 1], m[4 * i + 2], m[4 * i + 3]);
            }
            if (need_rank) {
                uint4* p = reinterpret_cast<uint4*>(sh.rank + tid * kJoinPerThread);
#pragma unroll
                for (int i = 0; i < kJoinPerThread / 4; ++i) {
                    p[i] = make_uint4(rnk[4 * i], rnk[4 * i + 1], rnk[4 * i + 2], rnk[4 * i + 3]);
                }
            }
        }
        __syncthreads();
        // 4. the outputs, each by its own alignment.  Every row of [a, b) has an owner in [0, na).
        const uint32_t* own = sh.own;
        const uint32_t* rank = sh.rank;
        if (aout) {
            if (arel) {
                expand_emit(aout, r.a, r.b, [=](uint64_t p) { return arel[own[p - tile_start] - 1u]; });
            } else {
                expand_emit(aout, r.a, r.b, [=](uint64_t p) { return own[p - tile_start] - 1u; });
            }
        }
        if (bout) {
            expand_emit(bout, r.a, r.b, [=](uint64_t p) { return first[own[p - tile_start] - 1u] + rank[p - tile_start]; });
        }
        if (kout) {
            expand_emit(kout, r.a, r.b, [=](uint64_t p) { return ka[own[p - tile_start] - 1u]; });
        }
        __syncthreads();                                                        // (the next tile clears the slots)
    }
}

}  // namespace rsx
