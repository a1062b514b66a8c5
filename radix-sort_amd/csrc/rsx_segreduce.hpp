// rsx_segreduce.hpp — kernels of rsx_segmented_reduce: sum / min / max / argmin / argmax of the values of every segment, one result per
// segment id (dense, not packed).  Included by rsx_capi.hip (host side: capi_segreduce.inc).
//
//   (unique_reset_kernel + unique_validate_kernel, unchanged: the first bad segment of the offsets, one word)
//   segreduce_tile_kernel  per 4096-element tile of the global grid: the restarts (scan_tile_restarts without keys: the starts of the
//                          non-empty segments) and a stop at off[S], a restart-flagged fold over the tile (the scan's thread and tile
//                          levels, shared code).  A segment that begins AND ends inside the tile is stored at out[s] at once; the walk over
//                          the offsets leaves s in LDS, at the place of the segment's last element.  What is left goes to per-tile partials: lead[t] = the
//                          elements before the tile's first flag (the whole tile without one), tail[t] = the elements from its last
//                          restart on, open[t] = the segment that tail[t] belongs to if that segment goes on behind the tile, else none.
//   segreduce_join_kernel  (1) one thread per segment: an empty one gets the identity (index 0xFFFFFFFF).  (2) one workgroup per open
//                          tile t: segment s = open[t] ends in tile u = (off[s+1] - 1) / 4096, known from the offsets alone, so the
//                          loads of lead[t+1 .. u] are independent; out[s] = tail[t] o J(lead[t+1 .. u]).  Reports bad offsets.
//
// ORDER OF A FLOAT SUM.  a o b has the EARLIER elements on the left unless said otherwise.  Elements outside [off[0], off[S]) count as 0;
// a flag (the restart at off[0], the stop at off[S]) always stands between them and anything that is stored.  The first two levels are the
// scan's (rsx_scan_by_key.hpp), the same code:
//   thread  (16 elements, thread q of a tile holds 16q .. 16q+15)  a[0] = v[0], a[j] = flagged a[j-1] o v[j], left to right.
//   tile    (256 threads)  the threads' a[15] are joined by a flagged Hillis-Steele scan over the 64 lanes of a wave (distances 1, 2, 4, ...
//           32: x[l] = x[l-d] o x[l]), the four wave totals are folded left to right and go on the left of the lanes' x: that is T(q).
//   A segment [b, e) whose last element e - 1 is element j of thread q of its tile, E = the part of it inside that tile:
//           E = a[j]             if the thread has a restart at or before j (the segment began in this thread);
//           E = T(q)             if j = 15 (thread q has no restart then, or the first case applied);
//           E = T(q - 1) o a[j]  otherwise (q = 0: a[j] alone).
//           If b lies in the same tile the result is E.  This is bit for bit what rsx_segmented_scan stores at e - 1 for such a segment.
//   grid    otherwise the segment covers the tiles t < t+1 < ... < u, m = u - t of them after the first: tail[t] = T(255) of tile t,
//           lead[t+i] = T(255) of the tiles in between, lead[u] = E.  J: thread r of the join's 256 folds lead[t+1+r], lead[t+1+r+256], ...
//           left to right (a STRIDED order, not the earlier-on-the-left one); the threads' partials are joined by a tree per wave
//           (distances 1, 2, ... 32: y[l] = y[l] o y[l+d], absent partials skipped) and the four wave totals are folded left to right.
//           The result is tail[t] o J.  With m <= 64 only the first wave has partials and the others stay out: the same association.
// Every choice is a function of the element's position on the global tile grid and of where the segment boundaries are, i.e. of values,
// offsets and n alone: not of the grid size, the workgroup a tile lands in, the engine's capacity or the stream.  There is no atomic on
// the value path and no workgroup waits for another: the launches are ordered by the stream.
// Steps on the longest path of J: ceil(m / 256) loads-and-folds, 6 tree levels, 3 folds: 2^16 partials (one segment of 2^28 elements) take
// 265 dependent steps, where reduce_carry_kernel's one wave takes 1024 + 6.
//
// ARGMIN / ARGMAX carry (value, position) pairs through the same levels.  (a, p) o (b, q) = the better of the two, the one with the lower
// position if neither is better: a NaN is better than every number, two NaNs tie, -0.0 and +0.0 tie.  That is commutative, so the strided
// order of J gives the FIRST extreme as well.  The position is the element's index in d_values (n <= 2^31 fits a word); what is stored is
// position - off[s].
//
// The op is a kernel argument (wave-uniform), as in the siblings; ARG is a template parameter: it adds an index register per element and a
// second output.  Instantiations: 4 value kinds x {plain, arg} for each of the two kernels.  No scratch memory.
#pragma once

#include "rsx_scan_by_key.hpp"

namespace rsx {

constexpr uint32_t kSegRedArgMin = 3u, kSegRedArgMax = 4u;        // RSX_REDUCE_ARGMIN / _ARGMAX (the kernels get kRedMin / kRedMax and ARG)
constexpr uint32_t kSegRedNone = 0xFFFFFFFFu;                     // open[t]: no segment goes on behind tile t; the index of an empty segment
constexpr int kSegRedJoinThreads = 256;

// What the levels carry: the value itself, or with ARG the value and its position.
template <typename Val>
struct SegPair {
    Val v;
    typename std::make_unsigned<typename std::conditional<sizeof(Val) == 8, int64_t, int32_t>::type>::type i;      // (as wide as v: no padding)
};
template <typename Val, bool ARG>
using SegItem = typename std::conditional<ARG, SegPair<Val>, Val>::type;

template <typename Val>
__device__ __forceinline__ SegPair<Val> red_shfl_up(SegPair<Val> x, int d)
{
    return SegPair<Val>{red_shfl_up(x.v, d), red_shfl_up(x.i, d)};
}

template <typename Val>
__device__ __forceinline__ SegPair<Val> red_shfl_down(SegPair<Val> x, int d)
{
    return SegPair<Val>{red_shfl_down(x.v, d), red_shfl_down(x.i, d)};
}

template <typename Val>
__device__ __forceinline__ Val seg_apply(uint32_t op, Val a, Val b)
{
    return red_apply(op, a, b);
}

// op is kRedMin or kRedMax
template <typename Val>
__device__ __forceinline__ SegPair<Val> seg_apply(uint32_t op, SegPair<Val> a, SegPair<Val> b)
{
    bool better, tie;
    if constexpr (std::is_integral<Val>::value) {
        better = op == kRedMin ? b.v < a.v : b.v > a.v;
        tie = a.v == b.v;
    } else {
        const bool an = a.v != a.v, bn = b.v != b.v;
        better = bn ? !an : (!an && (op == kRedMin ? b.v < a.v : b.v > a.v));
        tie = an == bn && (an || a.v == b.v);
    }
    return seg_select(better || (tie && b.i < a.i), b, a);
}

// c ? a : b, member by member: a select between two 16-byte pairs would go through memory
template <typename Val>
__device__ __forceinline__ Val seg_select(bool c, Val a, Val b)
{
    return c ? a : b;
}

template <typename Val>
__device__ __forceinline__ SegPair<Val> seg_select(bool c, SegPair<Val> a, SegPair<Val> b)
{
    return SegPair<Val>{c ? a.v : b.v, c ? a.i : b.i};
}

template <typename Val, bool ARG>
__device__ __forceinline__ SegItem<Val, ARG> seg_item(Val v, uint32_t pos)
{
    if constexpr (ARG) {
        return SegPair<Val>{v, pos};
    } else {
        return v;
    }
}

// The per-tile partials lie in one scratch buffer of 8-byte slots (capi_segreduce.inc); the positions exist with ARG only.
template <typename Val, bool ARG>
__device__ __forceinline__ void seg_put(Val* __restrict__ pv, uint32_t* __restrict__ pp, uint32_t t, SegItem<Val, ARG> x)
{
    if constexpr (ARG) {
        pv[t] = x.v;
        pp[t] = static_cast<uint32_t>(x.i);
    } else {
        pv[t] = x;
    }
}

template <typename Val, bool ARG>
__device__ __forceinline__ SegItem<Val, ARG> seg_get(const Val* __restrict__ pv, const uint32_t* __restrict__ pp, uint32_t t)
{
    if constexpr (ARG) {
        return SegPair<Val>{pv[t], pp[t]};
    } else {
        return pv[t];
    }
}

// the result of segment s: the value (optional with ARG) and the position relative to the segment's start
template <typename Val, bool ARG>
__device__ __forceinline__ void seg_store(const uint64_t* __restrict__ off, uint64_t n, uint64_t s, SegItem<Val, ARG> x, Val* __restrict__ vout,
                                          uint32_t* __restrict__ iout)
{
    if constexpr (ARG) {
        iout[s] = static_cast<uint32_t>(x.i) - static_cast<uint32_t>(uniq_off(off, s, n));
        if (vout) {
            vout[s] = x.v;
        }
    } else {
        vout[s] = x;
    }
}

// Workgroup b takes the tiles [b * chunk, (b + 1) * chunk); tiles outside [off[0], off[S]) are neither read nor given partials.
template <typename Val, bool ARG>
__global__ __launch_bounds__(kUniqThreads) void segreduce_tile_kernel(const Val* __restrict__ values, uint64_t n, const uint64_t* __restrict__ off,
                                                                      uint64_t nseg, const uint32_t* __restrict__ bad, uint32_t ntiles, uint32_t chunk,
                                                                      uint32_t op, Val* __restrict__ vout, uint32_t* __restrict__ iout,
                                                                      Val* __restrict__ lead, Val* __restrict__ tail, uint32_t* __restrict__ lead_pos,
                                                                      uint32_t* __restrict__ tail_pos, uint32_t* __restrict__ open_seg)
{
    using Item = SegItem<Val, ARG>;
    __shared__ UniqShared sh;
    __shared__ ScanShared<Item> ss;
    __shared__ ScanSegIds ids;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    uint64_t s0 = off ? uniq_lower_bound(off, nseg, n, static_cast<uint64_t>(t0) << kUniqTileShift) : 0;
    const bool vec_ok = (reinterpret_cast<uintptr_t>(values) & 15u) == 0;
    const auto apply = [op](Item a, Item b) { return seg_apply(op, a, b); };
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint64_t tile_start = static_cast<uint64_t>(t) << kUniqTileShift;
        const uint64_t tile_end = tile_start + kUniqTileKeys;
        if (tile_start >= hi || tile_end <= lo) continue;         // (uniform)
        const uint64_t first = tile_start + static_cast<uint64_t>(tid) * kUniqKpt;
        const bool whole = tile_start >= lo && tile_end <= hi;    // (uniform; hi <= n)
        Val v[kUniqKpt];
        scan_load_values(values, first, lo, hi, whole && vec_ok, v);
        uint64_t s0_next;
        const uint32_t rbits = scan_tile_restarts<uint32_t, false, true>(nullptr, n, off, nseg, lo, hi, tile_start, s0, sh, s0_next, &ids);
        if (!off) {
            __syncthreads();                                      // (the walk has no barrier of its own then)
        }
        const uint32_t* seg_last = ids.last + tid * kUniqKpt;     // seg_last[j]: the segment that began in this tile and ends with the thread's element j
        // a stop at off[S] when it falls inside the tile: what follows it belongs to no segment.  It comes after every restart.
        uint32_t fbits = rbits;
        if (hi > tile_start && hi >= first && hi < first + kUniqKpt) {
            fbits |= 1u << static_cast<uint32_t>(hi - first);
        }

        // 1. the thread's 16, left to right: pre = what comes before its first flag, acc = from its last flag on; a segment between two
        //    flags of one thread is complete and is stored at once
        Item pre = seg_item<Val, ARG>(v[0], static_cast<uint32_t>(first));
        Item acc = pre;
#pragma unroll
        for (int j = 1; j < kUniqKpt; ++j) {
            const Item x = seg_item<Val, ARG>(v[j], static_cast<uint32_t>(first + j));
            const bool flag = ((fbits >> j) & 1u) != 0;
            const bool earlier = (fbits & ((1u << j) - 1u)) != 0;     // an earlier flag in this thread: a restart (the stop is the last flag)
            if (flag && earlier) {
                seg_store<Val, ARG>(off, n, seg_last[j - 1], acc, vout, iout);
            }
            pre = seg_select(flag && !earlier, acc, pre);
            acc = seg_select(flag, x, apply(acc, x));
        }
        const uint32_t f = fbits != 0 ? 1u : 0u;

        // 2. the tile level: x = T(tid), ex = T(tid - 1)
        Item x, ex;
        uint32_t xf, exf;
        scan_tile_threads_with(apply, acc, f, ss, x, xf, ex, exf);

        // 3. the segment that the thread's first flag ends
        if (f) {
            const uint32_t j0 = static_cast<uint32_t>(__ffs(fbits)) - 1u;
            if (tid > 0 || j0 > 0) {
                const Item closed = seg_select(tid == 0, pre, seg_select(j0 > 0, apply(ex, pre), ex));
                if (tid > 0 && exf) {                             // it began at a restart of this tile
                    seg_store<Val, ARG>(off, n, ids.last[tid * kUniqKpt + j0 - 1u], closed, vout, iout);
                } else {                                          // the tile's first flag: what comes before it continues an earlier tile's segment
                    seg_put<Val, ARG>(lead, lead_pos, t, closed);
                }
            }
        }
        // 4. the tile's end
        if (tid == kUniqThreads - 1) {
            uint32_t open = kSegRedNone;
            if (tile_end <= hi) {                                 // (else the stop closed the last segment)
                if (!xf) {
                    seg_put<Val, ARG>(lead, lead_pos, t, x);      // the whole tile lies inside one segment
                } else if (ids.open == kSegRedNone) {             // the last segment that began here ends with the tile
                    seg_store<Val, ARG>(off, n, ids.last[kUniqTileKeys - 1], x, vout, iout);
                } else {
                    seg_put<Val, ARG>(tail, tail_pos, t, x);
                    open = ids.open;
                }
            }
            open_seg[t] = open;
        }
        s0 = s0_next;
        __syncthreads();
    }
}

// Any grid: the segments and the open tiles are taken grid-stride.  With bad offsets nothing is written and the first bad segment + 1
// goes to the mapped host words with the call's id, unless an earlier report is still pending there (as bins_zero_kernel does).
template <typename Val, bool ARG>
__global__ __launch_bounds__(kSegRedJoinThreads) void segreduce_join_kernel(uint64_t n, const uint64_t* __restrict__ off, uint64_t nseg,
                                                                            const uint32_t* __restrict__ bad, uint32_t ntiles, uint32_t op,
                                                                            Val* __restrict__ vout, uint32_t* __restrict__ iout,
                                                                            const Val* __restrict__ lead, const Val* __restrict__ tail,
                                                                            const uint32_t* __restrict__ lead_pos, const uint32_t* __restrict__ tail_pos,
                                                                            const uint32_t* __restrict__ open_seg, uint32_t* status_host, uint32_t call_id)
{
    using Item = SegItem<Val, ARG>;
    constexpr uint32_t WAVES = kSegRedJoinThreads / kWave;
    __shared__ Item wval[WAVES];
    __shared__ uint32_t whas[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t b = *bad;
    if (b != kUniqNoBad) {
        if (blockIdx.x == 0 && tid == 0 && __hip_atomic_load(status_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
            __hip_atomic_store(status_host + 1, call_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(status_host, b + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);        // (after the call's id)
        }
        return;
    }
    // (1) the empty segments
    const Val id = red_identity<Val>(op);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kSegRedJoinThreads;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kSegRedJoinThreads + tid; s < nseg; s += stride) {
        if (uniq_off(off, s, n) == uniq_off(off, s + 1, n)) {
            if (vout) {
                vout[s] = id;
            }
            if constexpr (ARG) {
                iout[s] = kSegRedNone;
            }
        }
    }
    // (2) the segments that cross a tile edge
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    if (lo >= hi) return;
    const uint32_t t_first = static_cast<uint32_t>(lo >> kUniqTileShift);
    const uint32_t t_end = static_cast<uint32_t>(min(static_cast<uint64_t>(ntiles), (hi + kUniqTileKeys - 1) >> kUniqTileShift));
    const auto apply = [op](Item a, Item c) { return seg_apply(op, a, c); };
#pragma unroll 1
    for (uint64_t t64 = static_cast<uint64_t>(t_first) + blockIdx.x; t64 < t_end; t64 += gridDim.x) {
        const uint32_t t = static_cast<uint32_t>(t64);
        const uint32_t s = open_seg[t];                          // (uniform)
        if (s == kSegRedNone) continue;
        const uint32_t u = static_cast<uint32_t>((uniq_off(off, static_cast<uint64_t>(s) + 1, n) - 1) >> kUniqTileShift);      // > t, < t_end
        const bool small = u - t <= kWave;                        // (uniform) only the first wave has partials: no barrier needed
        if (small && wave > 0) continue;
        Item p = seg_item<Val, ARG>(Val{0}, 0u);
        uint32_t has = 0;
#pragma unroll 1
        for (uint64_t w = static_cast<uint64_t>(t) + 1 + tid; w <= u; w += kSegRedJoinThreads) {
            const Item x = seg_get<Val, ARG>(lead, lead_pos, static_cast<uint32_t>(w));
            p = seg_select(has != 0, apply(p, x), x);
            has = 1;
        }
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const Item y = red_shfl_down(p, d);
            const uint32_t yh = __shfl_down(has, d);
            if (lane + d < kWave && yh) {
                p = seg_select(has != 0, apply(p, y), y);
                has = 1;
            }
        }
        if (!small) {
            if (lane == 0) {
                wval[wave] = p;
                whas[wave] = has;
            }
            __syncthreads();
            if (tid == 0) {
#pragma unroll
                for (uint32_t w = 1; w < WAVES; ++w) {
                    if (whas[w]) {
                        p = apply(p, wval[w]);                    // (wave 0 has a partial whenever a later wave has one)
                    }
                }
            }
        }
        if (tid == 0) {
            const Item a = seg_get<Val, ARG>(tail, tail_pos, t);
            seg_store<Val, ARG>(off, n, s, seg_select(has != 0, apply(a, p), a), vout, iout);
        }
        if (!small) {
            __syncthreads();
        }
    }
}

}  // namespace rsx
