// rsx_reduce.hpp — kernels of rsx_segmented_reduce_by_key: sum / min / max of the values that came with the equal keys of every segment.
// The grouping is rsx_segmented_unique's (rsx_unique.hpp: validate, sort with the positions as payload, heads per tile, table scan, run
// offsets); these two kernels replace unique_write_kernel.  Included by rsx_capi.hip (host side: capi_reduce.inc).
//
//   reduce_tile_kernel    per 4096-key tile of the global grid: heads as uniq_tile_heads finds them, the element's value (values[perm[i]]
//                         after a sort, values[i] in consecutive mode), a head-flagged segmented reduction over the tile.  Runs that begin
//                         AND end inside the tile store their value at run id table[tile] + rank; every head stores its key and position.
//                         What is left goes to per-tile partials: lead[t] = the elements before the tile's first head, tail[t] = the
//                         elements from its last head on, flags[t] says which of the two exist.
//   reduce_carry_kernel   one wave per tile with a tail: total = tail[t] o lead[t+1] o lead[t+2] o ... up to and including the first later
//                         tile that has a head, never beyond off[S]; stored at run id table[t+1] - 1.
//   (unique_counts_kernel, unchanged: the counts from the heads' positions)
//
// ORDER OF A FLOAT SUM.  a o b is written with the EARLIER elements on the left throughout.  Inside a tile: thread t folds its 16 elements
// left to right; a Hillis-Steele scan over the 64 lanes of a wave (distances 1, 2, 4, ... 32) joins the threads' partials; the four wave
// totals are folded left to right.  Across tiles: lane l of the carry wave folds lead[t+1+l], lead[t+1+l+64], ... left to right, the 64
// lane partials are joined by a tree (distances 1, 2, ... 32, lower lane on the left), and the tail goes on the left of that.  Every
// choice is a function of the element's position on the global tile grid and of where the heads are, i.e. of keys, offsets and n alone:
// not of the grid size, the workgroup a tile lands in, the engine's capacity or the stream.  There is no atomic on the value path.
//
// The op is a kernel argument (wave-uniform), not a template parameter: the value path is a handful of VALU instructions per element beside
// a gather from HBM, and 2 key widths x 4 value kinds x 2 load forms are instantiations enough.
#pragma once

#include "rsx_unique.hpp"

#include <limits>
#include <type_traits>

namespace rsx {

constexpr uint32_t kRedSum = 0, kRedMin = 1, kRedMax = 2;
constexpr uint32_t kRedTail = 1u, kRedLead = 2u, kRedStop = 4u;     // flags[t]: tail[t] belongs to a run; lead[t] holds something; a carry ends here
constexpr int kRedCarryThreads = 256;

// integers wrap (the sum is taken on the unsigned image); float min / max return NaN if either side is NaN (torch's amin / amax)
template <typename Val>
__device__ __forceinline__ Val red_apply(uint32_t op, Val a, Val b)
{
    if constexpr (std::is_integral<Val>::value) {
        using U = typename std::make_unsigned<Val>::type;
        const Val s = static_cast<Val>(static_cast<U>(a) + static_cast<U>(b));
        return op == kRedSum ? s : op == kRedMin ? (b < a ? b : a) : (b > a ? b : a);
    } else {
        const Val s = a + b;
        const Val lo = (b < a || b != b) ? b : a;
        const Val hi = (b > a || b != b) ? b : a;
        return op == kRedSum ? s : op == kRedMin ? lo : hi;
    }
}

// the op's identity: what a restart holds in an exclusive scan (rsx_scan_by_key.hpp) and what an empty segment reduces to (rsx_segreduce.hpp)
template <typename Val>
__device__ __forceinline__ Val red_identity(uint32_t op)
{
    if constexpr (std::is_integral<Val>::value) {
        return op == kRedSum ? Val{0} : op == kRedMin ? std::numeric_limits<Val>::max() : std::numeric_limits<Val>::lowest();
    } else {
        return op == kRedSum ? Val{0} : op == kRedMin ? std::numeric_limits<Val>::infinity() : -std::numeric_limits<Val>::infinity();
    }
}

template <typename Val>
__device__ __forceinline__ Val red_shfl_up(Val v, int d)
{
    uint32_t w[sizeof(Val) / 4];
    __builtin_memcpy(w, &v, sizeof(Val));
#pragma unroll
    for (unsigned c = 0; c < sizeof(Val) / 4; ++c) {
        w[c] = __shfl_up(w[c], d);
    }
    __builtin_memcpy(&v, w, sizeof(Val));
    return v;
}

template <typename Val>
__device__ __forceinline__ Val red_shfl_down(Val v, int d)
{
    uint32_t w[sizeof(Val) / 4];
    __builtin_memcpy(w, &v, sizeof(Val));
#pragma unroll
    for (unsigned c = 0; c < sizeof(Val) / 4; ++c) {
        w[c] = __shfl_down(w[c], d);
    }
    __builtin_memcpy(&v, w, sizeof(Val));
    return v;
}

template <typename Val>
struct RedShared {
    Val wval[kUniqThreads / kWave];
    uint32_t wflag[kUniqThreads / kWave];
    uint32_t lead0;                                                // kRedLead unless the tile's very first element is flagged
};

// PERM: perm[i] is the original position of grouped element i (after a sort), else it is i itself.  counts are taken from hp afterwards.
template <typename Key, typename Val, bool PERM>
__global__ __launch_bounds__(kUniqThreads) void reduce_tile_kernel(const Key* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                                   const Val* __restrict__ values, uint64_t n, const uint64_t* __restrict__ off,
                                                                   uint64_t nseg, const uint32_t* __restrict__ bad, const uint32_t* __restrict__ table,
                                                                   uint32_t ntiles, uint32_t chunk, uint32_t op, Key* __restrict__ kout,
                                                                   Val* __restrict__ vout, uint32_t* __restrict__ hp, Val* __restrict__ lead,
                                                                   Val* __restrict__ tail, uint32_t* __restrict__ flags)
{
    __shared__ UniqShared sh;
    __shared__ RedShared<Val> rs;
    constexpr int VV = 16 / sizeof(Val);
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    uint64_t s0 = uniq_lower_bound(off, nseg, n, static_cast<uint64_t>(t0) << kUniqTileShift);
    const bool vec_ok = (reinterpret_cast<uintptr_t>(values) & 15u) == 0;
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint64_t tile_start = static_cast<uint64_t>(t) << kUniqTileShift;
        const uint64_t tile_end = tile_start + kUniqTileKeys;
        if (tile_start >= hi || tile_end <= lo) continue;         // (uniform) no element of a run: nothing reads this tile's partials
        const uint64_t first = tile_start + static_cast<uint64_t>(tid) * kUniqKpt;
        const uint32_t tbase = table[t];
        const bool whole = tile_start >= lo && tile_end <= hi;    // (uniform) every element of the tile takes part (hi <= n)

        // the values: only positions in [lo, hi) are read; the others get a stand-in that no run ever sees
        Val v[kUniqKpt];
        if constexpr (PERM) {
            uint32_t p[kUniqKpt];
            if (whole) {
#pragma unroll
                for (int q = 0; q < kUniqKpt / 4; ++q) {
                    const U32x4 pv = *reinterpret_cast<const U32x4*>(perm + first + q * 4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        p[q * 4 + c] = pv.v[c];
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < kUniqKpt; ++j) {
                    const uint64_t i = first + j;
                    p[j] = i >= lo && i < hi ? perm[i] : 0xFFFFFFFFu;
                }
            }
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                v[j] = p[j] >= lo && p[j] < hi ? values[p[j]] : Val{0};
            }
        } else {
            if (whole && vec_ok) {
#pragma unroll
                for (int q = 0; q < kUniqKpt / VV; ++q) {
                    struct alignas(16) ValVec { Val x[VV]; };
                    const ValVec vv = *reinterpret_cast<const ValVec*>(values + first + q * VV);
#pragma unroll
                    for (int c = 0; c < VV; ++c) {
                        v[q * VV + c] = vv.x[c];
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < kUniqKpt; ++j) {
                    const uint64_t i = first + j;
                    v[j] = i >= lo && i < hi ? values[i] : Val{0};
                }
            }
        }

        Key k[kUniqKpt];
        uint32_t hbits, sbits;
        uint64_t s0_next;
        uniq_tile_heads(keys, n, off, nseg, lo, hi, tile_start, s0, sh, k, hbits, sbits, s0_next);
        uint32_t total;
        const uint32_t before = block_exclusive_scan<kUniqThreads>(static_cast<uint32_t>(__popc(hbits)), sh.wtot, total);
        const uint32_t base = tbase + before;                     // run id of the thread's first head
        // a stop at off[S] when it falls inside the tile: what follows it belongs to no run.  It comes after every head.
        uint32_t fbits = hbits;
        if (hi >= first && hi < first + kUniqKpt && hi > tile_start) {
            fbits |= 1u << static_cast<uint32_t>(hi - first);
        }
        const bool hi_inside = hi > tile_start && hi < tile_end;

        // 1. the thread's 16, left to right: pre = what comes before its first flag (all 16 without one), acc = from its last flag on;
        //    the runs between two flags of one thread are complete and are stored at once
        Val pre = v[0], acc = v[0];
        uint32_t g = base - 1u;                                   // run id of the head last passed
#pragma unroll
        for (int j = 0; j < kUniqKpt; ++j) {
            const bool flag = ((fbits >> j) & 1u) != 0;
            if (flag) {
                if ((fbits & ((1u << j) - 1u)) != 0) {            // an earlier flag in this thread: it was a head (the stop is the last flag)
                    vout[g] = acc;
                } else if (j > 0) {
                    pre = acc;
                }
                if ((hbits >> j) & 1u) {
                    ++g;
                    kout[g] = k[j];
                    if (hp) {
                        hp[g] = static_cast<uint32_t>(first + j);
                    }
                }
                acc = v[j];
            } else if (j > 0) {
                acc = red_apply(op, acc, v[j]);
            }
        }
        const uint32_t f = fbits != 0 ? 1u : 0u;
        if (!f) {
            pre = acc;
        }

        // 2. flagged inclusive scan of (f, acc) over the wave, the wave totals through LDS
        Val x = acc;
        uint32_t xf = f;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const Val y = red_shfl_up(x, d);
            const uint32_t yf = __shfl_up(xf, d);
            if (lane >= static_cast<uint32_t>(d)) {
                x = xf ? x : red_apply(op, y, x);
                xf |= yf;
            }
        }
        if (lane == kWave - 1) {
            rs.wval[wave] = x;
            rs.wflag[wave] = xf;
        }
        if (tid == 0) {
            rs.lead0 = (fbits & 1u) ? 0u : kRedLead;
        }
        Val ex = red_shfl_up(x, 1);                                // what the threads before hold open (tid 0: nothing)
        uint32_t exf = __shfl_up(xf, 1);
        __syncthreads();
        if (wave > 0) {
            Val pv = rs.wval[0];
            uint32_t pf = rs.wflag[0];
#pragma unroll
            for (uint32_t w = 1; w < kUniqThreads / kWave; ++w) {
                if (w < wave) {
                    const uint32_t tf = rs.wflag[w];
                    const Val tv = rs.wval[w];
                    pv = tf ? tv : red_apply(op, pv, tv);
                    pf |= tf;
                }
            }
            if (lane == 0) {
                ex = pv;
                exf = pf;
            } else {
                ex = exf ? ex : red_apply(op, pv, ex);
                exf |= pf;
            }
        }

        // 3. the run that the thread's first flag ends
        if (f) {
            const bool has_pre = (fbits & 1u) == 0;
            const Val closed = tid == 0 ? pre : has_pre ? red_apply(op, ex, pre) : ex;
            if (tid > 0 && exf) {
                vout[base - 1u] = closed;                         // it began at a head of this tile
            } else {
                lead[t] = closed;                                 // the tile's first flag: what comes before it continues an earlier tile's run
            }
        }
        if (tid == kUniqThreads - 1) {
            const Val all = f ? acc : red_apply(op, ex, acc);      // (f: the scan kept acc; else everything open before joins in)
            const uint32_t allf = f | exf;
            if (allf) {
                tail[t] = all;
            } else {
                lead[t] = all;
            }
            flags[t] = (allf && !hi_inside ? kRedTail : 0u) | (allf ? kRedStop : 0u) | rs.lead0;
        }
        s0 = s0_next;
        __syncthreads();
    }
}

// One wave per tile whose last run is still open at the tile's end (kRedTail).  The tiles it may look at end with off[S]; tiles outside
// [off[0], off[S]) were not written by this call and are not looked at.
template <typename Val>
__global__ __launch_bounds__(kRedCarryThreads) void reduce_carry_kernel(uint64_t n, const uint64_t* __restrict__ off, uint64_t nseg,
                                                                        const uint32_t* __restrict__ bad, const uint32_t* __restrict__ table,
                                                                        uint32_t ntiles, uint32_t op, Val* __restrict__ vout,
                                                                        const Val* __restrict__ lead, const Val* __restrict__ tail,
                                                                        const uint32_t* __restrict__ flags)
{
    if (*bad != kUniqNoBad) return;
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t nwaves = gridDim.x * (kRedCarryThreads / kWave);
    const uint32_t end = static_cast<uint32_t>(min(static_cast<uint64_t>(ntiles), (hi + kUniqTileKeys - 1) >> kUniqTileShift));
#pragma unroll 1
    for (uint32_t t = blockIdx.x * (kRedCarryThreads / kWave) + threadIdx.x / kWave; t < end; t += nwaves) {
        const uint64_t tile_start = static_cast<uint64_t>(t) << kUniqTileShift;
        if (tile_start + kUniqTileKeys <= lo || (flags[t] & kRedTail) == 0) continue;      // (wave-uniform)
        Val part = Val{0};
        uint32_t has = 0;
#pragma unroll 1
        for (uint32_t u0 = t + 1; u0 < end; u0 += kWave) {
            const uint32_t u = u0 + lane;
            const uint32_t fl = u < end ? flags[u] : kRedStop;
            const unsigned long long stops = __ballot((fl & kRedStop) != 0);
            const uint32_t last = stops ? static_cast<uint32_t>(__ffsll(stops)) - 1u : kWave - 1u;
            if (u < end && lane <= last && (fl & kRedLead) != 0) {
                const Val x = lead[u];
                part = has ? red_apply(op, part, x) : x;
                has = 1;
            }
            if (stops) break;
        }
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const Val y = red_shfl_down(part, d);
            const uint32_t yh = __shfl_down(has, d);
            if (lane + d < kWave && yh) {
                part = has ? red_apply(op, part, y) : y;
                has = 1;
            }
        }
        if (lane == 0) {
            const Val a = tail[t];
            vout[table[t + 1] - 1u] = has ? red_apply(op, a, part) : a;
        }
    }
}

}  // namespace rsx
