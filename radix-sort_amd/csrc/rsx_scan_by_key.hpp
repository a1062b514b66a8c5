// rsx_scan_by_key.hpp — kernels of rsx_segmented_scan: the running sum / min / max of the values inside every segment and every run of
// adjacent equal keys.  Included by rsx_capi.hip (host side: capi_scan.inc).
//
//   (unique_reset_kernel + unique_validate_kernel, unchanged: the first bad segment of the offsets, one word)
//   scan_tile_reduce_kernel  per 4096-element tile of the global grid: the restarts (segment starts, and with keys the heads that
//                            uniq_tile_heads finds), tail[t] = the fold from the tile's last restart to its end (the whole tile without
//                            one), flags[t] = has a restart | is in range.
//   scan_carry_kernel        ONE workgroup: the restart-flagged inclusive scan of the tails, 1024 tiles per step; carry[t + 1] = the fold
//                            of everything from the last restart up to the end of tile t.  Reports bad offsets.
//   scan_tile_kernel         per tile again: re-reads the values, scans the tile, puts carry[t] on the left of what lies before the
//                            tile's first restart, stores (16-byte stores where the output pointer allows).
//
// A position i in [off[0], off[S]) is a RESTART iff it starts a non-empty segment or (keys given) key[i] != key[i-1] by bits.  off[0] is
// one whenever the range is not empty, so every tile after the first in range has a carry and the first needs none.
//
// ORDER OF A FLOAT SUM.  a o b has the EARLIER elements on the left throughout; "flagged" means that a restart on the right side cuts the
// left side off: (a, fa) o (b, fb) = fb ? (b, 1) : (a o b, fa).  Elements outside [off[0], off[S]) count as 0 without a restart; a restart
// always stands between them and anything that is stored.  F(i), the inclusive fold at position i, is defined on three levels, and the
// value AT THE END of a level's unit is that of the level above:
//   thread  (16 elements, thread q of a tile holds 16q .. 16q+15)  a[0] = v[0], a[j] = flagged a[j-1] o v[j], left to right.
//           F(i) = G o a[j] for j < 15 before the thread's first restart, a[j] after it.  G = F(the element before the thread's first).
//   tile    (256 threads)  the threads' a[15] are joined by a flagged Hillis-Steele scan over the 64 lanes of a wave (distances 1, 2, 4, ...
//           32: x[l] = x[l-d] o x[l]), the four wave totals are folded left to right and go on the left of the lanes' x: that is T(q).
//           F(last element of thread q < 255) = carry[t] o T(q) before the tile's first restart, T(q) after it.  tail[t] = T(255).
//   grid    blocks of 1024 tiles, aligned on the global tile grid: the tails of 64 tiles (one wave) joined by the same flagged
//           Hillis-Steele scan, the 16 wave totals of the block folded left to right onto R, the flagged fold of all earlier blocks' wave
//           totals (left to right, beginning with the block that holds off[0]); carry[t + 1] = R o (wave totals before) o x[lane].
//           F(last element of tile t) = carry[t + 1].
// The inclusive result is F(i).  The exclusive result is F(i - 1), or the identity at a restart: the same bits, one place further on.
// Every choice is a function of the element's position on the global tile grid and of where the restarts are, i.e. of keys, offsets and
// n alone: not of the grid size, the workgroup a tile lands in, the engine's capacity or the stream.  There is no atomic on the value path
// and no workgroup waits for another: the three launches are ordered by the stream.
//
// The op is a kernel argument (wave-uniform) and so are the flags, as in rsx_reduce.hpp; instantiations: value kind x {no keys, u32, u64}.
#pragma once

#include "rsx_reduce.hpp"

#include <limits>

namespace rsx {

constexpr uint32_t kScanExclusive = 2u;                           // RSX_SCAN_EXCLUSIVE
constexpr uint32_t kScanRestart = 1u, kScanLive = 2u;             // flags[t]
constexpr int kScanCarryThreads = 1024;

template <typename Val>
struct ScanShared {
    Val wval[kUniqThreads / kWave];
    uint32_t wflag[kUniqThreads / kWave];
};

// The restart bits of the thread's 16 elements (bit j = element 16 * tid + j of the tile).  KEYS: uniq_tile_heads.  Without keys only the
// segment starts count: the same walk over the offsets that fall into the tile (s0 = first s with off[s] >= tile_start), without a key
// being read; without offsets either, the one restart is element 0.  Two barriers unless there are neither keys nor offsets; sh is
// rewritten by the next call, which the caller separates from this one's readers by a barrier of its own.
// ids (rsx_segreduce.hpp, without keys only): the walk also notes which segment ENDS at each element of the tile, for the segments that
// began in the tile, and which one began in it and goes on behind it.
struct ScanSegIds {
    uint32_t last[kUniqTileKeys];                                  // last[x] = s: element x is the last of segment s (written where that holds only)
    uint32_t open;                                                 // the segment that began in the tile and ends behind it, or 0xFFFFFFFF
};

template <typename Key, bool KEYS, bool IDS = false>
__device__ __forceinline__ uint32_t scan_tile_restarts(const Key* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ off, uint64_t nseg,
                                                       uint64_t lo, uint64_t hi, uint64_t tile_start, uint64_t s0, UniqShared& sh, uint64_t& s0_next,
                                                       ScanSegIds* ids = nullptr)
{
    if constexpr (KEYS) {
        Key k[kUniqKpt];
        uint32_t hbits, sbits;
        uniq_tile_heads(keys, n, off, nseg, lo, hi, tile_start, s0, sh, k, hbits, sbits, s0_next);
        return hbits;
    } else {
        const uint32_t tid = threadIdx.x;
        if (!off) {                                               // (uniform) one segment [0, n)
            s0_next = s0;
            if constexpr (IDS) {                                  // (the caller's barrier comes before anybody reads these)
                if (tid == 0) {
                    ids->open = tile_start == 0 && n > kUniqTileKeys ? 0u : 0xFFFFFFFFu;
                    if (tile_start == 0 && n <= kUniqTileKeys && n > 0) {
                        ids->last[n - 1] = 0u;
                    }
                }
            }
            return tile_start == 0 && tid == 0 ? 1u : 0u;
        }
        if (tid < kUniqTileKeys / 32) {
            sh.segbits[tid] = 0;
        }
        if (tid == 0) {
            sh.next_s0 = static_cast<uint32_t>(nseg + 1);
            if constexpr (IDS) {
                ids->open = 0xFFFFFFFFu;
            }
        }
        __syncthreads();
        const uint64_t tile_end = tile_start + kUniqTileKeys;
        for (uint64_t s = s0 + tid; s <= nseg; s += kUniqThreads) {
            const uint64_t o = off[s];
            if (o >= tile_end) {
                atomicMin(&sh.next_s0, static_cast<uint32_t>(s));
                break;
            }
            if (s < nseg && off[s + 1] > o) {                     // a non-empty segment starts here
                const uint32_t x = static_cast<uint32_t>(o - tile_start);
                atomicOr(&sh.segbits[x >> 5], 1u << (x & 31u));
                if constexpr (IDS) {
                    const uint64_t e = off[s + 1];
                    if (e <= tile_end) {
                        ids->last[static_cast<uint32_t>(e - 1 - tile_start)] = static_cast<uint32_t>(s);
                    } else {
                        ids->open = static_cast<uint32_t>(s);     // (one segment at most)
                    }
                }
            }
        }
        __syncthreads();
        s0_next = sh.next_s0;
        return (sh.segbits[tid >> 1] >> ((tid & 1u) * 16u)) & 0xFFFFu;
    }
}

// The thread's 16 values: only positions in [lo, hi) are read, the others are 0.  16-byte loads on whole tiles of an aligned pointer.
template <typename Val>
__device__ __forceinline__ void scan_load_values(const Val* values, uint64_t first, uint64_t lo, uint64_t hi, bool vec, Val (&v)[kUniqKpt])
{
    constexpr int VV = 16 / sizeof(Val);
    if (vec) {
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

// The tile level.  In: acc = the thread's fold from its last restart on (all 16 without one), f = it has a restart.  Out: (x, xf) = T(tid)
// and whether a restart of the tile lies at or before the thread's end; (ex, exf) = the same for the thread before (tid 0: exf = 0 and ex
// is not to be used).  One barrier; ss is rewritten by the next call, after the caller's own barrier.
// apply(a, b) is a o b with a the earlier side: the scan's red_apply, or rsx_segreduce.hpp's fold of (value, position) pairs.
template <typename Val, typename Apply>
__device__ __forceinline__ void scan_tile_threads_with(Apply apply, Val acc, uint32_t f, ScanShared<Val>& ss, Val& x, uint32_t& xf, Val& ex, uint32_t& exf)
{
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    x = acc;
    xf = f;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const Val y = red_shfl_up(x, d);
        const uint32_t yf = __shfl_up(xf, d);
        if (lane >= static_cast<uint32_t>(d)) {
            x = xf ? x : apply(y, x);
            xf |= yf;
        }
    }
    if (lane == kWave - 1) {
        ss.wval[wave] = x;
        ss.wflag[wave] = xf;
    }
    ex = red_shfl_up(x, 1);
    exf = __shfl_up(xf, 1);
    if (lane == 0) {
        exf = 0;
    }
    __syncthreads();
    if (wave > 0) {
        Val pv = ss.wval[0];
        uint32_t pf = ss.wflag[0];
#pragma unroll
        for (uint32_t w = 1; w < kUniqThreads / kWave; ++w) {
            if (w < wave) {
                const uint32_t tf = ss.wflag[w];
                const Val tv = ss.wval[w];
                pv = tf ? tv : apply(pv, tv);
                pf |= tf;
            }
        }
        if (lane == 0) {
            ex = pv;
            exf = pf;
        } else {
            ex = exf ? ex : apply(pv, ex);
            exf |= pf;
        }
        x = xf ? x : apply(pv, x);
        xf |= pf;
    }
}

template <typename Val>
__device__ __forceinline__ void scan_tile_threads(uint32_t op, Val acc, uint32_t f, ScanShared<Val>& ss, Val& x, uint32_t& xf, Val& ex, uint32_t& exf)
{
    scan_tile_threads_with([op](Val a, Val b) { return red_apply(op, a, b); }, acc, f, ss, x, xf, ex, exf);
}

// Workgroup b takes the tiles [b * chunk, (b + 1) * chunk); tiles outside [off[0], off[S]) are neither read nor given partials.
template <typename Key, typename Val, bool KEYS>
__global__ __launch_bounds__(kUniqThreads) void scan_tile_reduce_kernel(const Key* __restrict__ keys, const Val* __restrict__ values, uint64_t n,
                                                                        const uint64_t* __restrict__ off, uint64_t nseg, const uint32_t* __restrict__ bad,
                                                                        uint32_t ntiles, uint32_t chunk, uint32_t op, Val* __restrict__ tail,
                                                                        uint32_t* __restrict__ flags)
{
    __shared__ UniqShared sh;
    __shared__ ScanShared<Val> ss;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    uint64_t s0 = KEYS || off ? uniq_lower_bound(off, nseg, n, static_cast<uint64_t>(t0) << kUniqTileShift) : 0;
    const bool vec_ok = (reinterpret_cast<uintptr_t>(values) & 15u) == 0;
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
        const uint32_t rbits = scan_tile_restarts<Key, KEYS>(keys, n, off, nseg, lo, hi, tile_start, s0, sh, s0_next);
        Val acc = v[0];
#pragma unroll
        for (int j = 1; j < kUniqKpt; ++j) {
            acc = ((rbits >> j) & 1u) ? v[j] : red_apply(op, acc, v[j]);
        }
        Val x, ex;
        uint32_t xf, exf;
        scan_tile_threads(op, acc, rbits != 0 ? 1u : 0u, ss, x, xf, ex, exf);
        if (tid == kUniqThreads - 1) {
            tail[t] = x;
            flags[t] = (xf ? kScanRestart : 0u) | kScanLive;
        }
        s0 = s0_next;
        __syncthreads();
    }
}

// One workgroup, whatever n is: the grid level of the order above.  carry has ntiles + 1 entries; entry t + 1 is written for every tile t
// of [off[0], off[S]).  With bad offsets nothing is written and the first bad segment + 1 goes to the mapped host word, unless an earlier
// report is still pending there (as unique_offsets_kernel does).
template <typename Val>
__global__ __launch_bounds__(kScanCarryThreads) void scan_carry_kernel(uint64_t n, const uint64_t* __restrict__ off, uint64_t nseg,
                                                                       const uint32_t* __restrict__ bad, uint32_t ntiles, uint32_t op,
                                                                       const Val* __restrict__ tail, const uint32_t* __restrict__ flags,
                                                                       Val* __restrict__ carry, uint32_t* status_host)
{
    constexpr uint32_t WAVES = kScanCarryThreads / kWave;
    __shared__ Val wval[WAVES];
    __shared__ uint32_t wflag[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t b = *bad;
    if (b != kUniqNoBad) {
        if (tid == 0 && __hip_atomic_load(status_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
            __hip_atomic_store(status_host, b + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    if (lo >= hi) return;
    const uint32_t t_first = static_cast<uint32_t>(lo >> kUniqTileShift);
    const uint32_t t_end = static_cast<uint32_t>(min(static_cast<uint64_t>(ntiles), (hi + kUniqTileKeys - 1) >> kUniqTileShift));
    Val run = Val{0};                                             // R: cut off by the restart at off[0] before anything is stored
    uint32_t runf = 0;
#pragma unroll 1
    for (uint32_t base = t_first & ~static_cast<uint32_t>(kScanCarryThreads - 1); base < t_end; base += kScanCarryThreads) {
        const uint32_t t = base + tid;
        const bool live = t >= t_first && t < t_end;
        Val x = live ? tail[t] : Val{0};
        uint32_t xf = live ? (flags[t] & kScanRestart) : 0u;
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
            wval[wave] = x;
            wflag[wave] = xf;
        }
        __syncthreads();
        Val pv = run;
#pragma unroll
        for (uint32_t w = 0; w < WAVES; ++w) {
            if (w == wave) {                                      // (wave-uniform) what lies before this wave
                pv = run;
            }
            const uint32_t tf = wflag[w];
            const Val tv = wval[w];
            run = tf ? tv : red_apply(op, run, tv);
            runf |= tf;
        }
        if (live) {
            carry[t + 1] = xf ? x : red_apply(op, pv, x);
        }
        __syncthreads();
    }
}

// values and out may be the same pointer (in place): a thread has read its 16 before it stores them, and nobody else reads them.
template <typename Key, typename Val, bool KEYS>
__global__ __launch_bounds__(kUniqThreads) void scan_tile_kernel(const Key* __restrict__ keys, const Val* values, uint64_t n,
                                                                 const uint64_t* __restrict__ off, uint64_t nseg, const uint32_t* __restrict__ bad,
                                                                 uint32_t ntiles, uint32_t chunk, uint32_t op, uint32_t scan_flags,
                                                                 const Val* __restrict__ carry, Val* out)
{
    __shared__ UniqShared sh;
    __shared__ ScanShared<Val> ss;
    constexpr int VV = 16 / sizeof(Val);
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    if (lo >= hi) return;
    const uint32_t t_first = static_cast<uint32_t>(lo >> kUniqTileShift);
    uint64_t s0 = KEYS || off ? uniq_lower_bound(off, nseg, n, static_cast<uint64_t>(t0) << kUniqTileShift) : 0;
    const bool in_ok = (reinterpret_cast<uintptr_t>(values) & 15u) == 0, out_ok = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    const bool exclusive = (scan_flags & kScanExclusive) != 0;
    const Val id = red_identity<Val>(op);
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint64_t tile_start = static_cast<uint64_t>(t) << kUniqTileShift;
        const uint64_t tile_end = tile_start + kUniqTileKeys;
        if (tile_start >= hi || tile_end <= lo) continue;         // (uniform)
        const uint64_t first = tile_start + static_cast<uint64_t>(tid) * kUniqKpt;
        const bool whole = tile_start >= lo && tile_end <= hi;    // (uniform; hi <= n)
        const bool hasc = t > t_first;                            // (uniform) the first tile in range begins before or at the restart off[0]
        Val v[kUniqKpt];
        scan_load_values(values, first, lo, hi, whole && in_ok, v);
        const Val c = hasc ? carry[t] : Val{0};
        uint64_t s0_next;
        const uint32_t rbits = scan_tile_restarts<Key, KEYS>(keys, n, off, nseg, lo, hi, tile_start, s0, sh, s0_next);

        // the thread level: v[j] := a[j]
#pragma unroll
        for (int j = 1; j < kUniqKpt; ++j) {
            v[j] = ((rbits >> j) & 1u) ? v[j] : red_apply(op, v[j - 1], v[j]);
        }
        Val x, ex;
        uint32_t xf, exf;
        scan_tile_threads(op, v[kUniqKpt - 1], rbits != 0 ? 1u : 0u, ss, x, xf, ex, exf);

        // G = F(the element before the thread's first); there is none before the first element in range
        Val g;
        bool gv;
        if (tid == 0) {
            g = c;
            gv = hasc;
        } else {
            g = exf || !hasc ? ex : red_apply(op, c, ex);
            gv = true;
        }
        // v[j] := F: thread level for j < 15, the tile's (thread 255: the grid's) value at the thread's end
        Val prev = gv ? g : id;                                   // F(i - 1) of the element in hand
#pragma unroll
        for (int j = 0; j < kUniqKpt; ++j) {
            const bool cut = (rbits & ((2u << j) - 1u)) != 0;     // a restart of this thread at or before j
            Val fj;
            if (j < kUniqKpt - 1) {
                fj = cut || !gv ? v[j] : red_apply(op, g, v[j]);
            } else if (exclusive) {
                fj = v[j];                                        // (not stored)
            } else if (tid == kUniqThreads - 1) {
                fj = carry[t + 1];
            } else {
                fj = xf || !hasc ? x : red_apply(op, c, x);
            }
            if (exclusive) {
                v[j] = ((rbits >> j) & 1u) ? id : prev;
                prev = fj;
            } else {
                v[j] = fj;
            }
        }

        if (whole && out_ok) {
#pragma unroll
            for (int q = 0; q < kUniqKpt / VV; ++q) {
                struct alignas(16) ValVec { Val x[VV]; };
                ValVec vv;
#pragma unroll
                for (int k = 0; k < VV; ++k) {
                    vv.x[k] = v[q * VV + k];
                }
                *reinterpret_cast<ValVec*>(out + first + q * VV) = vv;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                const uint64_t i = first + j;
                if (i >= lo && i < hi) {
                    out[i] = v[j];
                }
            }
        }
        s0 = s0_next;
        __syncthreads();
    }
}

}  // namespace rsx
