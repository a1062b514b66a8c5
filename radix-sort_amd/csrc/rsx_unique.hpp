// rsx_unique.hpp — kernels of rsx_segmented_unique: the distinct keys of every segment [off[s], off[s+1]), their counts, first positions and
// the inverse map, from keys that are already grouped (the segmented / flat sort's output, or the raw input in consecutive mode).
// Included by rsx_capi.hip (host side: capi_unique.inc).
//
//   unique_reset_kernel      the first-bad-segment word := none (a kernel, so that a captured call replays it as written)
//   unique_validate_kernel   per segment: off[s+1] < off[s] or off[s+1] > n -> the first such segment (one word; every later kernel leaves at once)
//   unique_iota_kernel       0, 1, 2, ...: the positions a sort carries as its payload (written when the buffer grows, never again)
//   unique_count_kernel      per 4096-key tile of the global grid: heads (first keys of runs) -> flat [tile] table; for every off[s] inside the
//                            tile the heads of the tile before it -> run_offsets[s] (tile-local for now)
//   (scan_blocks_kernel + paste_scan_kernel, unchanged: the flat exclusive scan of that table, as the top-k's)
//   unique_offsets_kernel    per segment: run_offsets[s] += table[tile of off[s]]: final; reports a bad segment in consecutive mode
//   unique_write_kernel      per tile: recomputes the heads; run id g = table[tile] + rank; heads store key, first position and their own
//                            position hp[g]; every element stores inverse[position] = g - run_offsets[its segment]
//   unique_counts_kernel     per run: counts[g] = hp[g+1] - hp[g] (off[S] after the last run)
//
// An element i is a HEAD iff off[0] <= i < off[S] and (i starts a non-empty segment or key[i] != key[i-1]).  Segment starts: every workgroup
// walks a contiguous range of tiles, so ONE binary search in the offsets per workgroup finds the first off[s] >= its first tile, and each
// tile then walks the offsets that fall into it (256 at a time), setting a bit per start in LDS; where the walk stops is where the next
// tile's begins.  (A bitmap written by a per-segment kernel would cost n/8 bytes of memset and atomics per call and a dependent launch;
// the walk reads each offset twice per kernel, out of L2.)  Equality is equality of bit patterns, which is equality under every order map:
// the kernels need no codec.  d_offsets == NULL is the one segment [0, n) (nseg = 1).
#pragma once

#include "rsx_common.hpp"
#include "rsx_segmented.hpp"

namespace rsx {

constexpr int kUniqThreads = 256, kUniqKpt = 16;                // one tile = 256 x 16 keys, thread t holds keys 16t .. 16t+15
constexpr int kUniqTileShift = kSegTileShift;
constexpr uint32_t kUniqTileKeys = kSegTileKeys;
constexpr uint32_t kUniqNoBad = 0xFFFFFFFFu;
constexpr int kUniqSmallThreads = 256;

__device__ __forceinline__ uint64_t uniq_off(const uint64_t* __restrict__ off, uint64_t s, uint64_t n)
{
    return off ? off[s] : (s ? n : 0ull);
}

// first s in [0, nseg] with off[s] >= x, nseg + 1 if there is none (valid offsets are non-decreasing)
__device__ __forceinline__ uint64_t uniq_lower_bound(const uint64_t* __restrict__ off, uint64_t nseg, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = nseg + 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (uniq_off(off, mid, n) < x) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// no bad segment seen yet: the word every later kernel of the call tests first
__global__ __launch_bounds__(kWave) void unique_reset_kernel(uint32_t* __restrict__ bad)
{
    if (threadIdx.x == 0) {
        *bad = kUniqNoBad;
    }
}

__global__ __launch_bounds__(kUniqSmallThreads) void unique_validate_kernel(const uint64_t* __restrict__ off, uint64_t nseg, uint64_t n,
                                                                             uint32_t* __restrict__ bad)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kUniqSmallThreads;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kUniqSmallThreads + threadIdx.x; s < nseg; s += stride) {
        const uint64_t a = off[s], b = off[s + 1];
        if (b < a || b > n) {
            atomicMin(bad, static_cast<uint32_t>(s));
        }
    }
}

__global__ __launch_bounds__(kUniqSmallThreads) void unique_iota_kernel(uint32_t* __restrict__ out, uint64_t count)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kUniqSmallThreads;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kUniqSmallThreads + threadIdx.x; i < count; i += stride) {
        out[i] = static_cast<uint32_t>(i);
    }
}

// LDS of the tile kernels: one bit per key for the segment starts, one word per thread, the scans' wave totals, where the next tile's walk begins
struct UniqShared {
    uint32_t segbits[kUniqTileKeys / 32];
    uint32_t tinfo[kUniqThreads];
    uint32_t wtot[kUniqThreads / kWave];
    uint32_t next_s0;
};

// The heads of one tile.  In: s0 = first s with off[s] >= tile_start.  Out: the thread's 16 keys, its head bits and segment-start bits
// (bit j = key 16 * tid + j of the tile), and the next tile's s0.  Two barriers; sh.segbits / sh.next_s0 are rewritten by the next call,
// which the caller separates from this one's readers by a barrier of its own.
template <typename Key>
__device__ __forceinline__ void uniq_tile_heads(const Key* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ off, uint64_t nseg, uint64_t lo,
                                                uint64_t hi, uint64_t tile_start, uint64_t s0, UniqShared& sh, Key (&k)[kUniqKpt], uint32_t& hbits,
                                                uint32_t& sbits, uint64_t& s0_next)
{
    constexpr int VEC = KeyVec<Key>::N;
    constexpr int NV = kUniqKpt / VEC;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint64_t first = tile_start + static_cast<uint64_t>(tid) * kUniqKpt;
    if (tid < kUniqTileKeys / 32) {
        sh.segbits[tid] = 0;
    }
    if (tid == 0) {
        sh.next_s0 = static_cast<uint32_t>(nseg + 1);
    }
    const bool live = tile_start < hi && tile_start + kUniqTileKeys > lo;      // (uniform) tiles outside [off[0], off[S]) read no keys
    if (live && tile_start + kUniqTileKeys <= n) {
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const KeyVec<Key> v = load_keys16(keys + first + q * VEC);
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                k[q * VEC + c] = v.k[c];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kUniqKpt; ++j) {
            k[j] = live && first + j < n ? keys[first + j] : Key{0};
        }
    }
    Key left = Key{0};
    if (lane == 0 && live && first > 0 && first <= n) {
        left = keys[first - 1];
    }
    __syncthreads();
    const uint64_t tile_end = tile_start + kUniqTileKeys;
    for (uint64_t s = s0 + tid; s <= nseg; s += kUniqThreads) {
        const uint64_t o = uniq_off(off, s, n);
        if (o >= tile_end) {
            atomicMin(&sh.next_s0, static_cast<uint32_t>(s));
            break;
        }
        if (s < nseg && uniq_off(off, s + 1, n) > o) {          // a non-empty segment starts here
            const uint32_t x = static_cast<uint32_t>(o - tile_start);
            atomicOr(&sh.segbits[x >> 5], 1u << (x & 31u));
        }
    }
    __syncthreads();
    s0_next = sh.next_s0;
    sbits = (sh.segbits[tid >> 1] >> ((tid & 1u) * 16u)) & 0xFFFFu;
    const Key up = __shfl_up(k[kUniqKpt - 1], 1);
    if (lane != 0) {
        left = up;
    }
    hbits = 0;
#pragma unroll
    for (int j = 0; j < kUniqKpt; ++j) {
        const uint64_t i = first + j;
        const bool in = i >= lo && i < hi;
        const bool head = in && (((sbits >> j) & 1u) != 0 || k[j] != (j ? k[j > 0 ? j - 1 : 0] : left));
        hbits |= head ? 1u << j : 0u;
    }
}

// Exclusive running maximum over the workgroup of one value per thread (0 = nothing yet).  Two barriers.
template <int THREADS>
__device__ __forceinline__ uint32_t block_exclusive_max_scan(uint32_t v, uint32_t* wmax)
{
    constexpr int WAVES = THREADS / kWave;
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        x = lane >= static_cast<uint32_t>(d) && y > x ? y : x;
    }
    if (lane == kWave - 1) {
        wmax[wave] = x;
    }
    uint32_t before = __shfl_up(x, 1);
    before = lane == 0 ? 0u : before;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t t = wmax[w];
        before = static_cast<uint32_t>(w) < wave && t > before ? t : before;
    }
    __syncthreads();
    return before;
}

// Workgroup b counts the tiles [b * chunk, (b + 1) * chunk) of a table of `ntab` = tiles + 1 entries padded with zeros to `npad` (a multiple
// of 16: the scan kernels see 16 rows).  The extra tile is empty; it exists so that off[s] == n has a tile when n is a multiple of 4096 and
// so that the scanned table ends with the total.
template <typename Key>
__global__ __launch_bounds__(kUniqThreads) void unique_count_kernel(const Key* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ off,
                                                                    uint64_t nseg, const uint32_t* __restrict__ bad, uint32_t* __restrict__ table,
                                                                    uint32_t ntab, uint32_t npad, uint32_t chunk, uint64_t* __restrict__ uoff)
{
    __shared__ UniqShared sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, npad);
    if (*bad != kUniqNoBad) {
        for (uint32_t t = t0 + tid; t < t1; t += kUniqThreads) {
            table[t] = 0;
        }
        return;
    }
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    uint64_t s0 = t0 < ntab ? uniq_lower_bound(off, nseg, n, static_cast<uint64_t>(t0) << kUniqTileShift) : nseg + 1;
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        if (t >= ntab) {
            if (tid == 0) {
                table[t] = 0;
            }
            continue;
        }
        const uint64_t tile_start = static_cast<uint64_t>(t) << kUniqTileShift;
        Key k[kUniqKpt];
        uint32_t hbits, sbits;
        uint64_t s0_next;
        uniq_tile_heads(keys, n, off, nseg, lo, hi, tile_start, s0, sh, k, hbits, sbits, s0_next);
        uint32_t total;
        const uint32_t before = block_exclusive_scan<kUniqThreads, false>(static_cast<uint32_t>(__popc(hbits)), sh.wtot, total);
        sh.tinfo[tid] = (before << 16) | hbits;
        if (tid == 0) {
            table[t] = total;
        }
        __syncthreads();
        // every off[s] inside the tile (empty segments and off[S] too): the heads of the tile before it
        for (uint64_t s = s0 + tid; s <= nseg; s += kUniqThreads) {
            const uint64_t o = uniq_off(off, s, n);
            if (o >= tile_start + kUniqTileKeys) break;
            const uint32_t x = static_cast<uint32_t>(o - tile_start);
            const uint32_t ti = sh.tinfo[x >> 4];
            uoff[s] = (ti >> 16) + static_cast<uint32_t>(__popc(ti & ((1u << (x & 15u)) - 1u)));
        }
        s0 = s0_next;
        __syncthreads();
    }
}

// run_offsets[s] = heads before off[s]: the scanned table entry of its tile + the tile-local count unique_count_kernel left.  With bad
// offsets every entry is 0 (non-decreasing, total 0).  REPORT (consecutive mode, whose chain has no seg_scan_kernel): the first bad
// segment + 1 goes to the mapped host word unless an earlier report is still pending there.
__global__ __launch_bounds__(kUniqSmallThreads) void unique_offsets_kernel(const uint64_t* __restrict__ off, uint64_t nseg, uint64_t n,
                                                                            const uint32_t* __restrict__ bad, const uint32_t* __restrict__ table,
                                                                            uint64_t* __restrict__ uoff, uint32_t* status_host, int report)
{
    const uint32_t b = *bad;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kUniqSmallThreads;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kUniqSmallThreads + threadIdx.x; s <= nseg; s += stride) {
        uoff[s] = b != kUniqNoBad ? 0ull : table[uniq_off(off, s, n) >> kUniqTileShift] + uoff[s];
    }
    if (report && b != kUniqNoBad && blockIdx.x == 0 && threadIdx.x == 0 &&
        __hip_atomic_load(status_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
        __hip_atomic_store(status_host, b + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// POS: first positions or the inverse map are wanted (the segment of every element must be known); PERM: perm[i] is the original position
// of sorted element i (sorted mode), else the position is i itself.  NULL outputs are skipped.  A position read from perm is used as an
// index only when it is below n (after bad offsets the sort's scratch is undefined; such a call does not get this far, the test stays).
template <typename Key, bool POS, bool PERM>
__global__ __launch_bounds__(kUniqThreads) void unique_write_kernel(const Key* __restrict__ keys, const uint32_t* __restrict__ perm, uint64_t n,
                                                                    const uint64_t* __restrict__ off, uint64_t nseg, const uint32_t* __restrict__ bad,
                                                                    const uint32_t* __restrict__ table, uint32_t ntiles, uint32_t chunk,
                                                                    const uint64_t* __restrict__ uoff, Key* __restrict__ kout,
                                                                    uint32_t* __restrict__ first_out, uint32_t* __restrict__ inverse,
                                                                    uint32_t* __restrict__ hp)
{
    __shared__ UniqShared sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    uint64_t s0 = uniq_lower_bound(off, nseg, n, static_cast<uint64_t>(t0) << kUniqTileShift);
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint64_t tile_start = static_cast<uint64_t>(t) << kUniqTileShift;
        const uint64_t first = tile_start + static_cast<uint64_t>(tid) * kUniqKpt;
        const uint32_t tbase = table[t];
        // the segment that is running when the tile begins: s0 - 1 (off[s0 - 1] < tile_start <= off[s0])
        uint32_t carry_start = 0, carry_g = 0;
        if (POS && s0 > 0) {
            carry_start = static_cast<uint32_t>(uniq_off(off, s0 - 1, n));
            carry_g = static_cast<uint32_t>(uoff[s0 - 1]);
        }
        uint32_t p[kUniqKpt];
        if constexpr (PERM) {
            if (tile_start + kUniqTileKeys <= n) {
#pragma unroll
                for (int q = 0; q < kUniqKpt / 4; ++q) {
                    const U32x4 v = *reinterpret_cast<const U32x4*>(perm + first + q * 4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        p[q * 4 + c] = v.v[c];
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < kUniqKpt; ++j) {
                    p[j] = first + j < n ? perm[first + j] : 0u;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                p[j] = static_cast<uint32_t>(first + j);
            }
        }
        Key k[kUniqKpt];
        uint32_t hbits, sbits;
        uint64_t s0_next;
        uniq_tile_heads(keys, n, off, nseg, lo, hi, tile_start, s0, sh, k, hbits, sbits, s0_next);
        uint32_t total;
        const uint32_t before = block_exclusive_scan<kUniqThreads>(static_cast<uint32_t>(__popc(hbits)), sh.wtot, total);
        const uint32_t base = tbase + before;             // run id of the thread's first head
        uint32_t carry = 0;
        if constexpr (POS) {
            // (tile-local position + 1) << 16 | tile-local run id of the thread's last segment start: both grow with the position, so the
            // running maximum over the threads before is the last segment start before this thread
            uint32_t v = 0;
            if (sbits) {
                const uint32_t q = 31u - static_cast<uint32_t>(__clz(static_cast<int>(sbits)));
                v = ((tid * kUniqKpt + q + 1u) << 16) | (before + static_cast<uint32_t>(__popc(hbits & ((2u << q) - 1u))) - 1u);
            }
            carry = block_exclusive_max_scan<kUniqThreads>(v, sh.wtot);
        }
#pragma unroll
        for (int j = 0; j < kUniqKpt; ++j) {
            const uint64_t i = first + j;
            if (i < lo || i >= hi) continue;
            const uint32_t g = base + static_cast<uint32_t>(__popc(hbits & ((2u << j) - 1u))) - 1u;
            const bool head = ((hbits >> j) & 1u) != 0;
            if (head) {
                kout[g] = k[j];
                if (hp) {
                    hp[g] = static_cast<uint32_t>(i);
                }
            }
            if constexpr (POS) {
                const uint32_t sb = sbits & ((2u << j) - 1u);
                uint32_t seg_start, seg_g;
                if (sb) {
                    const uint32_t q = 31u - static_cast<uint32_t>(__clz(static_cast<int>(sb)));
                    seg_start = static_cast<uint32_t>(first) + q;
                    seg_g = base + static_cast<uint32_t>(__popc(hbits & ((2u << q) - 1u))) - 1u;
                } else if (carry) {
                    seg_start = static_cast<uint32_t>(tile_start) + (carry >> 16) - 1u;
                    seg_g = tbase + (carry & 0xFFFFu);
                } else {
                    seg_start = carry_start;
                    seg_g = carry_g;
                }
                if (head && first_out) {
                    first_out[g] = p[j] - seg_start;
                }
                if (inverse && p[j] < n) {
                    inverse[p[j]] = g - seg_g;
                }
            }
        }
        s0 = s0_next;
        __syncthreads();
    }
}

// The total is the last entry of the scanned table (0 after bad offsets: the count kernel zeroed it).
__global__ __launch_bounds__(kUniqSmallThreads) void unique_counts_kernel(const uint32_t* __restrict__ hp, const uint32_t* __restrict__ table,
                                                                           uint32_t ntiles, const uint64_t* __restrict__ off, uint64_t nseg, uint64_t n,
                                                                           uint32_t* __restrict__ counts)
{
    const uint32_t total = table[ntiles];
    const uint32_t end = static_cast<uint32_t>(uniq_off(off, nseg, n));
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kUniqSmallThreads;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kUniqSmallThreads + threadIdx.x; g < total; g += stride) {
        counts[g] = (g + 1 < total ? hp[g + 1] : end) - hp[g];
    }
}

}  // namespace rsx
