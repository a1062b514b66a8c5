// rsx_compact.hpp — kernels of rsx_segmented_compact: stream compaction (copy_if / DeviceSelect::Flagged / DevicePartition; torch's
// masked_select, x[mask], nonzero) of every segment [off[s], off[s+1]) by a byte mask or by one key bound per segment.  Included by
// rsx_capi.hip (host side: capi_compact.inc).
//
//   (unique_reset_kernel + unique_validate_kernel, unchanged: the first bad segment, one word; every later kernel leaves at once)
//   compact_count_kernel   per 4096-element tile of the global grid: kept elements -> flat [tile] table; for every off[s] inside the tile the
//                          kept elements of the tile before it -> koff[s] (tile-local for now): unique_count_kernel's walk
//   (scan_blocks_kernel + paste_scan_kernel, unchanged: the flat exclusive scan of that table)
//   (unique_offsets_kernel, unchanged: koff[s] += table[tile of off[s]]: final; zeros and the report to the status word on bad offsets)
//   compact_write_kernel   per tile: recomputes the predicate, ranks the kept elements (popcount of the thread's 16 keep bits, a wave
//                          scan, wave totals through LDS), STAGES the survivors in LDS at their rank and stores the staged copy to
//                          consecutive addresses.  Not launched when neither keys nor index are wanted.
//
// PREDICATE.  Mask form: element i is kept iff mask[i] != 0; a thread's 16 mask bytes are one 16-byte load where the mask pointer is
// 16-byte aligned and the tile is whole, guarded byte loads otherwise; the count kernel reads no key.  Bound form: key k of segment s is
// kept iff enc(k) <= enc(bounds[s]) (RSX_COMPACT_STRICT: <), enc = codec_encode with the engine's (A, M): one instantiation per key
// width.  RSX_COMPACT_INVERT flips either.  Elements outside [off[0], off[S]) are neither kept nor rejected: they do not exist.
//
// THE SEGMENT OF AN ELEMENT.  The bound form needs the segment's NUMBER (to load bounds[s]), the index output and the partition need its
// start; unique_write_kernel's start bits and running maximum give a start position but no number.  So: per tile, two bisections that
// gallop on from where the last tile's ended give the segments of the tile's first and last live element (uniform; scalar loads); a
// thread bisects between those two for its first live element — zero steps when the tile lies inside one segment — and again, from its
// current segment on, only when an element passes the end of that segment.  No LDS bitmap, no atomics, and no second walk of the offsets.
//
// DESTINATIONS.  With K(i) the kept elements in [off[0], i): K(i) = table[tile] + rank inside the tile.  Compact mode: kept element i
// goes to K(i).  Partition mode, element i of segment s: kept -> off[s] + (K(i) - koff[s]); rejected -> off[s] + (koff[s+1] - koff[s]) +
// (i - off[s]) - (K(i) - koff[s]).  No atomic decides a destination.
//
// STAGING.  Slot r of the staged copy lives at element r + (r >> 4) (compact_slot).  An LDS store is served in halves of 32 lanes over 32
// banks of 4 bytes; thread t's survivors start at rank ~ 16 t x keep rate, so without the skew the 32 lanes that store their j-th element
// together sit 16 words apart at keep rate 1: two banks, a 16-way conflict.  With it they sit 17 words apart: 32 banks, none (8-byte keys:
// 34 words, every second bank, two words each).  The copy-out reads slots tid, tid + 256, ...: consecutive elements but for one skipped per
// 16, one 2-way conflict per half wave.  Compact mode stages the kept elements at [0, total); partition mode, in a tile inside one segment,
// also the rejected ones behind them at [total, live), and both regions leave as two runs of consecutive addresses.  A partition tile
// that spans segments stores per element from registers (its destinations are no two runs).  LDS: 4352 keys + 4352 index words = 34 KiB
// (4-byte keys, 4 workgroups a CU) or 51 KiB (8-byte keys, 3 workgroups a CU) of the CU's 160 KiB.
#pragma once

#include "rsx_search.hpp"

namespace rsx {

constexpr uint32_t kCompactPartition = 8u, kCompactInvert = 16u, kCompactStrict = 32u;          // RSX_COMPACT_*
constexpr uint32_t kCompactSlots = kUniqTileKeys + kUniqTileKeys / 16;

__device__ __forceinline__ uint32_t compact_slot(uint32_t r) { return r + (r >> 4); }

// first s in [from, nseg] with off[s] > x, nseg + 1 if there is none; every s < from has off[s] <= x (the caller's).  Gallops from `from`.
__device__ __forceinline__ uint64_t compact_seg_upper(const uint64_t* __restrict__ off, uint64_t from, uint64_t nseg, uint64_t n, uint64_t x)
{
    uint64_t lo = from, hi = from, step = 1;
    while (hi <= nseg && uniq_off(off, hi, n) <= x) {
        lo = hi + 1;
        hi += step;
        step <<= 1;
    }
    hi = min(hi, nseg + 1);
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (uniq_off(off, mid, n) <= x) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// What is uniform over a tile: its live range [a, e) = the tile cut to [off[0], off[S]) and the segments of a and of e - 1.
struct CompactTile {
    uint32_t a, e;
    uint32_t s_first, s_last;
};

// false: the tile has no live element.  `from` carries the gallop's start from tile to tile (0 before the workgroup's first).
__device__ __forceinline__ bool compact_tile_range(const uint64_t* __restrict__ off, uint64_t nseg, uint64_t n, uint64_t lo, uint64_t hi,
                                                   uint64_t tile_start, uint64_t& from, CompactTile& tl)
{
    const uint64_t a = max(tile_start, lo), e = min(tile_start + kUniqTileKeys, hi);
    if (a >= e) return false;
    const uint64_t s_first = compact_seg_upper(off, from, nseg, n, a) - 1;             // (off[0] <= a: at least 1 comes back)
    const uint64_t s_last = compact_seg_upper(off, s_first + 1, nseg, n, e - 1) - 1;
    from = s_last + 1;
    tl.a = static_cast<uint32_t>(a);
    tl.e = static_cast<uint32_t>(e);
    tl.s_first = static_cast<uint32_t>(s_first);
    tl.s_last = static_cast<uint32_t>(s_last);
    return true;
}

// The segment a thread is in: its number and [start, end).
struct CompactCursor {
    uint32_t s, start, end;
};

// the segment of live element i among [s_lo, s_last] (off[s_lo] <= i is the caller's); empty segments are skipped
__device__ __forceinline__ void compact_seek(CompactCursor& c, const uint64_t* __restrict__ off, uint64_t n, uint32_t s_lo, uint32_t s_last, uint32_t i)
{
    c.s = off ? static_cast<uint32_t>(search_segment_of(off, s_lo, s_last, i)) : 0u;
    c.start = static_cast<uint32_t>(uniq_off(off, c.s, n));
    c.end = static_cast<uint32_t>(uniq_off(off, static_cast<uint64_t>(c.s) + 1, n));
}

template <typename Key>
__device__ __forceinline__ void compact_load_keys(const Key* __restrict__ keys, uint64_t n, uint64_t tile_start, Key (&k)[kUniqKpt])
{
    constexpr int VEC = KeyVec<Key>::N;
    const uint64_t first = tile_start + static_cast<uint64_t>(threadIdx.x) * kUniqKpt;
    if (tile_start + kUniqTileKeys <= n) {
#pragma unroll
        for (int q = 0; q < kUniqKpt / VEC; ++q) {
            const KeyVec<Key> v = load_keys16(keys + first + q * VEC);
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                k[q * VEC + c] = v.k[c];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kUniqKpt; ++j) {
            k[j] = first + j < n ? keys[first + j] : Key{0};
        }
    }
}

// bit j = element 16 tid + j of the tile is live (in [a, e))
__device__ __forceinline__ uint32_t compact_live_bits(uint64_t tile_start, const CompactTile& tl)
{
    const int64_t first = static_cast<int64_t>(tile_start) + static_cast<int64_t>(threadIdx.x) * kUniqKpt;
    const int64_t b0 = min(max(static_cast<int64_t>(tl.a) - first, int64_t{0}), int64_t{kUniqKpt});
    const int64_t b1 = min(max(static_cast<int64_t>(tl.e) - first, int64_t{0}), int64_t{kUniqKpt});
    return ((1u << b1) - 1u) & ~((1u << b0) - 1u);
}

// The keep bits of the thread's 16 elements (bit j = element 16 tid + j of the tile), live elements only.
template <typename Key, bool BOUND>
__device__ __forceinline__ uint32_t compact_keep_bits(const Key (&k)[kUniqKpt], const uint8_t* __restrict__ mask, const Key* __restrict__ bounds,
                                                      const uint64_t* __restrict__ off, uint64_t n, uint64_t tile_start, const CompactTile& tl,
                                                      uint32_t live, uint32_t flags, Key ca, Key cm)
{
    const uint64_t first = tile_start + static_cast<uint64_t>(threadIdx.x) * kUniqKpt;
    uint32_t bits = 0;
    if constexpr (BOUND) {
        if (live) {
            const bool strict = (flags & kCompactStrict) != 0;
            CompactCursor c;
            compact_seek(c, off, n, tl.s_first, tl.s_last, static_cast<uint32_t>(first) + static_cast<uint32_t>(__ffs(static_cast<int>(live)) - 1));
            Key b = codec_encode(bounds[c.s], ca, cm);
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                const uint32_t i = static_cast<uint32_t>(first) + j;
                if (((live >> j) & 1u) != 0 && i >= c.end) {
                    compact_seek(c, off, n, c.s + 1u, tl.s_last, i);
                    b = codec_encode(bounds[c.s], ca, cm);
                }
                const Key x = codec_encode(k[j], ca, cm);
                bits |= (strict ? x < b : x <= b) ? 1u << j : 0u;
            }
        }
    } else {
        const uint8_t* mp = mask + first;
        if ((reinterpret_cast<uintptr_t>(mask) & 15u) == 0 && tile_start + kUniqTileKeys <= n) {
            const U32x4 v = *reinterpret_cast<const U32x4*>(mp);
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                bits |= ((v.v[j >> 2] >> ((j & 3) * 8)) & 0xFFu) != 0 ? 1u << j : 0u;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                bits |= (first + j < n && mp[j] != 0) ? 1u << j : 0u;
            }
        }
    }
    bits = (flags & kCompactInvert) != 0 ? ~bits : bits;
    return bits & live;
}

// LDS of the count kernel: one word per thread for the walk of the offsets, the scan's wave totals
struct CompactCountShared {
    uint32_t tinfo[kUniqThreads];
    uint32_t wtot[kUniqThreads / kWave];
};

// Workgroup b counts the tiles [b * chunk, (b + 1) * chunk) of a table of `ntab` = tiles + 1 entries padded with zeros to `npad`
// (unique_count_kernel's table: the extra tile is empty and gives off[s] == n a tile when n is a multiple of 4096).
template <typename Key, bool BOUND>
__global__ __launch_bounds__(kUniqThreads) void compact_count_kernel(const Key* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ off,
                                                                     uint64_t nseg, const uint8_t* __restrict__ mask, const Key* __restrict__ bounds,
                                                                     uint32_t flags, Key ca, Key cm, const uint32_t* __restrict__ bad,
                                                                     uint32_t* __restrict__ table, uint32_t ntab, uint32_t npad, uint32_t chunk,
                                                                     uint64_t* __restrict__ koff)
{
    __shared__ CompactCountShared sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, npad);
    if (*bad != kUniqNoBad) {
        for (uint32_t t = t0 + tid; t < t1; t += kUniqThreads) {
            table[t] = 0;
        }
        return;
    }
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    uint64_t from = 0, wfrom = 0;
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        if (t >= ntab) {
            if (tid == 0) {
                table[t] = 0;
            }
            continue;
        }
        const uint64_t tile_start = static_cast<uint64_t>(t) << kUniqTileShift;
        CompactTile tl;
        uint32_t kbits = 0;
        if (compact_tile_range(off, nseg, n, lo, hi, tile_start, from, tl)) {       // (uniform)
            Key k[kUniqKpt];
            if constexpr (BOUND) {
                compact_load_keys(keys, n, tile_start, k);
            }
            kbits = compact_keep_bits<Key, BOUND>(k, mask, bounds, off, n, tile_start, tl, compact_live_bits(tile_start, tl), flags, ca, cm);
        }
        uint32_t total;
        const uint32_t before = block_exclusive_scan<kUniqThreads, false>(static_cast<uint32_t>(__popc(kbits)), sh.wtot, total);
        sh.tinfo[tid] = (before << 16) | kbits;
        if (tid == 0) {
            table[t] = total;
        }
        __syncthreads();
        // every off[s] inside the tile (empty segments and off[S] too): the kept elements of the tile before it
        wfrom = tile_start ? compact_seg_upper(off, wfrom, nseg, n, tile_start - 1) : 0ull;
        for (uint64_t s = wfrom + tid; s <= nseg; s += kUniqThreads) {
            const uint64_t o = uniq_off(off, s, n);
            if (o >= tile_start + kUniqTileKeys) break;
            const uint32_t x = static_cast<uint32_t>(o - tile_start);
            const uint32_t ti = sh.tinfo[x >> 4];
            koff[s] = (ti >> 16) + static_cast<uint32_t>(__popc(ti & ((1u << (x & 15u)) - 1u)));
        }
        __syncthreads();
    }
}

template <typename Key>
struct CompactWriteShared {
    Key skey[kCompactSlots];
    uint32_t sidx[kCompactSlots];
    uint32_t wtot[kUniqThreads / kWave];
};

// PART: partition mode.  kout / iout: NULL to skip (not both: the host does not launch then).  koff is final (unique_offsets_kernel).
template <typename Key, bool BOUND, bool PART>
__global__ __launch_bounds__(kUniqThreads) void compact_write_kernel(const Key* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ off,
                                                                     uint64_t nseg, const uint8_t* __restrict__ mask, const Key* __restrict__ bounds,
                                                                     uint32_t flags, Key ca, Key cm, const uint32_t* __restrict__ bad,
                                                                     const uint32_t* __restrict__ table, uint32_t ntiles, uint32_t chunk,
                                                                     const uint64_t* __restrict__ koff, Key* __restrict__ kout,
                                                                     uint32_t* __restrict__ iout)
{
    __shared__ CompactWriteShared<Key> sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    uint64_t from = 0;
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint64_t tile_start = static_cast<uint64_t>(t) << kUniqTileShift;
        CompactTile tl;
        if (!compact_tile_range(off, nseg, n, lo, hi, tile_start, from, tl)) continue;        // (uniform)
        const uint32_t first = static_cast<uint32_t>(tile_start) + tid * kUniqKpt;
        const uint32_t tbase = table[t];
        Key k[kUniqKpt];
        if (BOUND || kout) {                                      // (uniform) the index of a mask needs no key
            compact_load_keys(keys, n, tile_start, k);
        }
        const uint32_t live = compact_live_bits(tile_start, tl);
        const uint32_t kbits = compact_keep_bits<Key, BOUND>(k, mask, bounds, off, n, tile_start, tl, live, flags, ca, cm);
        uint32_t total;
        const uint32_t before = block_exclusive_scan<kUniqThreads>(static_cast<uint32_t>(__popc(kbits)), sh.wtot, total);
        const bool single = tl.s_first == tl.s_last;              // (uniform)
        if (!PART || single) {
            const uint32_t head = tl.a - static_cast<uint32_t>(tile_start);        // dead elements at the front of the tile
            CompactCursor c{0, 0, 0};
            if (iout && live) {
                compact_seek(c, off, n, tl.s_first, tl.s_last, first + static_cast<uint32_t>(__ffs(static_cast<int>(live)) - 1));
            }
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                const uint32_t i = first + j;
                const bool in = ((live >> j) & 1u) != 0, kept = ((kbits >> j) & 1u) != 0;
                const uint32_t rank = before + static_cast<uint32_t>(__popc(kbits & ((1u << j) - 1u)));
                if (iout && in && i >= c.end) {
                    compact_seek(c, off, n, c.s + 1u, tl.s_last, i);
                }
                if (kept || (PART && in)) {
                    const uint32_t slot = compact_slot(kept ? rank : total + (tid * kUniqKpt + j - head - rank));
                    sh.skey[slot] = k[j];
                    if (iout) {
                        sh.sidx[slot] = i - c.start;
                    }
                }
            }
            __syncthreads();
            uint32_t count = total;
            uint64_t dk = tbase, dr = 0;
            if constexpr (PART) {
                const uint64_t start = uniq_off(off, tl.s_first, n);
                const uint64_t k0 = koff[tl.s_first], kept_s = koff[static_cast<uint64_t>(tl.s_first) + 1] - k0;
                count = tl.e - tl.a;
                dk = start + (tbase - k0);
                dr = start + kept_s + (tl.a - start) - (tbase - k0);
            }
            for (uint32_t r = tid; r < count; r += kUniqThreads) {
                const uint64_t d = r < total ? dk + r : dr + (r - total);
                const uint32_t slot = compact_slot(r);
                if (kout) {
                    kout[d] = sh.skey[slot];
                }
                if (iout) {
                    iout[d] = sh.sidx[slot];
                }
            }
            __syncthreads();                                      // the next tile stages again
        } else {
            // a partition tile that spans segments: every element finds its own segment's start and counts
            if (live) {
                CompactCursor c;
                compact_seek(c, off, n, tl.s_first, tl.s_last, first + static_cast<uint32_t>(__ffs(static_cast<int>(live)) - 1));
                uint32_t k0 = static_cast<uint32_t>(koff[c.s]), kept_s = static_cast<uint32_t>(koff[static_cast<uint64_t>(c.s) + 1]) - k0;
#pragma unroll
                for (int j = 0; j < kUniqKpt; ++j) {
                    const uint32_t i = first + j;
                    if (((live >> j) & 1u) == 0) continue;
                    if (i >= c.end) {
                        compact_seek(c, off, n, c.s + 1u, tl.s_last, i);
                        k0 = static_cast<uint32_t>(koff[c.s]);
                        kept_s = static_cast<uint32_t>(koff[static_cast<uint64_t>(c.s) + 1]) - k0;
                    }
                    const uint32_t kb = tbase + before + static_cast<uint32_t>(__popc(kbits & ((1u << j) - 1u))) - k0;     // kept before i in its segment
                    const uint32_t rel = i - c.start;
                    const uint64_t d = static_cast<uint64_t>(c.start) + (((kbits >> j) & 1u) != 0 ? kb : kept_s + rel - kb);
                    if (kout) {
                        kout[d] = k[j];
                    }
                    if (iout) {
                        iout[d] = rel;
                    }
                }
            }
        }
    }
}

}  // namespace rsx
