// rsx_bins.hpp — kernels of rsx_segmented_histogram: S x B counters, counts[s * B + b] = the keys of segment [off[s], off[s+1]) that fall into
// bin b (cub::DeviceHistogram; torch.bincount, histc, histogram, per segment).  Included by rsx_capi.hip (host side: capi_histogram.inc).
// (rsx_histogram.hpp is the SORT's digit histogram: another kernel, untouched.)  The bin of a key: rsx_bin_math.hpp.
//
//   (unique_reset_kernel + unique_validate_kernel, unchanged: the first bad segment, one word)
//   bins_zero_kernel   counts[0 .. S * B) := 0 with 16-byte stores (element stores before the first and after the last 16-byte boundary).  A
//                      kernel and no memset, so that a captured call replays it as written.  Reports a bad segment to the status words.
//   bins_tile_kernel   the family's grid: tiles of 4096 keys, 256 threads x 16 consecutive keys, 16-byte loads; workgroup b walks the tiles
//                      [b * chunk, (b + 1) * chunk).  Leaves at once after bad offsets: every counter stays zero.
//
// A PIECE is what a tile holds of one segment.  Every piece takes one of two paths:
//   DIRECT  B > kBinsLdsMax, or the piece is shorter than kBinsDirectPiece keys: one no-return global atomic add per key that has a bin (a
//           thread adds a run of consecutive keys with one destination as one add).  Vocabulary-sized bins, and many short segments: a flush
//           of B LDS counters per 50-key piece would cost more than the piece.
//   LDS     everything else: the keys are counted with LDS atomic adds into B counters — one copy per wave while B <= kBinsWavePrivateMax,
//           so that a hot bin is contended by 64 lanes and not by 256; one shared copy above — and the workgroup KEEPS counting from tile to
//           tile while the segment stays the same.  The counters are flushed (the non-zero ones, one no-return global atomic add each, and
//           zeroed) when the segment changes and at the workgroup's end: a one-segment call flushes once per workgroup, not once per tile.
// A tile inside one segment is one piece and needs no look at the offsets beyond the tile's two bisections (compact_tile_range).  In a tile
// that spans segments every thread walks its 16 keys with a cursor (compact_seek); an LDS piece is at least kBinsDirectPiece = 256 keys long,
// so at most 16 of them fit a tile and (piece start - tile start) / 256 numbers them: the thread that holds a piece's first key writes its
// segment into that slot, and the workgroup then takes the slots in order, flushing in between.
//
// Edges form: the B + 1 edges are staged in LDS once per workgroup, mapped to the engine's order; a thread bisects 4 keys in lockstep, at
// most 13 probes each.  Counts are integers: the adds commute, and the result is bitwise reproducible in any arrival order.
// LDS: 16 KiB of counters, and 4097 mapped edges (16 / 32 KiB) in the edges form.  No scratch memory.
#pragma once

#include "rsx_bin_math.hpp"
#include "rsx_compact.hpp"

namespace rsx {

constexpr uint32_t kBinsLdsMax = 4096;                // bins the LDS path holds (16 KiB of counters); the edges form's bound too
constexpr uint32_t kBinsWavePrivateMax = 1024;        // ... of which every wave has its own copy up to here (4 x 1024 counters)
constexpr int kBinsDirectShift = 8;
constexpr uint32_t kBinsDirectPiece = 1u << kBinsDirectShift;       // pieces shorter than this take the direct path
constexpr uint32_t kBinsPieceSlots = kUniqTileKeys >> kBinsDirectShift;
constexpr int kBinsZeroThreads = 256;
constexpr int kBinsLockstep = 4;                      // bisections a thread runs together
constexpr uint32_t kBinsNone = 0xFFFFFFFFu;
static_assert(kBinsPieceSlots == 16, "a piece's slot is a 4-bit field");
static_assert(kBinsWavePrivateMax * (kUniqThreads / kWave) == kBinsLdsMax, "the wave-private copies fill the counters exactly");

using rsx_bins::EvenArgs;

__global__ __launch_bounds__(kBinsZeroThreads) void bins_zero_kernel(uint32_t* __restrict__ counts, uint64_t total, const uint32_t* __restrict__ bad,
                                                                     uint32_t* status_host, uint32_t call_id)
{
    const uint64_t head = min(total, static_cast<uint64_t>(((16u - (reinterpret_cast<uintptr_t>(counts) & 15u)) & 15u) >> 2));
    const uint64_t nvec = (total - head) >> 2, body_end = head + (nvec << 2);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBinsZeroThreads, first = static_cast<uint64_t>(blockIdx.x) * kBinsZeroThreads + threadIdx.x;
    U32x4* body = reinterpret_cast<U32x4*>(counts + head);
    for (uint64_t v = first; v < nvec; v += stride) {
        body[v] = U32x4{{0u, 0u, 0u, 0u}};
    }
    if (first < head) {
        counts[first] = 0u;
    } else if (first >= kWave && body_end + (first - kWave) < total) {      // (the tail has fewer than 4 counters)
        counts[body_end + (first - kWave)] = 0u;
    }
    const uint32_t b = *bad;
    if (b != kUniqNoBad && first == 0 && __hip_atomic_load(status_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
        __hip_atomic_store(status_host + 1, call_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(status_host, b + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);        // (after the call's id)
    }
}

template <typename Key, bool EDGES>
struct BinsShared {
    uint32_t cnt[kBinsLdsMax];
    uint32_t piece_seg[kBinsPieceSlots];
};
template <typename Key>
struct BinsShared<Key, true> {
    uint32_t cnt[kBinsLdsMax];
    uint32_t piece_seg[kBinsPieceSlots];
    Key edges[kBinsLdsMax + 1];
};

// The thread's adds, a run of equal destinations as one: add(dest, count) is the LDS or the global atomic.
template <typename Add>
struct BinsRun {
    Add add;
    uint32_t dest = kBinsNone, count = 0;
    __device__ __forceinline__ void put(uint32_t d)
    {
        if (d == dest) {
            ++count;
        } else {
            flush();
            dest = d;
            count = 1;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (count != 0) {
            add(dest, count);
        }
        count = 0;
        dest = kBinsNone;
    }
};

// FORM: rsx_bins::kFormEvenInt / kFormEvenFloat / kFormEdges.  ca, cm: the engine's order constants (edges form).
template <typename Key, int FORM>
__global__ __launch_bounds__(kUniqThreads) void bins_tile_kernel(const Key* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ off, uint64_t nseg,
                                                                 const Key* __restrict__ edges, EvenArgs<Key> ev, Key ca, Key cm, uint32_t nbins,
                                                                 const uint32_t* __restrict__ bad, uint32_t ntiles, uint32_t chunk,
                                                                 uint32_t* __restrict__ counts)
{
    constexpr bool EDGES = FORM == rsx_bins::kFormEdges;
    __shared__ BinsShared<Key, EDGES> sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    const uint32_t B = nbins;
    const bool use_lds = B <= kBinsLdsMax;                                   // (uniform)
    const bool wave_private = B <= kBinsWavePrivateMax;
    const uint32_t copies = wave_private ? kUniqThreads / kWave : 1u;
    uint32_t* mine = sh.cnt + (wave_private ? (tid / kWave) * B : 0u);       // this wave's counters
    if (use_lds) {
        for (uint32_t i = tid; i < B * copies; i += kUniqThreads) {
            sh.cnt[i] = 0u;
        }
    }
    if constexpr (EDGES) {
        for (uint32_t i = tid; i <= B; i += kUniqThreads) {
            sh.edges[i] = codec_encode(edges[i], ca, cm);
        }
    }
    __syncthreads();

    auto lds_add = [&](uint32_t b, uint32_t c) { __hip_atomic_fetch_add(mine + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    auto global_add = [&](uint32_t d, uint32_t c) { __hip_atomic_fetch_add(counts + d, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    // the counted keys of segment s leave for counts[s * B ..]; the counters are zero again afterwards (uniform call)
    auto flush = [&](uint32_t s) {
        __syncthreads();
        uint32_t* row = counts + static_cast<uint64_t>(s) * B;
        for (uint32_t b = tid; b < B; b += kUniqThreads) {
            uint32_t c = 0;
            for (uint32_t w = 0; w < copies; ++w) {
                c += sh.cnt[w * B + b];
                sh.cnt[w * B + b] = 0u;
            }
            if (c != 0) {
                __hip_atomic_fetch_add(row + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
    };

    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    uint64_t from = 0;
    uint32_t acc = kBinsNone;                                                // (uniform) the segment the LDS counters belong to
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint64_t tile_start = static_cast<uint64_t>(t) << kUniqTileShift;
        CompactTile tl;
        if (!compact_tile_range(off, nseg, n, lo, hi, tile_start, from, tl)) continue;        // (uniform)
        Key k[kUniqKpt];
        compact_load_keys(keys, n, tile_start, k);
        const uint32_t live = compact_live_bits(tile_start, tl);
        // the bin of every key, kNoBin for the dead and the dropped
        uint32_t bin[kUniqKpt];
        if constexpr (EDGES) {
#pragma unroll
            for (int g = 0; g < kUniqKpt / kBinsLockstep; ++g) {
                Key q[kBinsLockstep];
                uint32_t base[kBinsLockstep], len[kBinsLockstep];
#pragma unroll
                for (int r = 0; r < kBinsLockstep; ++r) {
                    q[r] = codec_encode(k[g * kBinsLockstep + r], ca, cm);
                    base[r] = 0;
                    len[r] = ((live >> (g * kBinsLockstep + r)) & 1u) != 0 ? B + 1u : 0u;
                }
                rsx_bins::bisect_right<kBinsLockstep>([&](uint32_t i) { return sh.edges[i]; }, q, base, len);
#pragma unroll
                for (int r = 0; r < kBinsLockstep; ++r) {
                    const int j = g * kBinsLockstep + r;
                    bin[j] = ((live >> j) & 1u) != 0 ? rsx_bins::edges_bin_of(base[r], q[r], sh.edges[B], B) : rsx_bins::kNoBin;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                const uint32_t b = FORM == rsx_bins::kFormEvenFloat ? rsx_bins::even_float_bin(k[j], ev, B) : rsx_bins::even_int_bin(k[j], ev, B);
                bin[j] = ((live >> j) & 1u) != 0 ? b : rsx_bins::kNoBin;
            }
        }
        const uint32_t tstart = static_cast<uint32_t>(tile_start), first = tstart + tid * kUniqKpt;
        if (tl.s_first == tl.s_last) {                                        // (uniform) one piece
            if (use_lds && tl.e - tl.a >= kBinsDirectPiece) {
                if (acc != tl.s_first) {
                    if (acc != kBinsNone) {
                        flush(acc);
                    }
                    acc = tl.s_first;
                }
                BinsRun<decltype(lds_add)> run{lds_add};
#pragma unroll
                for (int j = 0; j < kUniqKpt; ++j) {
                    if (bin[j] != rsx_bins::kNoBin) {
                        run.put(bin[j]);
                    }
                }
                run.flush();
            } else {
                const uint32_t row = tl.s_first * B;                          // (S * B <= 2^31)
                BinsRun<decltype(global_add)> run{global_add};
#pragma unroll
                for (int j = 0; j < kUniqKpt; ++j) {
                    if (bin[j] != rsx_bins::kNoBin) {
                        run.put(row + bin[j]);
                    }
                }
                run.flush();
            }
            continue;
        }
        // several pieces: short ones leave at once; the long ones are numbered, then taken in order
        __syncthreads();
        if (tid < kBinsPieceSlots) {
            sh.piece_seg[tid] = kBinsNone;
        }
        __syncthreads();
        uint64_t slots = 0;                                                   // 4 bits per key: the slot of its LDS piece
        uint32_t in_lds = 0;                                                  // bit j: key j belongs to an LDS piece
        if (live) {
            CompactCursor c;
            compact_seek(c, off, n, tl.s_first, tl.s_last, first + static_cast<uint32_t>(__ffs(static_cast<int>(live)) - 1));
            BinsRun<decltype(global_add)> run{global_add};
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                if (((live >> j) & 1u) == 0) continue;
                const uint32_t i = first + j;
                if (i >= c.end) {
                    compact_seek(c, off, n, c.s + 1u, tl.s_last, i);
                }
                const uint32_t pstart = max(c.start, tstart), pend = min(c.end, tstart + kUniqTileKeys);
                if (use_lds && pend - pstart >= kBinsDirectPiece) {
                    const uint32_t slot = (pstart - tstart) >> kBinsDirectShift;
                    if (i == pstart) {
                        sh.piece_seg[slot] = c.s;
                    }
                    slots |= static_cast<uint64_t>(slot) << (4 * j);
                    in_lds |= 1u << j;
                } else if (bin[j] != rsx_bins::kNoBin) {
                    run.put(c.s * B + bin[j]);
                }
            }
            run.flush();
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t slot = 0; slot < kBinsPieceSlots; ++slot) {
            const uint32_t s = sh.piece_seg[slot];
            if (s == kBinsNone) continue;                                     // (uniform)
            if (acc != s) {
                if (acc != kBinsNone) {
                    flush(acc);
                }
                acc = s;
            }
            BinsRun<decltype(lds_add)> run{lds_add};
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                if (((in_lds >> j) & 1u) != 0 && static_cast<uint32_t>(slots >> (4 * j) & 15u) == slot && bin[j] != rsx_bins::kNoBin) {
                    run.put(bin[j]);
                }
            }
            run.flush();
        }
    }
    if (acc != kBinsNone) {
        flush(acc);
    }
}

}  // namespace rsx
