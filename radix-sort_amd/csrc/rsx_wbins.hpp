// rsx_wbins.hpp — kernel of rsx_segmented_weighted_histogram: S x B 64-bit sums, sums[s * B + b] = the sum of the MASSES of the keys of segment
// [off[s], off[s+1]) that fall into bin b (torch.bincount(weights=), torch.histogram(weight=), numpy.histogram(weights=), per segment).
// Included by rsx_capi.hip (host side: capi_whistogram.inc).  The bin of a key: rsx_bin_math.hpp, exactly rsx_segmented_histogram's; the
// mass of a weight: rsx_mass_math.hpp, exactly rsx_segmented_weighted_select's, and its signed form.
//
//   (unique_reset_kernel + unique_validate_kernel, unchanged: the first bad segment, one word)
//   (bins_zero_kernel, unchanged, over 2 * S * B 32-bit words: the sums are zero before the first add; reports a bad segment)
//   wbins_tile_kernel   bins_tile_kernel's walk (rsx_bins.hpp: tiles of 4096 keys, 256 threads x 16 consecutive keys, pieces, the 16 piece
//                       slots, counting carried from tile to tile, a flush at a segment change and at the workgroup's end), with the
//                       thread's 16 weights loaded beside its keys and 64-bit counters.
//
// What differs from bins_tile_kernel:
//   WEIGHTS   16-byte loads where the weight pointer is 16-byte aligned and the tile is whole, guarded element loads otherwise.  A weight
//             becomes a 32-bit mass at once (UINT32: the word; floats: rsx_mass) and, in the signed form, one bit that says "negated": the
//             64-bit addend is formed where it is added, so a thread holds 16 words and 16 bits and not 16 64-bit values.
//   COUNTERS  64-bit: ds_add_u64 in LDS, no-return global_atomic_add_x2 to the result.  Modular 64-bit adds commute: the result is bitwise
//             reproducible in any arrival order, signed or not.
//   RUNS      the fold of a run of consecutive equal destinations (WbinsRun) carries a 64-bit sum and no count.
//   ZERO      a key whose mass is 0 has no bin: it issues no atomic and does not end a run.
//   LDS       the unweighted kernel's 16 KiB of counters, so the same occupancy: kWbinsLdsMax = 2048 bins in LDS, a copy per wave up to
//             kWbinsWavePrivateMax = 512, one shared copy above.  The edges form still takes 4096 bins: its edges are staged in LDS as
//             before (4097 keys), and bin counts above 2048 take the direct path.  No scratch memory.
#pragma once

#include "rsx_bins.hpp"
#include "rsx_mass_math.hpp"
#include "rsx_wselect.hpp"

namespace rsx {

constexpr uint32_t kWbinsLdsMax = 2048;               // bins the LDS path holds (16 KiB of 64-bit counters)
constexpr uint32_t kWbinsWavePrivateMax = 512;        // ... of which every wave has its own copy up to here (4 x 512 counters)
constexpr uint32_t kWbinsEdgesMax = kBinsLdsMax;      // the edges form's bound stays the unweighted call's
static_assert(kWbinsWavePrivateMax * (kUniqThreads / kWave) == kWbinsLdsMax, "the wave-private copies fill the counters exactly");
static_assert(kWbinsLdsMax * sizeof(uint64_t) == kBinsLdsMax * sizeof(uint32_t), "the LDS budget of the counters is the unweighted kernel's");

template <typename Key, bool EDGES>
struct WbinsShared {
    uint64_t sum[kWbinsLdsMax];
    uint32_t piece_seg[kBinsPieceSlots];
};
template <typename Key>
struct WbinsShared<Key, true> {
    uint64_t sum[kWbinsLdsMax];
    uint32_t piece_seg[kBinsPieceSlots];
    Key edges[kWbinsEdgesMax + 1];
};

// The thread's adds, a run of equal destinations as one: add(dest, sum) is the LDS or the global atomic.  A run whose signed masses
// cancel adds nothing.
template <typename Add>
struct WbinsRun {
    Add add;
    uint32_t dest = kBinsNone;
    uint64_t sum = 0;
    __device__ __forceinline__ void put(uint32_t d, uint64_t v)
    {
        if (d == dest) {
            sum += v;
        } else {
            flush();
            dest = d;
            sum = v;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (sum != 0) {
            add(dest, sum);
        }
        sum = 0;
        dest = kBinsNone;
    }
};

// The masses of the thread's 16 weights, and bit j of `neg`: mass j is added negated (signed form; 0 otherwise).
template <int WK>
__device__ __forceinline__ void wbins_load_masses(const void* __restrict__ weights, bool wvec, uint64_t n, uint64_t tile_start, int32_t wexp, bool is_signed,
                                                  uint32_t (&m)[kUniqKpt], uint32_t& neg)
{
    using WT = typename WselWord<WK>::type;
    constexpr int VEC = 16 / static_cast<int>(sizeof(WT));
    const WT* w = static_cast<const WT*>(weights);
    const uint64_t first = tile_start + static_cast<uint64_t>(threadIdx.x) * kUniqKpt;
    WT bits[kUniqKpt];
    if (wvec && tile_start + kUniqTileKeys <= n) {
#pragma unroll
        for (int q = 0; q < kUniqKpt / VEC; ++q) {
            const WselVec<WT, VEC> v = *reinterpret_cast<const WselVec<WT, VEC>*>(w + first + q * VEC);
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                bits[q * VEC + c] = v.w[c];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kUniqKpt; ++j) {
            bits[j] = first + j < n ? w[first + j] : WT{0};
        }
    }
    neg = 0;
#pragma unroll
    for (int j = 0; j < kUniqKpt; ++j) {
        if constexpr (WK == static_cast<int>(rsx_mass::kWeightUint32)) {
            m[j] = bits[j];
        } else {
            if (is_signed) {                                                 // (uniform)
                const rsx_mass::SignedMass sm = rsx_mass::signed_mass_of_bits(bits[j], static_cast<uint32_t>(WK), wexp);
                m[j] = sm.magnitude;
                neg |= sm.negative ? 1u << j : 0u;
            } else {
                m[j] = rsx_mass::mass_of_bits(bits[j], static_cast<uint32_t>(WK), wexp);
            }
        }
    }
}

// FORM: rsx_bins::kFormEvenInt / kFormEvenFloat / kFormEdges.  WK: RSX_WEIGHT_*.  ca, cm: the engine's order constants (edges form).
// wvec: the weights are 16-byte aligned.  is_signed: RSX_WHIST_SIGNED (float kinds).
template <typename Key, int FORM, int WK>
__global__ __launch_bounds__(kUniqThreads) void wbins_tile_kernel(const Key* __restrict__ keys, const void* __restrict__ weights, bool wvec, uint64_t n,
                                                                  const uint64_t* __restrict__ off, uint64_t nseg, const Key* __restrict__ edges,
                                                                  EvenArgs<Key> ev, Key ca, Key cm, uint32_t nbins, int32_t wexp, bool is_signed,
                                                                  const uint32_t* __restrict__ bad, uint32_t ntiles, uint32_t chunk,
                                                                  uint64_t* __restrict__ sums)
{
    constexpr bool EDGES = FORM == rsx_bins::kFormEdges;
    __shared__ WbinsShared<Key, EDGES> sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    const uint32_t B = nbins;
    const bool use_lds = B <= kWbinsLdsMax;                                  // (uniform)
    const bool wave_private = B <= kWbinsWavePrivateMax;
    const uint32_t copies = wave_private ? kUniqThreads / kWave : 1u;
    uint64_t* mine = sh.sum + (wave_private ? (tid / kWave) * B : 0u);       // this wave's counters
    if (use_lds) {
        for (uint32_t i = tid; i < B * copies; i += kUniqThreads) {
            sh.sum[i] = 0ull;
        }
    }
    if constexpr (EDGES) {
        for (uint32_t i = tid; i <= B; i += kUniqThreads) {                  // (B <= kWbinsEdgesMax: the host's check)
            sh.edges[i] = codec_encode(edges[i], ca, cm);
        }
    }
    __syncthreads();

    auto lds_add = [&](uint32_t b, uint64_t v) { __hip_atomic_fetch_add(mine + b, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    auto global_add = [&](uint32_t d, uint64_t v) { __hip_atomic_fetch_add(sums + d, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    // the summed masses of segment s leave for sums[s * B ..]; the counters are zero again afterwards (uniform call)
    auto flush = [&](uint32_t s) {
        __syncthreads();
        uint64_t* row = sums + static_cast<uint64_t>(s) * B;
        for (uint32_t b = tid; b < B; b += kUniqThreads) {
            uint64_t c = 0;
            for (uint32_t w = 0; w < copies; ++w) {
                c += sh.sum[w * B + b];
                sh.sum[w * B + b] = 0ull;
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
        uint32_t mass[kUniqKpt], neg;
        wbins_load_masses<WK>(weights, wvec, n, tile_start, wexp, is_signed, mass, neg);
        const uint32_t live = compact_live_bits(tile_start, tl);
        // the bin of every key, kNoBin for the dead, the dropped and the weightless
        uint32_t bin[kUniqKpt];
        if constexpr (EDGES) {
#pragma unroll
            for (int g = 0; g < kUniqKpt / kBinsLockstep; ++g) {
                Key q[kBinsLockstep];
                uint32_t base[kBinsLockstep], len[kBinsLockstep];
#pragma unroll
                for (int r = 0; r < kBinsLockstep; ++r) {
                    const int j = g * kBinsLockstep + r;
                    q[r] = codec_encode(k[j], ca, cm);
                    base[r] = 0;
                    len[r] = ((live >> j) & 1u) != 0 && mass[j] != 0u ? B + 1u : 0u;
                }
                rsx_bins::bisect_right<kBinsLockstep>([&](uint32_t i) { return sh.edges[i]; }, q, base, len);
#pragma unroll
                for (int r = 0; r < kBinsLockstep; ++r) {
                    const int j = g * kBinsLockstep + r;
                    bin[j] = ((live >> j) & 1u) != 0 && mass[j] != 0u ? rsx_bins::edges_bin_of(base[r], q[r], sh.edges[B], B) : rsx_bins::kNoBin;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                const uint32_t b = FORM == rsx_bins::kFormEvenFloat ? rsx_bins::even_float_bin(k[j], ev, B) : rsx_bins::even_int_bin(k[j], ev, B);
                bin[j] = ((live >> j) & 1u) != 0 && mass[j] != 0u ? b : rsx_bins::kNoBin;
            }
        }
        auto addend = [&](int j) { return rsx_mass::signed_addend(mass[j], ((neg >> j) & 1u) != 0); };
        const uint32_t tstart = static_cast<uint32_t>(tile_start), first = tstart + tid * kUniqKpt;
        if (tl.s_first == tl.s_last) {                                        // (uniform) one piece
            if (use_lds && tl.e - tl.a >= kBinsDirectPiece) {
                if (acc != tl.s_first) {
                    if (acc != kBinsNone) {
                        flush(acc);
                    }
                    acc = tl.s_first;
                }
                WbinsRun<decltype(lds_add)> run{lds_add};
#pragma unroll
                for (int j = 0; j < kUniqKpt; ++j) {
                    if (bin[j] != rsx_bins::kNoBin) {
                        run.put(bin[j], addend(j));
                    }
                }
                run.flush();
            } else {
                const uint32_t row = tl.s_first * B;                          // (S * B <= 2^30)
                WbinsRun<decltype(global_add)> run{global_add};
#pragma unroll
                for (int j = 0; j < kUniqKpt; ++j) {
                    if (bin[j] != rsx_bins::kNoBin) {
                        run.put(row + bin[j], addend(j));
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
            WbinsRun<decltype(global_add)> run{global_add};
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
                    run.put(c.s * B + bin[j], addend(j));
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
            WbinsRun<decltype(lds_add)> run{lds_add};
#pragma unroll
            for (int j = 0; j < kUniqKpt; ++j) {
                if (((in_lds >> j) & 1u) != 0 && static_cast<uint32_t>(slots >> (4 * j) & 15u) == slot && bin[j] != rsx_bins::kNoBin) {
                    run.put(bin[j], addend(j));
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
