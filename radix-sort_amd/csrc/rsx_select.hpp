// rsx_select.hpp — kernels of rsx_segmented_select: for up to 8 ranks per segment, the entry at that rank of the segment's stable sort
// (key and position), by radix select.  Included by rsx_capi.hip (host side: capi_select.inc).  Reuses the segmented sort's classify
// chain, the top-k's tile grid (topk_tile, topk_load_tile, TopkState) and the unchanged table scan.
//
//   seg_classify_kernel / seg_scan_kernel     (rsx_segmented.hpp; the writing classify records every large segment's id)
//   select_init_kernel        one-key segments -> the slots whose rank is 0; every (large segment, q) -> (prefix 0, krem = rank + 1), or
//                             inactive (krem 0) when the rank is not below the segment's length
//   select_sort_kernel        segments of 2..4096 keys: one workgroup each sorts (key, position) in LDS and stores the image slots its ranks name
//   select_hist_kernel<RC>    one select round, ONE pass over the keys for all ranks: per group of tiles and per q, 256-bin counts of the
//                             keys whose higher digits equal prefix q (round 0: one histogram, every prefix is empty)
//   select_pick_kernel        one select round: per (large segment, q), sums the group partials and picks the digit where the count crosses krem
//   select_count_kernel<RC>   per tile: keys equal to threshold q -> digit row q of the [segment][digit][tile] table (other rows zero)
//   (scan_blocks_kernel + paste_scan_kernel, unchanged: a flat exclusive scan of that table)
//   select_locate_kernel      per tile: for every q whose krem-th tie lies in this tile (table entries only; other tiles leave without
//                             reading keys), finds that key and stores it and its position
//
// State, partial counts and outputs are laid out [segment][q] with the call's R = ranks_per_segment; RC in {1, 2, 4, 8} is the
// compiled capacity (register arrays, LDS histograms) and q >= R is inactive.  After the last round state[j*R+q].prefix is the encoded
// key at the rank and krem says which of its ties, in index order, is the wanted one.
#pragma once

#include "rsx_topk.hpp"

namespace rsx {

constexpr uint32_t kSelectMaxRanks = 8;      // 8 x 4 per-wave 256-bin histograms = 32 KiB of LDS; 8 tie rows of the 16 digit rows per segment

template <typename Key>
__global__ __launch_bounds__(kTopkInitThreads) void select_init_kernel(const uint64_t* __restrict__ off, uint64_t nseg, uint64_t n,
                                                                       const Key* __restrict__ in, const uint32_t* __restrict__ ranks, uint32_t R,
                                                                       Key* __restrict__ kout, uint32_t* __restrict__ iout,
                                                                       const SegHeader* __restrict__ hdr, const SegLarge* __restrict__ large,
                                                                       TopkState* __restrict__ state)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kTopkInitThreads;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kTopkInitThreads + threadIdx.x; s < nseg; s += stride) {
        const uint64_t a = off[s], b = off[s + 1];
        if (b >= a && b <= n && b - a == 1) {
            for (uint32_t q = 0; q < R; ++q) {
                if (ranks[s * R + q] == 0u) {
                    kout[s * R + q] = in[a];
                    iout[s * R + q] = 0u;
                }
            }
        }
    }
    const uint64_t items = static_cast<uint64_t>(hdr->nlarge) * R;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTopkInitThreads + threadIdx.x; i < items; i += stride) {
        const SegLarge sg = large[i / R];
        const uint32_t r = ranks[sg.pad * R + i % R];
        state[i] = TopkState{0ull, r < sg.b - sg.a ? r + 1u : 0u, 0u};
    }
}

// Segments of 2..THREADS*KPT keys of small class `cls`, one per workgroup at a time (grid stride over the class's list): topk_sort_kernel's
// LDS sort of (key, position); after the last pass thread q < R takes image slot ranks[s*R + q] if it is below the segment's length.
template <typename Key, int THREADS, int KPT>
__global__ __launch_bounds__(THREADS) void select_sort_kernel(const Key* __restrict__ in, const uint32_t* __restrict__ ranks, uint32_t R,
                                                              Key* __restrict__ kout, uint32_t* __restrict__ iout, const uint64_t* __restrict__ off,
                                                              const uint32_t* __restrict__ list, const SegHeader* __restrict__ hdr, int cls,
                                                              int passes, KeyCodec<Key> codec)
{
    using L = SegSortLayout<Key, THREADS, KPT>;
    constexpr int KD = L::KD;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* xbuf = smem;
    uint32_t* cnt = smem + L::XBUF_DW;
    uint32_t* wtot = cnt + L::CNT_DW;
    uint32_t* dstart = wtot + 16;
    const uint32_t tid = threadIdx.x;
    const uint32_t count = hdr->count[cls];
    const uint32_t base = hdr->base[cls];
    const Key pad_key = codec_decode(static_cast<Key>(~Key{0}), codec.ea, codec.em);

#pragma unroll 1
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint64_t s = list[base + item];
        const uint64_t a = off[s];
        const uint64_t len64 = off[s + 1] - a;
        const uint32_t len = len64 < static_cast<uint64_t>(L::TILE) ? static_cast<uint32_t>(len64) : static_cast<uint32_t>(L::TILE);
        const Key* src = in + a;
        const uint32_t want = tid < R ? ranks[s * R + tid] : 0xFFFFFFFFu;
        const bool take = want < len;
        Key kk[KPT];
        uint32_t pl[KPT];
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t li = tid * KPT + i;
            kk[i] = codec_encode(li < len ? src[li] : pad_key, codec.ea, codec.em);
            pl[i] = li;
        }
#pragma unroll 1
        for (int pass = 0; pass < passes; ++pass) {
            const bool last = pass + 1 == passes;
            uint32_t slot[KPT], dg[KPT];
            seg_rank<Key, THREADS, KPT>(kk, pass * kRadixBits, slot, dg, cnt, wtot, dstart);
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                *reinterpret_cast<Key*>(xbuf + seg_image_dw(slot[i], KD)) = kk[i];
            }
            __syncthreads();
            if (!last) {
#pragma unroll
                for (int i = 0; i < KPT; ++i) {
                    kk[i] = *reinterpret_cast<const Key*>(xbuf + seg_image_dw(tid * KPT + i, KD));
                }
            } else if (take) {
                kout[s * R + tid] = codec_decode(*reinterpret_cast<const Key*>(xbuf + seg_image_dw(want, KD)), codec.da, codec.dm);
            }
            __syncthreads();               // every thread has taken its keys: the image carries the payload now
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                xbuf[seg_image_dw(slot[i], 1)] = pl[i];
            }
            __syncthreads();
            if (!last) {
#pragma unroll
                for (int i = 0; i < KPT; ++i) {
                    pl[i] = xbuf[seg_image_dw(tid * KPT + i, 1)];
                }
            } else if (take) {
                iout[s * R + tid] = xbuf[seg_image_dw(want, 1)];
            }
            __syncthreads();               // the image and the counters are free for the next round / segment
        }
    }
}

// One select round over the tiles of the large segments, in groups of `gtiles` consecutive tiles (one workgroup per group, grid
// stride), as topk_hist_kernel, but every key is compared with the prefixes of all R ranks of its segment and counted into the
// histogram of each one it matches: hist[q][wave][bin].  Round 0 has one empty prefix, so it counts into q = 0 alone and writes
// row q = 0 alone (select_pick_kernel reads that row for every q).  Partials: start_part[(j*R + q)*256 ..] for the segment j that
// begins inside the group, cont_part[(g*R + q)*256 ..] for the segment that was already running when group g began.
template <typename Key, int RC>
__global__ __launch_bounds__(kTopkThreads) void select_hist_kernel(const Key* __restrict__ keys, const SegHeader* __restrict__ hdr,
                                                                   const SegLarge* __restrict__ large, const uint32_t* __restrict__ tstart,
                                                                   const TopkState* __restrict__ state, uint32_t* __restrict__ start_part,
                                                                   uint32_t* __restrict__ cont_part, uint32_t gtiles, int round, uint32_t R,
                                                                   KeyCodec<Key> codec)
{
    constexpr int THREADS = kTopkThreads, KPT = kTopkKpt;
    constexpr int VEC = KeyVec<Key>::N;
    constexpr int NV = KPT / VEC;
    constexpr int WAVES = THREADS / kWave;
    constexpr int BITS = static_cast<int>(sizeof(Key)) * 8;
    constexpr uint32_t QSTRIDE = WAVES * kTopkBins;
    __shared__ uint32_t hist[RC * QSTRIDE];
    const uint32_t tid = threadIdx.x;
    const uint32_t ntiles = hdr->tiles, nlarge = hdr->nlarge;
    const uint32_t ngroups = (ntiles + gtiles - 1) / gtiles;
    const int shift = BITS - kTopkDigitBits * (round + 1);
    const int hshift = shift + kTopkDigitBits;          // < BITS from round 1 on
    const uint32_t rows = round == 0 ? 1u : R;          // histograms in use this round
    uint32_t* mine = hist + (tid / kWave) * kTopkBins;

    for (uint32_t i = tid; i < RC * QSTRIDE; i += THREADS) {
        hist[i] = 0;
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint32_t t0 = g * gtiles;
        const uint32_t t1 = t0 + gtiles < ntiles ? t0 + gtiles : ntiles;
        uint32_t j = topk_segment_of(t0, tstart, nlarge);
        // flushes segment j's counts (wave-uniform call); the histograms are zero again afterwards
        auto flush = [&](uint32_t jj) {
            __syncthreads();
            uint32_t* dst = tstart[jj] < t0 ? cont_part + static_cast<uint64_t>(g) * R * kTopkBins : start_part + static_cast<uint64_t>(jj) * R * kTopkBins;
            for (uint32_t x = tid; x < rows * kTopkBins; x += THREADS) {
                const uint32_t q = x / kTopkBins, d = x % kTopkBins;
                uint32_t c = 0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) {
                    c += hist[q * QSTRIDE + w * kTopkBins + d];
                    hist[q * QSTRIDE + w * kTopkBins + d] = 0;
                }
                dst[x] = c;
            }
            __syncthreads();
        };
        Key want[RC];                  // prefix q shifted down to its chosen digits; inactive q: a value no key can match
        bool act[RC];
        auto load_state = [&](uint32_t jj) {
#pragma unroll
            for (int q = 0; q < RC; ++q) {
                act[q] = false;
                want[q] = 0;
                if (static_cast<uint32_t>(q) < R) {
                    const TopkState st = state[static_cast<uint64_t>(jj) * R + q];
                    act[q] = st.krem != 0u;
                    want[q] = round == 0 ? Key{0} : static_cast<Key>(static_cast<Key>(st.prefix) >> hshift);
                }
            }
        };
        load_state(j);
#pragma unroll 1
        for (uint32_t t = t0; t < t1; ++t) {
            if (tstart[j + 1] <= t) {
                flush(j);
                ++j;
                load_state(j);
            }
            const TopkTile tl = topk_tile(t, j, large, tstart);
            auto count = [&](Key key) {
                const Key e = codec_encode(key, codec.ea, codec.em);
                const uint32_t d = static_cast<uint32_t>(e >> shift) & (kTopkBins - 1);
                if (round == 0) {
                    atomicAdd(&mine[d], 1u);
                } else {
                    const Key h = static_cast<Key>(e >> hshift);
#pragma unroll
                    for (int q = 0; q < RC; ++q) {
                        if (act[q] && h == want[q]) {
                            atomicAdd(&mine[q * QSTRIDE + d], 1u);
                        }
                    }
                }
            };
            if (tl.len == kSegTileKeys) {            // a whole tile of the global grid: 16-byte aligned
                KeyVec<Key> v[NV];
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    v[q] = load_keys16(keys + tl.start + static_cast<uint32_t>(q) * THREADS * VEC + tid * VEC);
                }
#pragma unroll
                for (int q = 0; q < NV; ++q) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        count(v[q].k[e]);
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < KPT; ++r) {
                    const uint32_t li = static_cast<uint32_t>(r) * THREADS + tid;
                    if (li < tl.len) {
                        count(keys[tl.start + li]);
                    }
                }
            }
        }
        flush(j);
    }
}

// One select round, per (large segment j, q) (one workgroup, grid stride): topk_pick_kernel on the partial rows of (j, q) — row q = 0
// in round 0, where all ranks share the one histogram.  Inactive states are left alone.
template <typename Key>
__global__ __launch_bounds__(kTopkPickThreads) void select_pick_kernel(const SegHeader* __restrict__ hdr, const uint32_t* __restrict__ tstart,
                                                                       TopkState* __restrict__ state, const uint32_t* __restrict__ start_part,
                                                                       const uint32_t* __restrict__ cont_part, uint32_t gtiles, int round, uint32_t R)
{
    constexpr int SLICES = kTopkPickThreads / kWave;       // each wave sums a slice of the rows, 4 bins per lane
    constexpr int BITS = static_cast<int>(sizeof(Key)) * 8;
    __shared__ __attribute__((aligned(16))) uint32_t part[SLICES * kTopkBins];
    __shared__ uint32_t wtot[kTopkPickThreads / kWave];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (kWave - 1), slice = tid / kWave;
    const uint64_t items = static_cast<uint64_t>(hdr->nlarge) * R;
    const int shift = BITS - kTopkDigitBits * (round + 1);

#pragma unroll 1
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const TopkState st = state[item];
        if (st.krem == 0u) continue;               // workgroup-uniform
        const uint32_t j = static_cast<uint32_t>(item / R);
        const uint32_t row = round == 0 ? 0u : static_cast<uint32_t>(item % R);
        const uint32_t gs = tstart[j] / gtiles, ge = (tstart[j + 1] - 1) / gtiles;
        U32x4 sum{{0u, 0u, 0u, 0u}};
        if (slice == 0) {
            sum = *reinterpret_cast<const U32x4*>(start_part + (static_cast<uint64_t>(j) * R + row) * kTopkBins + lane * 4);
        }
#pragma unroll 8
        for (uint32_t g = gs + 1 + slice; g <= ge; g += SLICES) {
            const U32x4 x = *reinterpret_cast<const U32x4*>(cont_part + (static_cast<uint64_t>(g) * R + row) * kTopkBins + lane * 4);
            sum.v[0] += x.v[0];
            sum.v[1] += x.v[1];
            sum.v[2] += x.v[2];
            sum.v[3] += x.v[3];
        }
        *reinterpret_cast<U32x4*>(part + slice * kTopkBins + lane * 4) = sum;
        __syncthreads();                           // (also: every thread has read state[item] before it may change)
        uint32_t c = 0;
        if (tid < kTopkBins) {
#pragma unroll
            for (int w = 0; w < SLICES; ++w) {
                c += part[w * kTopkBins + tid];
            }
        }
        uint32_t total;
        const uint32_t before = block_exclusive_scan<kTopkPickThreads>(c, wtot, total);
        if (tid < kTopkBins && before < st.krem && st.krem <= before + c) {       // exactly one digit: the counts add up to >= krem
            state[item] = TopkState{st.prefix | (static_cast<uint64_t>(tid) << shift), st.krem - before, 0u};
        }
        __syncthreads();                           // part is free for the next item
    }
}

// Per tile of the large segments: how many keys equal threshold q -> table[16 * tstart[j] + q * tiles(j) + tile of j] for q < R
// (0 for an inactive q), rows R..15 zero.  Thread t holds keys 16t .. 16t+15 of the tile; counts travel two to a word.
template <typename Key, int RC>
__global__ __launch_bounds__(kTopkThreads) void select_count_kernel(const Key* __restrict__ keys, uint32_t* __restrict__ table,
                                                                    const SegHeader* __restrict__ hdr, const SegLarge* __restrict__ large,
                                                                    const uint32_t* __restrict__ tstart, const TopkState* __restrict__ state,
                                                                    uint32_t R, KeyCodec<Key> codec)
{
    constexpr int P = (RC + 1) / 2;
    constexpr int WAVES = kTopkThreads / kWave;
    __shared__ uint32_t wsum[WAVES * P];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t ntiles = hdr->tiles, nlarge = hdr->nlarge;

#pragma unroll 1
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const TopkTile tl = topk_tile(t, topk_segment_of(t, tstart, nlarge), large, tstart);
        Key thr[RC];
        bool act[RC];
#pragma unroll
        for (int q = 0; q < RC; ++q) {
            act[q] = false;
            thr[q] = 0;
            if (static_cast<uint32_t>(q) < R) {
                const TopkState st = state[static_cast<uint64_t>(tl.j) * R + q];
                act[q] = st.krem != 0u;
                thr[q] = static_cast<Key>(st.prefix);
            }
        }
        Key k[kTopkKpt];
        topk_load_tile(keys, tl, k);
        uint32_t pk[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            pk[p] = 0;
        }
#pragma unroll
        for (int i = 0; i < kTopkKpt; ++i) {
            const Key e = codec_encode(k[i], codec.ea, codec.em);
            const bool in = tid * kTopkKpt + i < tl.len;
#pragma unroll
            for (int q = 0; q < RC; ++q) {
                pk[q >> 1] += in && act[q] && e == thr[q] ? 1u << (16 * (q & 1)) : 0u;
            }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const uint32_t incl = wave_inclusive_scan(pk[p]);
            if (lane == kWave - 1) {
                wsum[wave * P + p] = incl;
            }
        }
        __syncthreads();
        if (tid < kRadix) {
            uint32_t v = 0;
            if (tid < static_cast<uint32_t>(RC)) {
                uint32_t tot = 0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) {
                    tot += wsum[w * P + (tid >> 1)];
                }
                v = (tid & 1u) ? tot >> 16 : tot & 0xFFFFu;
            }
            table[tl.entry + tid * tl.stride] = v;
        }
        __syncthreads();                           // wsum is free for the next tile
    }
}

// Per tile: the table is the flat exclusive scan of select_count_kernel's counts, so entry (j, q, tile) minus entry (j, q, 0) is the
// number of ties of threshold q in the tiles of j before this one, and the next entry minus this one the ties inside it.  The tile in
// which that running count crosses krem holds the wanted key: the krem-th tie in index order.  A tile that holds none of its
// segment's R wanted keys leaves without reading its keys.
template <typename Key>
__global__ __launch_bounds__(kTopkThreads) void select_locate_kernel(const Key* __restrict__ keys, const uint32_t* __restrict__ table,
                                                                     const SegHeader* __restrict__ hdr, const SegLarge* __restrict__ large,
                                                                     const uint32_t* __restrict__ tstart, const TopkState* __restrict__ state,
                                                                     uint32_t R, Key* __restrict__ kout, uint32_t* __restrict__ iout,
                                                                     KeyCodec<Key> codec)
{
    __shared__ uint32_t wtot[kTopkThreads / kWave];
    const uint32_t tid = threadIdx.x;
    const uint32_t ntiles = hdr->tiles, nlarge = hdr->nlarge;

#pragma unroll 1
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const TopkTile tl = topk_tile(t, topk_segment_of(t, tstart, nlarge), large, tstart);
        const uint32_t ti = t - tstart[tl.j];
        uint32_t hits = 0;                         // bit q: the wanted tie of rank q lies in this tile (workgroup-uniform)
        for (uint32_t q = 0; q < R; ++q) {
            const uint32_t krem = state[static_cast<uint64_t>(tl.j) * R + q].krem;
            const uint32_t e = tl.entry + q * tl.stride;
            const uint32_t here = table[e];
            const uint32_t before = here - table[e - ti], cnt = table[e + 1] - here;
            hits |= (krem != 0u && before < krem && krem <= before + cnt) ? 1u << q : 0u;
        }
        if (hits == 0) continue;
        Key kk[kTopkKpt];
        topk_load_tile(keys, tl, kk);
        const uint64_t s = large[tl.j].pad;
        const uint32_t pos0 = static_cast<uint32_t>(tl.start - tl.a) + tid * kTopkKpt;
        for (uint32_t q = 0; q < R; ++q) {
            if (!((hits >> q) & 1u)) continue;
            const TopkState st = state[static_cast<uint64_t>(tl.j) * R + q];
            const Key thr = static_cast<Key>(st.prefix);
            const uint32_t e = tl.entry + q * tl.stride;
            const uint32_t need = st.krem - (table[e] - table[e - ti]);      // 1-based among this tile's ties
            uint32_t eq = 0;                       // bit i: key i of this thread is a tie
#pragma unroll
            for (int i = 0; i < kTopkKpt; ++i) {
                const bool in = tid * kTopkKpt + i < tl.len;
                eq |= in && codec_encode(kk[i], codec.ea, codec.em) == thr ? 1u << i : 0u;
            }
            const uint32_t c = __popc(eq);
            uint32_t total;
            const uint32_t run = block_exclusive_scan<kTopkThreads>(c, wtot, total);
            if (run < need && need <= run + c) {   // exactly one thread
                uint32_t left = need - run;        // the left-th set bit of eq
#pragma unroll
                for (int i = 0; i < kTopkKpt; ++i) {
                    if ((eq >> i) & 1u) {
                        if (--left == 0) {
                            kout[s * R + q] = kk[i];
                            iout[s * R + q] = pos0 + i;
                        }
                    }
                }
            }
        }
    }
}

}  // namespace rsx
