// rsx_topk.hpp — kernels of rsx_segmented_topk: the first min(k, L) entries of the stable sort of every segment, by radix select.
// Included by rsx_capi.hip (host side: capi_topk.inc).  Reuses the segmented sort's classify chain, tile grid and table scan.
//
//   seg_classify_kernel / seg_scan_kernel     (rsx_segmented.hpp; the writing classify records every large segment's id)
//   topk_init_kernel          one-key segments -> their single output slot; every large segment's select state -> (prefix 0, k)
//   topk_sort_kernel<FINAL=false>   segments of 2..4096 keys: one workgroup each sorts (key, position) in LDS and stores ranks < k
//   topk_hist_kernel          one select round: per group of tiles, 256-bin counts of the keys whose higher digits equal the prefix
//   topk_pick_kernel          one select round: per large segment, sums the group partials and picks the digit that holds the k-th key
//   topk_count_kernel         per tile: keys better than / equal to / worse than the segment's threshold -> [segment][digit][tile] table
//   (scan_blocks_kernel + paste_scan_kernel, unchanged: a flat exclusive scan of that table)
//   topk_compact_kernel       per tile: the better keys and the first ties, in index order, to k candidate slots of the segment
//   topk_sort_kernel<FINAL=true>    per large segment: the stable LDS sort of its k candidates (their positions as payload)
//
// Digits of the select rounds are 8 bits of the ENCODED key (KeyCodec), most significant first: 4 rounds for 32-bit keys, 8 for
// 64-bit.  All state lives on the device and the host enqueues a fixed chain; rounds are separated by kernel boundaries.  The
// round's histogram does not funnel counts through global atomics: each workgroup counts a group of consecutive tiles in LDS and
// writes one 256-word partial per segment it touches (START row of the segment that begins in the group, CONT row of the group for
// the segment that was already running); the pick kernel adds a segment's START row and the CONT rows of the groups it covers.
#pragma once

#include "rsx_segmented.hpp"

namespace rsx {

constexpr uint32_t kTopkMaxK = kSegTileKeys;       // k <= one LDS tile
constexpr int kTopkDigitBits = 8;
constexpr int kTopkBins = 1 << kTopkDigitBits;
constexpr int kTopkThreads = kSegChainThreads, kTopkKpt = kSegChainKpt;    // one tile = 256 x 16 keys, the chain's grid
constexpr int kTopkPickThreads = 1024;
constexpr int kTopkInitThreads = 256;

struct TopkState {
    uint64_t prefix;     // encoded digits chosen so far (lower digits zero); after the last round: the k-th key of the segment, encoded
    uint32_t krem;       // keys still to take among those whose higher digits equal the prefix (the rest of k is strictly better)
    uint32_t pad;
};

// Large segment j and tile t's place in it: the segmented chain's seg_tile plus the segment index.
struct TopkTile {
    uint64_t start, a;
    uint32_t len, entry, stride, j;
};

__device__ __forceinline__ uint32_t topk_segment_of(uint32_t t, const uint32_t* __restrict__ tstart, uint32_t nlarge)
{
    uint32_t lo = 0, hi = nlarge;                  // tstart[lo] <= t < tstart[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tstart[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ TopkTile topk_tile(uint32_t t, uint32_t j, const SegLarge* __restrict__ large, const uint32_t* __restrict__ tstart)
{
    const uint32_t ts = tstart[j], te = tstart[j + 1];
    const SegLarge sg = large[j];
    const uint32_t ti = t - ts;
    const uint64_t g = (sg.a >> kSegTileShift) + ti;
    const uint64_t g0 = g << kSegTileShift, g1 = (g + 1) << kSegTileShift;
    const uint64_t start = sg.a > g0 ? sg.a : g0;
    const uint64_t end = sg.b < g1 ? sg.b : g1;
    TopkTile r;
    r.start = start;
    r.a = sg.a;
    r.len = static_cast<uint32_t>(end - start);
    r.entry = kRadix * ts + ti;
    r.stride = te - ts;
    r.j = j;
    return r;
}

// One-key segments go straight to their output slot (position 0); every large segment starts its select with an empty prefix.
template <typename Key>
__global__ __launch_bounds__(kTopkInitThreads) void topk_init_kernel(const uint64_t* __restrict__ off, uint64_t nseg, uint64_t n,
                                                                     const Key* __restrict__ in, Key* __restrict__ kout,
                                                                     uint32_t* __restrict__ iout, uint32_t k, const SegHeader* __restrict__ hdr,
                                                                     TopkState* __restrict__ state)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kTopkInitThreads;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kTopkInitThreads + threadIdx.x; s < nseg; s += stride) {
        const uint64_t a = off[s], b = off[s + 1];
        if (b >= a && b <= n && b - a == 1) {
            kout[s * k] = in[a];
            iout[s * k] = 0u;
        }
    }
    const uint32_t nlarge = hdr->nlarge;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kTopkInitThreads + threadIdx.x; j < nlarge; j += stride) {
        state[j] = TopkState{0ull, k, 0u};
    }
}

// FINAL = false: segments of 2..THREADS*KPT keys of small class `cls`, one per workgroup at a time (grid stride over the class's list),
// payload = position in the segment.  FINAL = true: the k candidates of every large segment (keys at cand + j*k in index order, their
// positions at cidx + j*k).  Both: load (encode), every 4-bit pass inside LDS (seg_rank), store ranks < min(k, len) to out[s*k + rank].
// Pads (past the end) are the encoded all-ones key: last in every pass, never stored.
template <typename Key, int THREADS, int KPT, bool FINAL>
__global__ __launch_bounds__(THREADS) void topk_sort_kernel(const Key* __restrict__ in, const uint32_t* __restrict__ cidx, Key* __restrict__ kout,
                                                            uint32_t* __restrict__ iout, const uint64_t* __restrict__ off,
                                                            const uint32_t* __restrict__ list, const SegHeader* __restrict__ hdr,
                                                            const SegLarge* __restrict__ large, int cls, int passes, uint32_t k,
                                                            KeyCodec<Key> codec)
{
    using L = SegSortLayout<Key, THREADS, KPT>;
    constexpr int KD = L::KD;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* xbuf = smem;
    uint32_t* cnt = smem + L::XBUF_DW;
    uint32_t* wtot = cnt + L::CNT_DW;
    uint32_t* dstart = wtot + 16;
    const uint32_t tid = threadIdx.x;
    const uint32_t count = FINAL ? hdr->nlarge : hdr->count[cls];
    const uint32_t base = FINAL ? 0u : hdr->base[cls];
    const Key pad_key = codec_decode(static_cast<Key>(~Key{0}), codec.ea, codec.em);

#pragma unroll 1
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        uint64_t s, a;
        uint32_t len;
        const Key* src;
        if constexpr (FINAL) {
            s = large[item].pad;
            a = static_cast<uint64_t>(item) * k;
            len = k;
            src = in + a;
        } else {
            s = list[base + item];
            a = off[s];
            const uint64_t len64 = off[s + 1] - a;
            len = len64 < static_cast<uint64_t>(L::TILE) ? static_cast<uint32_t>(len64) : static_cast<uint32_t>(L::TILE);
            src = in + a;
        }
        const uint32_t m = len < k ? len : k;
        const uint64_t dst = s * k;
        Key kk[KPT];
        uint32_t pl[KPT];
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t li = tid * KPT + i;
            kk[i] = codec_encode(li < len ? src[li] : pad_key, codec.ea, codec.em);
            if constexpr (FINAL) {
                pl[i] = li < len ? cidx[a + li] : 0u;
            } else {
                pl[i] = li;
            }
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
            } else {
#pragma unroll
                for (int r = 0; r < KPT; ++r) {
                    const uint32_t i = static_cast<uint32_t>(r) * THREADS + tid;
                    if (i < m) {
                        kout[dst + i] = codec_decode(*reinterpret_cast<const Key*>(xbuf + seg_image_dw(i, KD)), codec.da, codec.dm);
                    }
                }
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
            } else {
#pragma unroll
                for (int r = 0; r < KPT; ++r) {
                    const uint32_t i = static_cast<uint32_t>(r) * THREADS + tid;
                    if (i < m) {
                        iout[dst + i] = xbuf[seg_image_dw(i, 1)];
                    }
                }
            }
            __syncthreads();               // the image and the counters are free for the next round / segment
        }
    }
}

// One select round over the tiles of the large segments, in groups of `gtiles` consecutive tiles (one workgroup per group, grid
// stride): counts, per segment, the digit at `shift` of the encoded keys whose digits above it equal the segment's prefix (round 0:
// every key).  Counts gather in LDS (one 256-bin histogram per wave) and leave once per (group, segment): to start_part[j] for the
// segment j that begins inside the group, to cont_part[g] for the segment that was already running when group g began.
template <typename Key>
__global__ __launch_bounds__(kTopkThreads) void topk_hist_kernel(const Key* __restrict__ keys, const SegHeader* __restrict__ hdr,
                                                                 const SegLarge* __restrict__ large, const uint32_t* __restrict__ tstart,
                                                                 const TopkState* __restrict__ state, uint32_t* __restrict__ start_part,
                                                                 uint32_t* __restrict__ cont_part, uint32_t gtiles, int round,
                                                                 KeyCodec<Key> codec)
{
    constexpr int THREADS = kTopkThreads, KPT = kTopkKpt;
    constexpr int VEC = KeyVec<Key>::N;
    constexpr int NV = KPT / VEC;
    constexpr int WAVES = THREADS / kWave;
    constexpr int BITS = static_cast<int>(sizeof(Key)) * 8;
    __shared__ uint32_t hist[WAVES * kTopkBins];
    const uint32_t tid = threadIdx.x;
    const uint32_t ntiles = hdr->tiles, nlarge = hdr->nlarge;
    const uint32_t ngroups = (ntiles + gtiles - 1) / gtiles;
    const int shift = BITS - kTopkDigitBits * (round + 1);
    const int hshift = shift + kTopkDigitBits;          // < BITS from round 1 on
    uint32_t* mine = hist + (tid / kWave) * kTopkBins;

    for (uint32_t i = tid; i < WAVES * kTopkBins; i += THREADS) {
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
            uint32_t* dst = tstart[jj] < t0 ? cont_part + static_cast<uint64_t>(g) * kTopkBins : start_part + static_cast<uint64_t>(jj) * kTopkBins;
            for (uint32_t d = tid; d < kTopkBins; d += THREADS) {
                uint32_t c = 0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) {
                    c += hist[w * kTopkBins + d];
                    hist[w * kTopkBins + d] = 0;
                }
                dst[d] = c;
            }
            __syncthreads();
        };
        Key want = static_cast<Key>(state[j].prefix);
#pragma unroll 1
        for (uint32_t t = t0; t < t1; ++t) {
            if (tstart[j + 1] <= t) {
                flush(j);
                ++j;
                want = static_cast<Key>(state[j].prefix);
            }
            const TopkTile tl = topk_tile(t, j, large, tstart);
            auto count = [&](Key key) {
                const Key e = codec_encode(key, codec.ea, codec.em);
                if (round == 0 || (e >> hshift) == (want >> hshift)) {
                    atomicAdd(&mine[static_cast<uint32_t>(e >> shift) & (kTopkBins - 1)], 1u);
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

// One select round, per large segment (one workgroup, grid stride): the segment's counts = its START row + the CONT rows of the
// groups after the one it begins in, up to the one holding its last tile; then the digit d whose running count crosses krem is
// appended to the prefix and the keys before it (strictly better) leave krem.
template <typename Key>
__global__ __launch_bounds__(kTopkPickThreads) void topk_pick_kernel(const SegHeader* __restrict__ hdr, const uint32_t* __restrict__ tstart,
                                                                     TopkState* __restrict__ state, const uint32_t* __restrict__ start_part,
                                                                     const uint32_t* __restrict__ cont_part, uint32_t gtiles, int round)
{
    constexpr int SLICES = kTopkPickThreads / kWave;       // each wave sums a slice of the rows, 4 bins per lane
    constexpr int BITS = static_cast<int>(sizeof(Key)) * 8;
    __shared__ __attribute__((aligned(16))) uint32_t part[SLICES * kTopkBins];
    __shared__ uint32_t wtot[kTopkPickThreads / kWave];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (kWave - 1), slice = tid / kWave;
    const uint32_t nlarge = hdr->nlarge;
    const int shift = BITS - kTopkDigitBits * (round + 1);

#pragma unroll 1
    for (uint32_t j = blockIdx.x; j < nlarge; j += gridDim.x) {
        const TopkState st = state[j];
        const uint32_t gs = tstart[j] / gtiles, ge = (tstart[j + 1] - 1) / gtiles;
        U32x4 sum{{0u, 0u, 0u, 0u}};
        if (slice == 0) {
            sum = *reinterpret_cast<const U32x4*>(start_part + static_cast<uint64_t>(j) * kTopkBins + lane * 4);
        }
#pragma unroll 8
        for (uint32_t g = gs + 1 + slice; g <= ge; g += SLICES) {
            const U32x4 x = *reinterpret_cast<const U32x4*>(cont_part + static_cast<uint64_t>(g) * kTopkBins + lane * 4);
            sum.v[0] += x.v[0];
            sum.v[1] += x.v[1];
            sum.v[2] += x.v[2];
            sum.v[3] += x.v[3];
        }
        *reinterpret_cast<U32x4*>(part + slice * kTopkBins + lane * 4) = sum;
        __syncthreads();                           // (also: every thread has read state[j] before it may change)
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
            state[j] = TopkState{st.prefix | (static_cast<uint64_t>(tid) << shift), st.krem - before, 0u};
        }
        __syncthreads();                           // part is free for the next segment
    }
}

// Per tile of the large segments: how many keys are better than the segment's threshold (digit 0), equal to it (digit 1) and worse
// (digit 2) -> table[16 * tstart[j] + digit * tiles(j) + tile of j], digits 3..15 zero.  Thread t holds keys 16t .. 16t+15 of the tile.
template <typename Key>
__device__ __forceinline__ void topk_load_tile(const Key* __restrict__ keys, const TopkTile& tl, Key (&k)[kTopkKpt])
{
    constexpr int VEC = KeyVec<Key>::N;
    constexpr int NV = kTopkKpt / VEC;
    const uint32_t tid = threadIdx.x;
    if (tl.len == kSegTileKeys) {
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const KeyVec<Key> v = load_keys16(keys + tl.start + tid * kTopkKpt + q * VEC);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                k[q * VEC + e] = v.k[e];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < kTopkKpt; ++i) {
            const uint32_t li = tid * kTopkKpt + i;
            k[i] = li < tl.len ? keys[tl.start + li] : Key{0};
        }
    }
}

template <typename Key>
__global__ __launch_bounds__(kTopkThreads) void topk_count_kernel(const Key* __restrict__ keys, uint32_t* __restrict__ table,
                                                                  const SegHeader* __restrict__ hdr, const SegLarge* __restrict__ large,
                                                                  const uint32_t* __restrict__ tstart, const TopkState* __restrict__ state,
                                                                  KeyCodec<Key> codec)
{
    __shared__ uint32_t wtot[kTopkThreads / kWave];
    const uint32_t tid = threadIdx.x;
    const uint32_t ntiles = hdr->tiles, nlarge = hdr->nlarge;

#pragma unroll 1
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const TopkTile tl = topk_tile(t, topk_segment_of(t, tstart, nlarge), large, tstart);
        const Key thr = static_cast<Key>(state[tl.j].prefix);
        Key k[kTopkKpt];
        topk_load_tile(keys, tl, k);
        uint32_t packed = 0;                       // better | equal << 16
#pragma unroll
        for (int i = 0; i < kTopkKpt; ++i) {
            const Key e = codec_encode(k[i], codec.ea, codec.em);
            const bool in = tid * kTopkKpt + i < tl.len;
            packed += in && e < thr ? 1u : 0u;
            packed += in && e == thr ? 0x10000u : 0u;
        }
        uint32_t total;
        (void)block_exclusive_scan<kTopkThreads>(packed, wtot, total);
        if (tid < kRadix) {
            const uint32_t better = total & 0xFFFFu, equal = total >> 16;
            const uint32_t v = tid == 0 ? better : tid == 1 ? equal : tid == 2 ? tl.len - better - equal : 0u;
            table[tl.entry + tid * tl.stride] = v;
        }
    }
}

// Per tile: the better keys and the ties among the first k of the segment go, with their positions, to the segment's k candidate
// slots in index order.  The table is the flat exclusive scan of topk_count_kernel's counts, so entry (j, 0, tile) and (j, 1, tile)
// minus the keys of the large segments before j are the slots of the tile's first better key and first tie.  Tiles that hold
// neither leave without reading their keys.
template <typename Key>
__global__ __launch_bounds__(kTopkThreads) void topk_compact_kernel(const Key* __restrict__ keys, const uint32_t* __restrict__ table,
                                                                    const SegHeader* __restrict__ hdr, const SegLarge* __restrict__ large,
                                                                    const uint32_t* __restrict__ tstart, const TopkState* __restrict__ state,
                                                                    uint32_t k, Key* __restrict__ cand, uint32_t* __restrict__ cidx,
                                                                    KeyCodec<Key> codec)
{
    __shared__ uint32_t wtot[kTopkThreads / kWave];
    const uint32_t tid = threadIdx.x;
    const uint32_t ntiles = hdr->tiles, nlarge = hdr->nlarge;

#pragma unroll 1
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const TopkTile tl = topk_tile(t, topk_segment_of(t, tstart, nlarge), large, tstart);
        const SegLarge sg = large[tl.j];
        const uint64_t before = sg.a - sg.dest;                       // keys of the large segments before j
        const uint32_t e0 = tl.entry, e1 = tl.entry + tl.stride;
        const uint32_t b0 = static_cast<uint32_t>(table[e0] - before), b1 = static_cast<uint32_t>(table[e1] - before);
        const uint32_t nb = table[e0 + 1] - table[e0], ne = table[e1 + 1] - table[e1];
        if (nb == 0 && (ne == 0 || b1 >= k)) continue;      // workgroup-uniform: nothing of this tile is kept
        const Key thr = static_cast<Key>(state[tl.j].prefix);
        Key kk[kTopkKpt];
        topk_load_tile(keys, tl, kk);
        uint32_t packed = 0;
#pragma unroll
        for (int i = 0; i < kTopkKpt; ++i) {
            const Key e = codec_encode(kk[i], codec.ea, codec.em);
            const bool in = tid * kTopkKpt + i < tl.len;
            packed += in && e < thr ? 1u : 0u;
            packed += in && e == thr ? 0x10000u : 0u;
        }
        uint32_t total;
        uint32_t run = block_exclusive_scan<kTopkThreads>(packed, wtot, total);
        uint32_t pb = b0 + (run & 0xFFFFu), pe = b1 + (run >> 16);
        Key* ck = cand + static_cast<uint64_t>(tl.j) * k;
        uint32_t* ci = cidx + static_cast<uint64_t>(tl.j) * k;
        const uint32_t pos0 = static_cast<uint32_t>(tl.start - tl.a) + tid * kTopkKpt;
#pragma unroll
        for (int i = 0; i < kTopkKpt; ++i) {
            const Key e = codec_encode(kk[i], codec.ea, codec.em);
            const bool in = tid * kTopkKpt + i < tl.len;
            if (in && e < thr) {
                ck[pb] = kk[i];
                ci[pb] = pos0 + i;
                ++pb;
            } else if (in && e == thr) {
                if (pe < k) {
                    ck[pe] = kk[i];
                    ci[pe] = pos0 + i;
                }
                ++pe;
            }
        }
    }
}

}  // namespace rsx
