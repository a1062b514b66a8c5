// rsx_segmented.hpp — kernels of rsx_segmented_sort: many independent key ranges [off[s], off[s+1]) sorted in one call.
// Included by rsx_capi.hip (host side: capi_segmented.inc).
//
//   seg_classify_kernel<false>   per block of 2048 segments: validity, size class, tiles and keys of the large ones -> block sums
//   seg_scan_kernel              one workgroup: exclusive scan of the block sums, totals -> SegHeader, first bad segment -> mapped host word
//   seg_classify_kernel<true>    per segment: its slot in the small-class list or in the large-segment table; segments of one key are copied
//   seg_small_sort_kernel        segments of at most one tile, one workgroup each, every pass inside LDS (tile_sort_kernel's ranking)
//   seg_histogram_kernel         large segments: per-tile digit counts into the [large segment][digit][tile of segment] table
//   (scan_blocks_kernel + paste_scan_kernel, unchanged: a flat exclusive scan of that table)
//   seg_reorder_kernel           large segments: the stable scatter of one pass, each key back into its own segment's index range
//
// Every launch is sized on the host from n and the segment count alone; the real counts live in SegHeader on the device and the
// workgroups walk them with a grid stride (workgroups with nothing to do leave at once).  Keys are coded with the engine's order map
// (KeyCodec: both directions set in the small sorts; the chain encodes in its first pass and decodes in its last, zero constants
// elsewhere), so one instantiation per key width serves every key kind and direction.
#pragma once

#include "rsx_common.hpp"

namespace rsx {

constexpr int kSegTileShift = 12;
constexpr uint32_t kSegTileKeys = 1u << kSegTileShift;      // tiles of the large-segment chain: the global 4096-key grid, clipped at segment ends
constexpr int kSegClasses = 3;                               // small classes: 2..256, 257..1024, 1025..4096 keys
constexpr uint32_t kSegClass0Max = 256, kSegClass1Max = 1024;
constexpr int kSegClassifyThreads = 256;
constexpr int kSegPerThread = 8;
constexpr int kSegPerBlock = kSegClassifyThreads * kSegPerThread;
constexpr int kSegScanThreads = 256;
constexpr int kSegChainThreads = 256, kSegChainKpt = 16;   // one tile = 256 x 16 keys
// fields of the per-block sums (uint64 each): the three small classes, large segments, their tiles and keys, first bad segment
constexpr int SF_LARGE = 3, SF_TILES = 4, SF_KEYS = 5, SF_BAD = 6, SF_SUMS = 6, SF_STRIDE = 8;

struct SegHeader {
    uint32_t count[kSegClasses];     // segments of each small class
    uint32_t base[kSegClasses];      // where each class starts in the shared list
    uint32_t nlarge;                 // large segments taking the chain (0 when the bounds below were exceeded)
    uint32_t tiles;                  // their tiles
    uint32_t chain_ok;
    uint32_t pad[7];
};

struct SegLarge {
    uint64_t a, b;                   // [a, b)
    uint64_t dest;                   // a - (keys of the large segments before this one), modulo 2^64: slot = dest + scanned table entry + rank in digit
    uint64_t pad;                    // the segment's index for rsx_segmented_topk, else 0
};

__device__ __forceinline__ uint32_t seg_class(uint64_t len)
{
    return len <= kSegClass0Max ? 0u : len <= kSegClass1Max ? 1u : len <= kSegTileKeys ? 2u : 3u;
}

__device__ __forceinline__ uint64_t seg_tiles(uint64_t a, uint64_t b)
{
    return ((b + kSegTileKeys - 1) >> kSegTileShift) - (a >> kSegTileShift);
}

// Exclusive scan over the workgroup of F uint64 values per thread; tot gets the sums.  lds: THREADS/64 * F words.
template <int THREADS, int F>
__device__ __forceinline__ void block_scan_u64(uint64_t (&v)[F], uint64_t (&tot)[F], uint64_t* lds)
{
    constexpr int WAVES = THREADS / kWave;
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint64_t inc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        uint64_t x = v[f];
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint64_t y = __shfl_up(x, d);
            x += lane >= static_cast<uint32_t>(d) ? y : 0ull;
        }
        inc[f] = x;
        if (lane == kWave - 1) {
            lds[wave * F + f] = x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < F; ++f) {
        uint64_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint64_t t = lds[w * F + f];
            before += static_cast<uint32_t>(w) < wave ? t : 0ull;
            all += t;
        }
        v[f] = before + inc[f] - v[f];
        tot[f] = all;
    }
    __syncthreads();
}

// WRITE = false: block sums of the fields into bsum[block][SF_STRIDE] (SF_BAD: the block's first bad segment, ~0 if none).
// WRITE = true: bsum holds the scanned block prefixes (seg_scan_kernel); every segment takes its place: small classes -> list,
// large segments -> large[] / tstart[] (only when the header says the chain's bounds hold), one-key segments are copied.
// IDS = true (rsx_segmented_topk): each large segment's index goes to SegLarge::pad and one-key segments are left to the caller.
template <typename Key, bool WRITE, bool IDS = false>
__global__ __launch_bounds__(kSegClassifyThreads) void seg_classify_kernel(const uint64_t* __restrict__ off, uint64_t nseg, uint64_t n,
                                                                           uint64_t* __restrict__ bsum, const SegHeader* __restrict__ hdr,
                                                                           uint32_t* __restrict__ list, SegLarge* __restrict__ large,
                                                                           uint32_t* __restrict__ tstart, const Key* __restrict__ kin,
                                                                           Key* __restrict__ kout, const uint32_t* __restrict__ pin,
                                                                           uint32_t* __restrict__ pout)
{
    __shared__ uint64_t lds[(kSegClassifyThreads / kWave) * SF_SUMS];
    __shared__ unsigned long long first_bad;
    if (threadIdx.x == 0) {
        first_bad = ~0ull;
    }
    const uint64_t first = static_cast<uint64_t>(blockIdx.x) * kSegPerBlock + static_cast<uint64_t>(threadIdx.x) * kSegPerThread;
    uint64_t f[SF_SUMS] = {0, 0, 0, 0, 0, 0};
    uint64_t bad = ~0ull;
    for (int i = 0; i < kSegPerThread; ++i) {
        const uint64_t s = first + i;
        if (s >= nseg) break;
        const uint64_t a = off[s], b = off[s + 1];
        if (b < a || b > n) {
            bad = bad < s ? bad : s;
            continue;
        }
        const uint64_t len = b - a;
        if (len < 2) continue;
        const uint32_t c = seg_class(len);
        f[c] += 1;
        if (c == SF_LARGE) {
            f[SF_TILES] += seg_tiles(a, b);
            f[SF_KEYS] += len;
        }
    }
    uint64_t tot[SF_SUMS];
    block_scan_u64<kSegClassifyThreads, SF_SUMS>(f, tot, lds);      // (its barriers also order first_bad's initialisation)
    if (bad != ~0ull) {
        atomicMin(&first_bad, static_cast<unsigned long long>(bad));
    }
    if constexpr (!WRITE) {
        __syncthreads();
        if (threadIdx.x < SF_SUMS) {
            bsum[static_cast<uint64_t>(blockIdx.x) * SF_STRIDE + threadIdx.x] = tot[threadIdx.x];
        }
        if (threadIdx.x == SF_BAD) {
            bsum[static_cast<uint64_t>(blockIdx.x) * SF_STRIDE + SF_BAD] = first_bad;
        }
    } else {
        (void)tot;
        const uint64_t* bp = bsum + static_cast<uint64_t>(blockIdx.x) * SF_STRIDE;
#pragma unroll
        for (int k = 0; k < SF_SUMS; ++k) {
            f[k] += bp[k];
        }
        const bool chain = hdr->chain_ok != 0;
        for (int i = 0; i < kSegPerThread; ++i) {
            const uint64_t s = first + i;
            if (s >= nseg) break;
            const uint64_t a = off[s], b = off[s + 1];
            if (b < a || b > n) continue;
            const uint64_t len = b - a;
            if (len == 1) {
                if constexpr (!IDS) {
                    kout[a] = kin[a];
                    if (pout) {
                        pout[a] = pin[a];
                    }
                }
                continue;
            }
            if (len == 0) continue;
            const uint32_t c = seg_class(len);
            if (c < kSegClasses) {
                list[hdr->base[c] + f[c]] = static_cast<uint32_t>(s);
                f[c] += 1;
            } else {
                if (chain) {
                    const uint64_t j = f[SF_LARGE];
                    large[j] = SegLarge{a, b, a - f[SF_KEYS], IDS ? s : 0};
                    tstart[j] = static_cast<uint32_t>(f[SF_TILES]);
                }
                f[SF_LARGE] += 1;
                f[SF_TILES] += seg_tiles(a, b);
                f[SF_KEYS] += len;
            }
        }
    }
}

// One workgroup: exclusive scan of the block sums in place, totals and class bases -> hdr.  The chain runs only while the large
// segments stay within the bounds the host sized its buffers by (max_large, max_tiles, n keys): valid segments always do — they are
// disjoint — so a miss means bad offsets, which are reported anyway.  The first bad segment (+1) goes to the mapped host word, unless
// an earlier call's report is still pending there.
__global__ __launch_bounds__(kSegScanThreads) void seg_scan_kernel(uint64_t* __restrict__ bsum, uint32_t nblocks, SegHeader* __restrict__ hdr,
                                                                    uint32_t* __restrict__ tstart, uint64_t n, uint64_t max_large,
                                                                    uint64_t max_tiles, uint32_t* status_host)
{
    __shared__ uint64_t lds[(kSegScanThreads / kWave) * SF_SUMS];
    __shared__ unsigned long long first_bad;
    if (threadIdx.x == 0) {
        first_bad = ~0ull;
    }
    const uint32_t per = (nblocks + kSegScanThreads - 1) / kSegScanThreads;
    const uint32_t b0 = threadIdx.x * per;
    uint64_t f[SF_SUMS] = {0, 0, 0, 0, 0, 0};
    uint64_t bad = ~0ull;
    for (uint32_t i = 0; i < per; ++i) {
        if (b0 + i >= nblocks) break;
        const uint64_t* bp = bsum + static_cast<uint64_t>(b0 + i) * SF_STRIDE;
#pragma unroll
        for (int k = 0; k < SF_SUMS; ++k) {
            f[k] += bp[k];
        }
        bad = bad < bp[SF_BAD] ? bad : bp[SF_BAD];
    }
    uint64_t tot[SF_SUMS];
    block_scan_u64<kSegScanThreads, SF_SUMS>(f, tot, lds);
    if (bad != ~0ull) {
        atomicMin(&first_bad, static_cast<unsigned long long>(bad));
    }
    for (uint32_t i = 0; i < per; ++i) {
        if (b0 + i >= nblocks) break;
        uint64_t* bp = bsum + static_cast<uint64_t>(b0 + i) * SF_STRIDE;
#pragma unroll
        for (int k = 0; k < SF_SUMS; ++k) {
            const uint64_t c = bp[k];
            bp[k] = f[k];
            f[k] += c;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool ok = tot[SF_LARGE] <= max_large && tot[SF_TILES] <= max_tiles && tot[SF_KEYS] <= n;
        hdr->count[0] = static_cast<uint32_t>(tot[0]);
        hdr->count[1] = static_cast<uint32_t>(tot[1]);
        hdr->count[2] = static_cast<uint32_t>(tot[2]);
        hdr->base[0] = 0;
        hdr->base[1] = static_cast<uint32_t>(tot[0]);
        hdr->base[2] = static_cast<uint32_t>(tot[0] + tot[1]);
        hdr->nlarge = ok ? static_cast<uint32_t>(tot[SF_LARGE]) : 0u;
        hdr->tiles = ok ? static_cast<uint32_t>(tot[SF_TILES]) : 0u;
        hdr->chain_ok = ok ? 1u : 0u;
        if (ok && max_large) {          // (no large segment can exist when max_large is 0: the host allocated no tile starts)
            tstart[tot[SF_LARGE]] = static_cast<uint32_t>(tot[SF_TILES]);
        }
        if (first_bad != ~0ull && __hip_atomic_load(status_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
            __hip_atomic_store(status_host, static_cast<uint32_t>(first_bad + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// LDS image of one tile in the segmented kernels: tile_sort_kernel's (16 slots per row + 4 dwords of padding), any KPT that divides 16.
template <typename Key, int THREADS, int KPT>
struct SegSortLayout {
    static constexpr int TILE = THREADS * KPT;
    static constexpr int KD = sizeof(Key) / 4;
    static constexpr int XBUF_DW = TILE * KD + TILE / 4;
    static constexpr int CNT_DW = 8 * THREADS;
    static constexpr int TOTAL_DW = XBUF_DW + CNT_DW + 16 + kRadix + 2 * kRadix;   // image, counters, wave totals, digit starts, 16 x uint64 bases
    static constexpr size_t BYTES = static_cast<size_t>(TOTAL_DW) * 4;
    static_assert(KPT <= 16 && 16 % KPT == 0 && THREADS % kWave == 0 && TILE <= 32768, "geometry");
};

__device__ __forceinline__ uint32_t seg_image_dw(uint32_t slot, int kd)
{
    return slot * kd + ((slot >> 4) << 2);
}

// One stable 4-bit ranking round of the KPT keys each thread holds (thread t = slots KPT*t ..): tile_sort_kernel's ranking, i.e.
// nibble counters in a register, packed [digit&7][thread] words, a raking scan.  Gives every key's tile-local slot and (dstart) the
// first slot of every digit.  Two barriers; cnt / wtot / dstart are free again after the caller's next barrier.
template <typename Key, int THREADS, int KPT>
__device__ __forceinline__ void seg_rank(const Key (&k)[KPT], int shift, uint32_t (&slot)[KPT], uint32_t (&dg)[KPT], uint32_t* cnt,
                                         uint32_t* wtot, uint32_t* dstart)
{
    const uint32_t tid = threadIdx.x;
    u32_alias* cnt32 = reinterpret_cast<u32_alias*>(cnt);
    const u16_alias* cnt16 = reinterpret_cast<const u16_alias*>(cnt);
    constexpr uint32_t RAKE_STRIDE = THREADS / 8;
    uint64_t seen = 0;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        dg[i] = digit_of(k[i], shift, Key{0}, static_cast<uint32_t>(kRadix - 1));
        const uint32_t sh4 = dg[i] << 2;
        slot[i] = static_cast<uint32_t>(seen >> sh4) & 15u;
        if (i + 1 < KPT) {
            seen += 1ull << sh4;
        }
    }
    const uint32_t seen_lo = static_cast<uint32_t>(seen), seen_hi = static_cast<uint32_t>(seen >> 32);
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        cnt32[l * THREADS + tid] = __builtin_amdgcn_ubfe(seen_lo, 4u * l, 4u) | (__builtin_amdgcn_ubfe(seen_hi, 4u * l, 4u) << 16);
    }
    atomicAdd(cnt + (dg[KPT - 1] & 7u) * THREADS + tid, 1u << ((dg[KPT - 1] >> 3) * 16u));
    __syncthreads();
    {
        U32x4 a = *reinterpret_cast<const U32x4*>(cnt + tid * 8);
        U32x4 b = *reinterpret_cast<const U32x4*>(cnt + tid * 8 + 4);
        const uint32_t sum = a.v[0] + a.v[1] + a.v[2] + a.v[3] + b.v[0] + b.v[1] + b.v[2] + b.v[3];
        uint32_t total;
        uint32_t run = block_exclusive_scan<THREADS>(sum, wtot, total);
        run += total << 16;
        if ((tid % RAKE_STRIDE) == 0) {
            dstart[tid / RAKE_STRIDE] = run & 0xFFFFu;
            dstart[tid / RAKE_STRIDE + 8] = run >> 16;
        }
        uint32_t t;
        t = a.v[0]; a.v[0] = run; run += t;
        t = a.v[1]; a.v[1] = run; run += t;
        t = a.v[2]; a.v[2] = run; run += t;
        t = a.v[3]; a.v[3] = run; run += t;
        t = b.v[0]; b.v[0] = run; run += t;
        t = b.v[1]; b.v[1] = run; run += t;
        t = b.v[2]; b.v[2] = run; run += t;
        t = b.v[3]; b.v[3] = run;
        *reinterpret_cast<U32x4*>(cnt + tid * 8) = a;
        *reinterpret_cast<U32x4*>(cnt + tid * 8 + 4) = b;
    }
    __syncthreads();
    uint32_t first_of_digit[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        first_of_digit[i] = cnt16[(((dg[i] & 7u) * THREADS + tid) << 1) + (dg[i] >> 3)];
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        slot[i] += first_of_digit[i];
    }
}

// Segments of 2..THREADS*KPT keys, one per workgroup at a time (grid stride over the class's list): load (encode), `passes` stable
// rounds inside LDS, store (decode).  Pads (past the segment's end) are the encoded all-ones key: digit 15 in every pass, last in
// index order, never stored.
template <typename Key, int THREADS, int KPT, bool PAYLOAD>
__global__ __launch_bounds__(THREADS) void seg_small_sort_kernel(const Key* __restrict__ in, Key* __restrict__ out, const uint32_t* __restrict__ pin,
                                                                 uint32_t* __restrict__ pout, const uint64_t* __restrict__ off,
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
    const uint32_t count = hdr->count[cls], base = hdr->base[cls];
    const Key pad_key = codec_decode(static_cast<Key>(~Key{0}), codec.ea, codec.em);

#pragma unroll 1
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint32_t s = list[base + item];
        const uint64_t a = off[s];
        const uint64_t len64 = off[s + 1] - a;
        const uint32_t len = len64 < static_cast<uint64_t>(L::TILE) ? static_cast<uint32_t>(len64) : static_cast<uint32_t>(L::TILE);
        Key k[KPT];
        uint32_t pl[PAYLOAD ? KPT : 1];
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t li = tid * KPT + i;
            k[i] = codec_encode(li < len ? in[a + li] : pad_key, codec.ea, codec.em);
            if constexpr (PAYLOAD) {
                pl[i] = li < len ? pin[a + li] : 0u;
            }
        }
#pragma unroll 1
        for (int pass = 0; pass < passes; ++pass) {
            const bool last = pass + 1 == passes;
            uint32_t slot[KPT], dg[KPT];
            seg_rank<Key, THREADS, KPT>(k, pass * kRadixBits, slot, dg, cnt, wtot, dstart);
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                *reinterpret_cast<Key*>(xbuf + seg_image_dw(slot[i], KD)) = k[i];
            }
            __syncthreads();
            if (!last) {
#pragma unroll
                for (int i = 0; i < KPT; ++i) {
                    k[i] = *reinterpret_cast<const Key*>(xbuf + seg_image_dw(tid * KPT + i, KD));
                }
            } else {
#pragma unroll
                for (int r = 0; r < KPT; ++r) {
                    const uint32_t i = static_cast<uint32_t>(r) * THREADS + tid;
                    if (i < len) {
                        out[a + i] = codec_decode(*reinterpret_cast<const Key*>(xbuf + seg_image_dw(i, KD)), codec.da, codec.dm);
                    }
                }
            }
            if constexpr (PAYLOAD) {
                __syncthreads();           // every thread has taken its keys: the image carries the payload now
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
                        if (i < len) {
                            pout[a + i] = xbuf[seg_image_dw(i, 1)];
                        }
                    }
                }
            }
            __syncthreads();               // the image and the counters are free for the next round / segment
        }
    }
}

// Tile t of the large-segment chain: the segment (binary search over the tile starts), the key range, the first table entry and
// the table's row stride (= the segment's tile count).  Wave-uniform.
struct SegTile {
    uint64_t start, dest;
    uint32_t len, entry, stride;
};

__device__ __forceinline__ SegTile seg_tile(uint32_t t, const SegLarge* __restrict__ large, const uint32_t* __restrict__ tstart, uint32_t nlarge)
{
    uint32_t lo = 0, hi = nlarge;                  // tstart[lo] <= t < tstart[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tstart[mid] <= t) lo = mid; else hi = mid;
    }
    const uint32_t ts = tstart[lo], te = tstart[lo + 1];
    const SegLarge sg = large[lo];
    const uint32_t ti = t - ts;
    const uint64_t g = (sg.a >> kSegTileShift) + ti;
    const uint64_t g0 = g << kSegTileShift, g1 = (g + 1) << kSegTileShift;
    const uint64_t start = sg.a > g0 ? sg.a : g0;
    const uint64_t end = sg.b < g1 ? sg.b : g1;
    SegTile r;
    r.start = start;
    r.len = static_cast<uint32_t>(end - start);
    r.dest = sg.dest;
    r.entry = kRadix * ts + ti;
    r.stride = te - ts;
    return r;
}

// Digit counts of every tile of the large segments: table[16 * tstart[j] + digit * tiles(j) + tile of j].  codec: the first pass
// encodes (zero constants otherwise).
template <typename Key>
__global__ __launch_bounds__(kSegChainThreads) void seg_histogram_kernel(const Key* __restrict__ keys, uint32_t* __restrict__ table,
                                                                         const SegHeader* __restrict__ hdr, const SegLarge* __restrict__ large,
                                                                         const uint32_t* __restrict__ tstart, int shift, KeyCodec<Key> codec)
{
    constexpr int THREADS = kSegChainThreads, KPT = kSegChainKpt;
    constexpr int VEC = KeyVec<Key>::N;
    constexpr int NV = KPT / VEC;
    constexpr int REP = 32, RSTRIDE = kRadix + 1;
    __shared__ uint32_t cnt[REP * RSTRIDE];
    const uint32_t tid = threadIdx.x;
    const uint32_t ntiles = hdr->tiles, nlarge = hdr->nlarge;
    uint32_t* mine = cnt + (tid & (REP - 1)) * RSTRIDE;
    auto dig = [=](Key key) -> uint32_t { return digit_of(codec_encode(key, codec.ea, codec.em), shift, Key{0}, static_cast<uint32_t>(kRadix - 1)); };

#pragma unroll 1
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        for (uint32_t i = tid; i < REP * RSTRIDE; i += THREADS) {
            cnt[i] = 0;
        }
        __syncthreads();
        const SegTile tl = seg_tile(t, large, tstart, nlarge);
        if (tl.len == kSegTileKeys) {            // a whole tile of the global grid: 16-byte aligned
            KeyVec<Key> v[NV];
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                v[j] = load_keys16(keys + tl.start + static_cast<uint32_t>(j) * THREADS * VEC + tid * VEC);
            }
#pragma unroll
            for (int j = 0; j < NV; ++j) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    atomicAdd(&mine[dig(v[j].k[e])], 1u);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < KPT; ++r) {
                const uint32_t li = static_cast<uint32_t>(r) * THREADS + tid;
                if (li < tl.len) {
                    atomicAdd(&mine[dig(keys[tl.start + li])], 1u);
                }
            }
        }
        __syncthreads();
        if (tid < kRadix) {
            uint32_t s = 0;
#pragma unroll
            for (int r = 0; r < REP; ++r) {
                s += cnt[r * RSTRIDE + tid];
            }
            table[tl.entry + tid * tl.stride] = s;
        }
        __syncthreads();
    }
}

// The stable scatter of one pass over the tiles of the large segments.  The table is the flat exclusive scan of the counts, so
// entry (j, d, tile) minus the keys of the large segments before j is where the tile's keys of digit d start inside segment j.
template <typename Key, bool PAYLOAD>
__global__ __launch_bounds__(kSegChainThreads) void seg_reorder_kernel(const Key* __restrict__ in, Key* __restrict__ out, const uint32_t* __restrict__ pin,
                                                                       uint32_t* __restrict__ pout, const uint32_t* __restrict__ table,
                                                                       const SegHeader* __restrict__ hdr, const SegLarge* __restrict__ large,
                                                                       const uint32_t* __restrict__ tstart, int shift, KeyCodec<Key> codec)
{
    constexpr int THREADS = kSegChainThreads, KPT = kSegChainKpt;
    using L = SegSortLayout<Key, THREADS, KPT>;
    constexpr int KD = L::KD;
    constexpr int VEC = KeyVec<Key>::N;
    constexpr int NV = KPT / VEC;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* xbuf = smem;
    uint32_t* cnt = smem + L::XBUF_DW;
    uint32_t* wtot = cnt + L::CNT_DW;
    uint32_t* dstart = wtot + 16;
    uint64_t* gbase = reinterpret_cast<uint64_t*>(dstart + kRadix);     // per digit: global slot of tile-local slot 0
    const uint32_t tid = threadIdx.x;
    const uint32_t ntiles = hdr->tiles, nlarge = hdr->nlarge;
    const Key pad_key = codec_decode(static_cast<Key>(~Key{0}), codec.ea, codec.em);

#pragma unroll 1
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const SegTile tl = seg_tile(t, large, tstart, nlarge);
        Key k[KPT];
        uint32_t pl[PAYLOAD ? KPT : 1];
        if (tl.len == kSegTileKeys) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const KeyVec<Key> v = load_keys16(in + tl.start + tid * KPT + j * VEC);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    k[j * VEC + e] = v.k[e];
                }
            }
            if constexpr (PAYLOAD) {
#pragma unroll
                for (int q = 0; q < KPT / 4; ++q) {
                    const U32x4 x = *reinterpret_cast<const U32x4*>(pin + tl.start + tid * KPT + q * 4);
                    pl[q * 4 + 0] = x.v[0];
                    pl[q * 4 + 1] = x.v[1];
                    pl[q * 4 + 2] = x.v[2];
                    pl[q * 4 + 3] = x.v[3];
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                const uint32_t li = tid * KPT + i;
                k[i] = li < tl.len ? in[tl.start + li] : pad_key;
                if constexpr (PAYLOAD) {
                    pl[i] = li < tl.len ? pin[tl.start + li] : 0u;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            k[i] = codec_encode(k[i], codec.ea, codec.em);
        }
        uint32_t slot[KPT], dg[KPT];
        seg_rank<Key, THREADS, KPT>(k, shift, slot, dg, cnt, wtot, dstart);
        if (tid < kRadix) {
            gbase[tid] = tl.dest + table[tl.entry + tid * tl.stride] - dstart[tid];
        }
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            *reinterpret_cast<Key*>(xbuf + seg_image_dw(slot[i], KD)) = k[i];
        }
        __syncthreads();
        uint32_t od[KPT];              // digit of the key in output slot r * THREADS + tid (for the payload)
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            const uint32_t i = static_cast<uint32_t>(r) * THREADS + tid;
            const Key y = *reinterpret_cast<const Key*>(xbuf + seg_image_dw(i, KD));
            od[r] = digit_of(y, shift, Key{0}, static_cast<uint32_t>(kRadix - 1));
            if (i < tl.len) {
                out[gbase[od[r]] + i] = codec_decode(y, codec.da, codec.dm);
            }
        }
        if constexpr (PAYLOAD) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                xbuf[seg_image_dw(slot[i], 1)] = pl[i];
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < KPT; ++r) {
                const uint32_t i = static_cast<uint32_t>(r) * THREADS + tid;
                if (i < tl.len) {
                    pout[gbase[od[r]] + i] = xbuf[seg_image_dw(i, 1)];
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace rsx
