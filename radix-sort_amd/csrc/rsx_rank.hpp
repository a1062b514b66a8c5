// rsx_rank.hpp — kernels of rsx_segmented_rank: the rank of every key inside its segment [off[s], off[s+1]) under one of five tie rules,
// and the size of its tie group.  Included by rsx_capi.hip (host side: capi_rank.inc); the rules: rsx_rank_math.hpp.
//
//   rank_ones_kernel     per segment: one-key segments get rank 0 and 1 tie; reports the first bad segment under this call's name
//   rank_small_kernel    segments of 2..4096 keys, one workgroup each in the segmented sort's three class shapes: (encoded key, position)
//                        sorted in LDS with seg_rank, head flags, three scans, ranks written to the LDS slot of their position, stored
//                        in index order.  Nothing but the keys is read and nothing but the result written.
//   rank_flat_kernel     d_offsets == NULL: the one segment [0, n) as the chain's header, large-segment table and tile starts
//   rank_edge_kernel     per tile of the sorted large segments (the chain's tiles: the 4096-key grid clipped at segment ends): heads, first
//                        head, last head -> the tile's record
//   rank_join_kernel     per large segment: the three scans of rsx_rank_math.hpp over its tiles' records -> every tile's carries
//   rank_write_kernel    per tile: recomputes the heads; rank and tie count of every key to the position it came from (the sort's payload)
//
// A HEAD is a sorted key whose bits differ from its predecessor's, or the first key of its segment: equality of bit patterns, which is
// equality under every order map, as in rsx_unique.hpp.  Positions inside the kernels are relative to the segment.  The tile records live
// in the segmented table, which the sort chain has finished with: kRankRec words per tile.
#pragma once

#include "rsx_common.hpp"
#include "rsx_rank_math.hpp"
#include "rsx_segmented.hpp"
#include "rsx_unique.hpp"

namespace rsx {

constexpr int kRankThreads = kSegChainThreads, kRankKpt = kSegChainKpt;      // one tile = 256 x 16 keys, thread t holds keys 16t .. 16t+15
constexpr int kRankSmallThreads = 256;
constexpr int kRankRec = 8;                 // words of a tile's record: heads, first, last, -, start, next, dense, -
constexpr int kRankScanWords = 12;          // LDS words of rank_block_scan
static_assert(kRankRec <= kRadix, "the records must fit the segmented table");

struct RankScan {
    uint32_t prev;          // the last head in the threads before (kNone: none)
    uint32_t next;          // the first head in the threads after (kNone: none)
    uint32_t before;        // the heads in the threads before
};

// The three scans of rsx_rank_math.hpp over the workgroup, exclusive, of one piece per thread.  Two barriers; w is free after them.
template <int THREADS>
__device__ __forceinline__ RankScan rank_block_scan(uint32_t last, uint32_t first, uint32_t heads, uint32_t* w)
{
    constexpr int WAVES = THREADS / kWave;
    static_assert(WAVES <= 4, "w holds three rows of four");
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t a = last, b = first, c = heads;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t ya = __shfl_up(a, d), yb = __shfl_down(b, d), yc = __shfl_up(c, d);
        a = lane >= static_cast<uint32_t>(d) ? rsx_rank::carry_start(ya, a) : a;
        b = lane + static_cast<uint32_t>(d) < static_cast<uint32_t>(kWave) ? rsx_rank::carry_next(yb, b) : b;
        c += lane >= static_cast<uint32_t>(d) ? yc : 0u;
    }
    if (lane == kWave - 1) {
        w[wave] = a;
        w[8 + wave] = c;
    }
    if (lane == 0) {
        w[4 + wave] = b;
    }
    uint32_t ea = __shfl_up(a, 1), eb = __shfl_down(b, 1);
    ea = lane == 0 ? rsx_rank::kNone : ea;
    eb = lane == kWave - 1 ? rsx_rank::kNone : eb;
    __syncthreads();
    uint32_t pa = rsx_rank::kNone, pb = rsx_rank::kNone, pc = 0;
#pragma unroll
    for (int x = 0; x < WAVES; ++x) {
        if (static_cast<uint32_t>(x) < wave) {
            pa = rsx_rank::carry_start(pa, w[x]);
            pc = rsx_rank::carry_dense(pc, w[8 + x]);
        }
    }
#pragma unroll
    for (int x = WAVES - 1; x >= 0; --x) {
        if (static_cast<uint32_t>(x) > wave) {
            pb = rsx_rank::carry_next(pb, w[4 + x]);
        }
    }
    __syncthreads();
    RankScan r;
    r.prev = rsx_rank::carry_start(pa, ea);
    r.next = rsx_rank::carry_next(pb, eb);
    r.before = pc + c - heads;
    return r;
}

// A thread's piece: its head bits (bit j = position rel + j) as the scans' input.
__device__ __forceinline__ void rank_piece(uint32_t hbits, uint32_t rel, uint32_t& last, uint32_t& first, uint32_t& heads)
{
    last = hbits ? rel + 31u - static_cast<uint32_t>(__clz(static_cast<int>(hbits))) : rsx_rank::kNone;
    first = hbits ? rel + static_cast<uint32_t>(__ffs(static_cast<int>(hbits))) - 1u : rsx_rank::kNone;
    heads = static_cast<uint32_t>(__popc(hbits));
}

// Key j of the thread: its run [start, end) and the distinct keys before it, from the thread's bits and what lies outside the thread
// (prev: the last head before the thread, next: the first head after it or the segment's end, dense: the heads before the thread).
__device__ __forceinline__ void rank_element(uint32_t hbits, int j, uint32_t rel, uint32_t prev, uint32_t next, uint32_t dense, uint32_t method,
                                             uint32_t& rank, uint32_t& ties)
{
    const uint32_t upto = hbits & ((2u << j) - 1u), after = (hbits >> j) >> 1;
    const uint32_t start = upto ? rel + 31u - static_cast<uint32_t>(__clz(static_cast<int>(upto))) : prev;
    const uint32_t end = after ? rel + static_cast<uint32_t>(j) + static_cast<uint32_t>(__ffs(static_cast<int>(after))) : next;
    rank = rsx_rank::rank_of(method, start, end, dense + static_cast<uint32_t>(__popc(upto)) - 1u, rel + static_cast<uint32_t>(j));
    ties = rsx_rank::ties_of(start, end);
}

// One-key segments, and the report: the first bad segment + 1 goes to the mapped host word with this call's id beside it, unless an
// earlier report is still pending there (the sort chain that follows then leaves the words alone).
__global__ __launch_bounds__(kRankSmallThreads) void rank_ones_kernel(const uint64_t* __restrict__ off, uint64_t nseg, const uint32_t* __restrict__ bad,
                                                                       uint32_t* __restrict__ rank_out, uint32_t* __restrict__ ties_out,
                                                                       uint32_t* status_host, uint32_t call_id)
{
    const uint32_t b = *bad;
    if (b != kUniqNoBad) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && __hip_atomic_load(status_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
            __hip_atomic_store(status_host + 1, call_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(status_host, b + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);        // (after the call's id)
        }
        return;
    }
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kRankSmallThreads;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kRankSmallThreads + threadIdx.x; s < nseg; s += stride) {
        const uint64_t a = off[s];
        if (off[s + 1] - a == 1) {
            rank_out[a] = 0u;
            if (ties_out) {
                ties_out[a] = 1u;
            }
        }
    }
}

// Segments of 2..THREADS*KPT keys, one per workgroup at a time (grid stride over the class's list), seg_small_sort_kernel's rounds with the
// positions 0 .. len-1 generated as the payload.  Pads (past the segment's end) are the encoded all-ones key with the positions len ..:
// last in every round, so the sorted slots below len are the segment's keys.
template <typename Key, int THREADS, int KPT>
__global__ __launch_bounds__(THREADS) void rank_small_kernel(const Key* __restrict__ in, const uint64_t* __restrict__ off, const uint32_t* __restrict__ list,
                                                             const SegHeader* __restrict__ hdr, const uint32_t* __restrict__ bad, int cls, int passes, Key ea,
                                                             Key em, uint32_t method, uint32_t* __restrict__ rank_out, uint32_t* __restrict__ ties_out)
{
    using L = SegSortLayout<Key, THREADS, KPT>;
    constexpr int KD = L::KD;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* xbuf = smem;
    uint32_t* cnt = smem + L::XBUF_DW;
    uint32_t* wtot = cnt + L::CNT_DW;
    uint32_t* dstart = wtot + 16;
    static_assert(kRankScanWords <= 16, "the scans use the wave totals' words");
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    if (*bad != kUniqNoBad) return;
    const uint32_t count = hdr->count[cls], base = hdr->base[cls];
    const Key pad_key = static_cast<Key>(~Key{0});

#pragma unroll 1
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint32_t s = list[base + item];
        const uint64_t a = off[s];
        const uint64_t len64 = off[s + 1] - a;
        const uint32_t len = len64 < static_cast<uint64_t>(L::TILE) ? static_cast<uint32_t>(len64) : static_cast<uint32_t>(L::TILE);
        Key k[KPT];
        uint32_t pl[KPT];
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t li = tid * KPT + i;
            k[i] = li < len ? codec_encode(in[a + li], ea, em) : pad_key;
            pl[i] = li;
        }
        Key left = Key{0};
#pragma unroll 1
        for (int pass = 0; pass < passes; ++pass) {
            uint32_t slot[KPT], dg[KPT];
            seg_rank<Key, THREADS, KPT>(k, pass * kRadixBits, slot, dg, cnt, wtot, dstart);
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                *reinterpret_cast<Key*>(xbuf + seg_image_dw(slot[i], KD)) = k[i];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                k[i] = *reinterpret_cast<const Key*>(xbuf + seg_image_dw(tid * KPT + i, KD));
            }
            if (pass + 1 == passes && lane == 0 && tid > 0) {          // the key before the wave's first, for the head flags
                left = *reinterpret_cast<const Key*>(xbuf + seg_image_dw(tid * KPT - 1, KD));
            }
            __syncthreads();               // every thread has taken its keys: the image carries the positions now
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                xbuf[seg_image_dw(slot[i], 1)] = pl[i];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                pl[i] = xbuf[seg_image_dw(tid * KPT + i, 1)];
            }
            __syncthreads();               // the image and the counters are free for the next round
        }
        // heads of the sorted slots, the three scans, the ranks
        const Key up = __shfl_up(k[KPT - 1], 1);
        if (lane != 0) {
            left = up;
        }
        const uint32_t rel = tid * KPT;
        uint32_t hbits = 0;
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t li = rel + i;
            const bool head = li < len && (li == 0 || k[i] != (i ? k[i > 0 ? i - 1 : 0] : left));
            hbits |= head ? 1u << i : 0u;
        }
        uint32_t last, first, heads;
        rank_piece(hbits, rel, last, first, heads);
        const RankScan sc = rank_block_scan<THREADS>(last, first, heads, wtot);
        const uint32_t next = rsx_rank::carry_next(len, sc.next);
        uint32_t tie[KPT];
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            uint32_t rank;
            rank_element(hbits, i, rel, sc.prev, next, sc.before, method, rank, tie[i]);
            if (rel + i < len) {
                xbuf[seg_image_dw(pl[i], 1)] = rank;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            const uint32_t i = static_cast<uint32_t>(r) * THREADS + tid;
            if (i < len) {
                rank_out[a + i] = xbuf[seg_image_dw(i, 1)];
            }
        }
        __syncthreads();
        if (ties_out) {
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                if (rel + i < len) {
                    xbuf[seg_image_dw(pl[i], 1)] = tie[i];
                }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < KPT; ++r) {
                const uint32_t i = static_cast<uint32_t>(r) * THREADS + tid;
                if (i < len) {
                    ties_out[a + i] = xbuf[seg_image_dw(i, 1)];
                }
            }
            __syncthreads();
        }
    }
}

// The flat form: what the classify chain would have left for the one large segment [0, n).
__global__ __launch_bounds__(kWave) void rank_flat_kernel(SegHeader* __restrict__ hdr, SegLarge* __restrict__ large, uint32_t* __restrict__ tstart, uint64_t n)
{
    if (threadIdx.x == 0) {
        const uint32_t tiles = static_cast<uint32_t>((n + kSegTileKeys - 1) >> kSegTileShift);
        hdr->count[0] = hdr->count[1] = hdr->count[2] = 0;
        hdr->base[0] = hdr->base[1] = hdr->base[2] = 0;
        hdr->nlarge = 1;
        hdr->tiles = tiles;
        hdr->chain_ok = 1;
        large[0] = SegLarge{0, n, 0, 0};
        tstart[0] = 0;
        tstart[1] = tiles;
    }
}

// Tile t of the sorted large segments: seg_tile's walk, with what the rank needs of the segment.  Wave-uniform.
struct RankTile {
    uint64_t start, a;          // the tile's first key and the segment's, global
    uint32_t len, seg_len;
};

__device__ __forceinline__ RankTile rank_tile(uint32_t t, const SegLarge* __restrict__ large, const uint32_t* __restrict__ tstart, uint32_t nlarge)
{
    uint32_t lo = 0, hi = nlarge;                  // tstart[lo] <= t < tstart[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tstart[mid] <= t) lo = mid; else hi = mid;
    }
    const SegLarge sg = large[lo];
    const uint64_t g = (sg.a >> kSegTileShift) + (t - tstart[lo]);
    const uint64_t g0 = g << kSegTileShift, g1 = (g + 1) << kSegTileShift;
    const uint64_t start = sg.a > g0 ? sg.a : g0;
    const uint64_t end = sg.b < g1 ? sg.b : g1;
    RankTile r;
    r.start = start;
    r.a = sg.a;
    r.len = static_cast<uint32_t>(end - start);
    r.seg_len = static_cast<uint32_t>(sg.b - sg.a);
    return r;
}

// The thread's 16 sorted keys of the tile and their head bits (bit j = key 16 * tid + j of the tile).  No barrier.
template <typename Key>
__device__ __forceinline__ uint32_t rank_tile_heads(const Key* __restrict__ keys, const RankTile& tl)
{
    constexpr int VEC = KeyVec<Key>::N;
    constexpr int NV = kRankKpt / VEC;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t li0 = tid * kRankKpt;
    Key k[kRankKpt];
    if (tl.len == kSegTileKeys) {            // a whole tile of the global grid: 16-byte aligned
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const KeyVec<Key> v = load_keys16(keys + tl.start + li0 + q * VEC);
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                k[q * VEC + c] = v.k[c];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kRankKpt; ++j) {
            k[j] = li0 + j < tl.len ? keys[tl.start + li0 + j] : Key{0};
        }
    }
    Key left = Key{0};
    if (lane == 0 && li0 < tl.len && (li0 > 0 || tl.start > tl.a)) {
        left = keys[tl.start + li0 - 1];
    }
    const Key up = __shfl_up(k[kRankKpt - 1], 1);
    if (lane != 0) {
        left = up;
    }
    const bool seg_first = tl.start == tl.a;
    uint32_t hbits = 0;
#pragma unroll
    for (int j = 0; j < kRankKpt; ++j) {
        const uint32_t li = li0 + j;
        const bool head = li < tl.len && ((li == 0 && seg_first) || k[j] != (j ? k[j > 0 ? j - 1 : 0] : left));
        hbits |= head ? 1u << j : 0u;
    }
    return hbits;
}

template <typename Key>
__global__ __launch_bounds__(kRankThreads) void rank_edge_kernel(const Key* __restrict__ keys, const uint32_t* __restrict__ bad,
                                                                 const SegHeader* __restrict__ hdr, const SegLarge* __restrict__ large,
                                                                 const uint32_t* __restrict__ tstart, uint32_t* __restrict__ table)
{
    __shared__ uint32_t w[kRankScanWords];
    const uint32_t tid = threadIdx.x;
    if (*bad != kUniqNoBad) return;
    const uint32_t ntiles = hdr->tiles, nlarge = hdr->nlarge;
#pragma unroll 1
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RankTile tl = rank_tile(t, large, tstart, nlarge);
        const uint32_t hbits = rank_tile_heads(keys, tl);
        uint32_t last, first, heads;
        rank_piece(hbits, static_cast<uint32_t>(tl.start - tl.a) + tid * kRankKpt, last, first, heads);
        const RankScan sc = rank_block_scan<kRankThreads>(last, first, heads, w);
        uint32_t* rec = table + static_cast<uint64_t>(t) * kRankRec;
        if (tid == kRankThreads - 1) {
            rec[0] = rsx_rank::carry_dense(sc.before, heads);
            rec[2] = rsx_rank::carry_start(sc.prev, last);
        }
        if (tid == 0) {
            rec[1] = rsx_rank::carry_next(sc.next, first);
        }
    }
}

// One workgroup per large segment at a time: thread x folds the records of `per` consecutive tiles, the workgroup scans the 256 pieces,
// and every thread walks its tiles again, forward for start and dense, backward for next.
__global__ __launch_bounds__(kRankThreads) void rank_join_kernel(const uint32_t* __restrict__ bad, const SegHeader* __restrict__ hdr,
                                                                 const SegLarge* __restrict__ large, const uint32_t* __restrict__ tstart,
                                                                 uint32_t* __restrict__ table)
{
    __shared__ uint32_t w[kRankScanWords];
    const uint32_t tid = threadIdx.x;
    if (*bad != kUniqNoBad) return;
    const uint32_t nlarge = hdr->nlarge;
#pragma unroll 1
    for (uint32_t j = blockIdx.x; j < nlarge; j += gridDim.x) {
        const uint32_t ts = tstart[j], T = tstart[j + 1] - ts;
        const SegLarge sg = large[j];
        const uint32_t L = static_cast<uint32_t>(sg.b - sg.a);
        const uint32_t per = (T + kRankThreads - 1) / kRankThreads;
        const uint32_t x0 = min(tid * per, T), x1 = min(x0 + per, T);
        uint32_t* recs = table + static_cast<uint64_t>(ts) * kRankRec;
        uint32_t last = rsx_rank::kNone, first = rsx_rank::kNone, heads = 0;
        for (uint32_t x = x0; x < x1; ++x) {
            const uint32_t* rec = recs + static_cast<uint64_t>(x) * kRankRec;
            heads = rsx_rank::carry_dense(heads, rec[0]);
            first = rsx_rank::carry_next(rec[1], first);          // (the earlier head wins)
            last = rsx_rank::carry_start(last, rec[2]);
        }
        const RankScan sc = rank_block_scan<kRankThreads>(last, first, heads, w);
        uint32_t start = sc.prev, dense = sc.before;
        for (uint32_t x = x0; x < x1; ++x) {
            uint32_t* rec = recs + static_cast<uint64_t>(x) * kRankRec;
            rec[4] = start;
            rec[6] = dense;
            start = rsx_rank::carry_start(start, rec[2]);
            dense = rsx_rank::carry_dense(dense, rec[0]);
        }
        uint32_t next = sc.next;
        for (uint32_t x = x1; x-- > x0;) {
            uint32_t* rec = recs + static_cast<uint64_t>(x) * kRankRec;
            rec[5] = next != rsx_rank::kNone ? next : L;
            next = rsx_rank::carry_next(next, rec[1]);
        }
    }
}

// A position read from perm is used as an index only when it is below n (after bad offsets the sort's scratch is undefined; such a call
// does not get this far, the test stays).
template <typename Key>
__global__ __launch_bounds__(kRankThreads) void rank_write_kernel(const Key* __restrict__ keys, const uint32_t* __restrict__ perm, uint64_t n,
                                                                  const uint32_t* __restrict__ bad, const SegHeader* __restrict__ hdr,
                                                                  const SegLarge* __restrict__ large, const uint32_t* __restrict__ tstart,
                                                                  const uint32_t* __restrict__ table, uint32_t method, uint32_t* __restrict__ rank_out,
                                                                  uint32_t* __restrict__ ties_out)
{
    __shared__ uint32_t w[kRankScanWords];
    const uint32_t tid = threadIdx.x;
    if (*bad != kUniqNoBad) return;
    const uint32_t ntiles = hdr->tiles, nlarge = hdr->nlarge;
#pragma unroll 1
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RankTile tl = rank_tile(t, large, tstart, nlarge);
        const uint32_t li0 = tid * kRankKpt;
        uint32_t p[kRankKpt];
        if (tl.len == kSegTileKeys) {
#pragma unroll
            for (int q = 0; q < kRankKpt / 4; ++q) {
                const U32x4 v = *reinterpret_cast<const U32x4*>(perm + tl.start + li0 + q * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    p[q * 4 + c] = v.v[c];
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < kRankKpt; ++j) {
                p[j] = li0 + j < tl.len ? perm[tl.start + li0 + j] : 0u;
            }
        }
        const uint32_t hbits = rank_tile_heads(keys, tl);
        const uint32_t rel = static_cast<uint32_t>(tl.start - tl.a) + li0;
        uint32_t last, first, heads;
        rank_piece(hbits, rel, last, first, heads);
        const RankScan sc = rank_block_scan<kRankThreads>(last, first, heads, w);
        const uint32_t* rec = table + static_cast<uint64_t>(t) * kRankRec;
        const uint32_t prev = rsx_rank::carry_start(rec[4], sc.prev);
        const uint32_t next = rsx_rank::carry_next(rec[5], sc.next);
        const uint32_t dense = rsx_rank::carry_dense(rec[6], sc.before);
#pragma unroll
        for (int j = 0; j < kRankKpt; ++j) {
            uint32_t rank, ties;
            rank_element(hbits, j, rel, prev, next, dense, method, rank, ties);
            if (li0 + j < tl.len && p[j] < n) {
                rank_out[p[j]] = rank;
                if (ties_out) {
                    ties_out[p[j]] = ties;
                }
            }
        }
    }
}

}  // namespace rsx
