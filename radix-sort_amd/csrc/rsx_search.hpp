// rsx_search.hpp — kernel of rsx_segmented_search: lower / upper bound of every query in the sorted haystack segment of the same number
// (thrust's vectorised binary search, torch.searchsorted / bucketize with ragged rows).  Included by rsx_capi.hip (host side:
// capi_search.inc).
//
//   (unique_reset_kernel + unique_validate_kernel, unchanged, once per offsets array: the first bad segment of either, one word)
//   search_kernel   the work is tiled over the QUERIES.  A tile is kSearchTileQ = 1024 consecutive query positions of the global grid
//                   (tile t = positions [1024 t, 1024 t + 1024)); a workgroup of 256 threads takes it, thread q the positions q, q + 256,
//                   q + 512, q + 768 of the tile, so that every load of queries and every store of results is coalesced.  Workgroup b
//                   takes the tiles [b * chunk, (b + 1) * chunk), chunk = ceil(tiles / (16 x CUs)): the scan's rule.
//
// THE ORDER.  Keys and queries are compared as plain unsigned numbers after codec_encode with the engine's (A, M) (rsx_common.hpp): the
// map the sort itself uses, so "before" is before in the order the haystack was sorted in, whatever the key kind and direction, and
// "equal" is equality of bit patterns.  Queries are encoded once, as they are loaded; keys as they are staged or probed.  Memory is never
// rewritten.  With before(k) = k < q, or k <= q under RSX_SEARCH_RIGHT, the result is #{ i in the segment : before(key_i) }, found as the
// partition point of a branch-free bisection: (base, len) -> before(key[base + len / 2]) ? (base + len / 2 + 1, len - len / 2 - 1)
// : (base, len / 2).  Every index it forms lies in [0, L): on a haystack that is not sorted the result is unspecified but in [0, L], and
// nothing outside the segment is read.  A thread runs the bisections of its four queries in lockstep, four loads in flight per step.
//
// A tile finds the segment of its first and of its last live query — a bisection in qoff, one division in the even form, nothing with one
// segment — and takes one of three paths (uniform over the workgroup).  With Qt the tile's live queries and L the segment's keys:
//   RESIDENT  first and last segment are the same, L <= 4096 (kSegTileKeys) and 16 Qt >= L.  The segment is staged in LDS, encoded:
//             16-byte loads over the part of it that is 16-byte aligned, element loads for the head before and the tail after.  Every
//             bisection runs in LDS.  The rule: staging reads L keys once, coalesced; a direct search reads about log2 L <= 12 dependent
//             sectors per query; below one query per 16 keys the staging costs more sectors than the probes it saves.
//   SAMPLED   the same segment, L > 4096 and Qt >= 256.  The kSearchSamples = 1024 keys at the positions p(i) = floor(i L / 1024),
//             i = 0 .. 1023, are staged in LDS, encoded (p(0) = 0; the stride is at least 4).  The bisection over the samples — ten levels —
//             gives c = #{ i : before(sample_i) }.  c = 0: the result is 0 (key 0 is not before q).  Otherwise key p(c-1) is before q and
//             key p(c) (c = 1024: the end, L) is not: the result lies in [p(c-1) + 1, p(c)] and the remaining levels bisect that window in
//             global memory.  Below a quarter of a tile the 1024 sample loads cost more than the ten levels of the queries they serve.
//   DIRECT    everything else: the tile spans several segments, or the staging does not pay.  Every thread finds the segment of each of
//             its queries (a bisection in qoff between the tile's first and last segment; a division in the even form) and bisects it in
//             global memory.
// A workgroup that walks several tiles keeps what it has staged: the next tile of the same segment and path searches it as it is.
// RSX_SEARCH_SAMPLED=0 in the environment of rsx_create sends what would be SAMPLED to DIRECT (tools/search_bench.py measures the two).
//
// One instantiation per key width; key kind and direction are the two codec constants among the arguments.  No atomics, no cross-lane
// operation, no workgroup waits for another.  Static LDS: 4096 keys (16 KiB / 32 KiB).
#pragma once

#include "rsx_unique.hpp"

namespace rsx {

constexpr int kSearchThreads = 256, kSearchQpt = 4;
constexpr int kSearchTileShift = 10;
constexpr uint32_t kSearchTileQ = 1u << kSearchTileShift;       // = kSearchThreads * kSearchQpt
constexpr uint32_t kSearchSamples = 1024;
constexpr int kSearchSampleShift = 10;
constexpr uint32_t kSearchResidentMax = kSegTileKeys;           // keys of a segment that is staged whole
constexpr uint32_t kSearchResidentPay = 16;                     // ... when kSearchResidentPay * Qt >= L
constexpr uint32_t kSearchSampledPay = 256;                     // live queries of a tile from which the samples are staged
constexpr uint32_t kSearchRight = 4u;                           // RSX_SEARCH_RIGHT
constexpr uint32_t kSearchNoSampled = 1u;                       // mode bit: SAMPLED tiles take DIRECT
static_assert(kSearchTileQ == kSearchThreads * kSearchQpt, "a thread holds kSearchQpt queries of a tile");

// largest s in [lo, hi] with qoff[s] <= j (qoff[lo] <= j is the caller's): the segment of query position j, empty segments skipped
__device__ __forceinline__ uint64_t search_segment_of(const uint64_t* __restrict__ qoff, uint64_t lo, uint64_t hi, uint64_t j)
{
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (qoff[mid] <= j) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return lo;
}

// kSearchQpt bisections in lockstep.  at(r, i) = the encoded key i of query r's range; (base[r], len[r]) in, base[r] = the count out.
template <typename Key, typename At>
__device__ __forceinline__ void search_bisect(At&& at, const Key (&q)[kSearchQpt], bool right, uint32_t (&base)[kSearchQpt], uint32_t (&len)[kSearchQpt])
{
    uint32_t any = 0;
#pragma unroll
    for (int r = 0; r < kSearchQpt; ++r) {
        any |= len[r];
    }
    while (any != 0) {
        Key k[kSearchQpt];
#pragma unroll
        for (int r = 0; r < kSearchQpt; ++r) {
            k[r] = len[r] != 0 ? at(r, base[r] + (len[r] >> 1)) : Key{0};
        }
        any = 0;
#pragma unroll
        for (int r = 0; r < kSearchQpt; ++r) {
            const uint32_t half = len[r] >> 1;
            const bool before = len[r] != 0 && (right ? k[r] <= q[r] : k[r] < q[r]);
            base[r] = before ? base[r] + half + 1 : base[r];
            len[r] = before ? len[r] - half - 1 : half;
            any |= len[r];
        }
    }
}

template <typename Key>
__global__ __launch_bounds__(kSearchThreads) void search_kernel(const Key* __restrict__ keys, uint64_t n, const uint64_t* __restrict__ off, uint64_t nseg,
                                                                const Key* __restrict__ queries, uint64_t nq, const uint64_t* __restrict__ qoff,
                                                                uint32_t qper, const uint32_t* __restrict__ bad, uint32_t* status_host,
                                                                uint32_t ntiles, uint32_t chunk, uint32_t flags, uint32_t mode, Key ca, Key cm,
                                                                uint32_t* __restrict__ out)
{
    __shared__ Key stage[kSearchResidentMax];
    constexpr int VEC = KeyVec<Key>::N;
    constexpr uint32_t kNone = 0, kResident = 1, kSampled = 2;
    const uint32_t tid = threadIdx.x;
    const uint32_t b = *bad;
    if (b != kUniqNoBad) {                                        // nothing is written; the first bad segment + 1 goes to the mapped host word
        if (blockIdx.x == 0 && tid == 0 && __hip_atomic_load(status_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
            __hip_atomic_store(status_host, b + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    const uint64_t qlo = qoff ? qoff[0] : 0ull, qhi = qoff ? qoff[nseg] : nq;
    const bool right = (flags & kSearchRight) != 0;
    uint32_t staged = kNone;                                      // (uniform) what `stage` holds, and of which segment
    uint64_t staged_seg = 0;
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint64_t tile_start = static_cast<uint64_t>(t) << kSearchTileShift;
        const uint64_t a = max(tile_start, qlo), e = min(tile_start + kSearchTileQ, qhi);
        if (a >= e) continue;                                     // (uniform) no live query
        // the segments of the first and the last live query
        uint64_t s_first = 0, s_last = 0;
        if (qoff) {
            s_first = search_segment_of(qoff, 0, nseg - 1, a);
            s_last = search_segment_of(qoff, s_first, nseg - 1, e - 1);
        } else if (off) {
            s_first = static_cast<uint32_t>(a) / qper;            // (a < 2^31)
            s_last = e - 1 < (s_first + 1) * qper ? s_first : s_first + 1;      // (only compared with s_first)
        }
        Key q[kSearchQpt];
        bool live[kSearchQpt];
#pragma unroll
        for (int r = 0; r < kSearchQpt; ++r) {
            const uint64_t j = tile_start + tid + static_cast<uint32_t>(r) * kSearchThreads;
            live[r] = j >= a && j < e;
            q[r] = live[r] ? codec_encode(queries[j], ca, cm) : Key{0};
        }
        uint32_t base[kSearchQpt], len[kSearchQpt];
        uint32_t path = kNone;                                    // kNone: direct
        uint64_t hs = 0;
        uint32_t L = 0;
        if (s_first == s_last) {
            hs = uniq_off(off, s_first, n);
            L = static_cast<uint32_t>(uniq_off(off, s_first + 1, n) - hs);
            const uint32_t qt = static_cast<uint32_t>(e - a);
            if (L <= kSearchResidentMax) {
                path = static_cast<uint64_t>(qt) * kSearchResidentPay >= L ? kResident : kNone;
            } else {
                path = qt >= kSearchSampledPay && !(mode & kSearchNoSampled) ? kSampled : kNone;
            }
        }
        if (path != kNone && (staged != path || staged_seg != s_first)) {
            const Key* seg = keys + hs;
            if (path == kResident) {
                // [hs, hs + L) = head | 16-byte vectors | tail; head = the keys before the first 16-byte boundary
                const uint32_t mis = static_cast<uint32_t>(hs & (VEC - 1));
                const uint32_t head = min(mis ? VEC - mis : 0u, L);
                const uint32_t nvec = (L - head) / VEC;
                for (uint32_t v = tid; v < nvec; v += kSearchThreads) {
                    const KeyVec<Key> kv = load_keys16(seg + head + v * VEC);
#pragma unroll
                    for (int c = 0; c < VEC; ++c) {
                        stage[head + v * VEC + c] = codec_encode(kv.k[c], ca, cm);
                    }
                }
                const uint32_t body_end = head + nvec * VEC;
                if (tid < head) {
                    stage[tid] = codec_encode(seg[tid], ca, cm);
                } else if (tid >= kWave && body_end + (tid - kWave) < L) {        // (the tail has fewer than VEC keys)
                    stage[body_end + (tid - kWave)] = codec_encode(seg[body_end + (tid - kWave)], ca, cm);
                }
            } else {
#pragma unroll
                for (uint32_t i = tid; i < kSearchSamples; i += kSearchThreads) {
                    const uint32_t p = static_cast<uint32_t>((static_cast<uint64_t>(i) * L) >> kSearchSampleShift);
                    stage[i] = codec_encode(seg[p], ca, cm);
                }
            }
            staged = path;
            staged_seg = s_first;
            __syncthreads();
        }
        if (path == kResident) {
#pragma unroll
            for (int r = 0; r < kSearchQpt; ++r) {
                base[r] = 0;
                len[r] = live[r] ? L : 0u;
            }
            search_bisect(([&](int, uint32_t i) { return stage[i]; }), q, right, base, len);
        } else if (path == kSampled) {
            const Key* seg = keys + hs;
#pragma unroll
            for (int r = 0; r < kSearchQpt; ++r) {
                base[r] = 0;
                len[r] = live[r] ? kSearchSamples : 0u;
            }
            search_bisect(([&](int, uint32_t i) { return stage[i]; }), q, right, base, len);
#pragma unroll
            for (int r = 0; r < kSearchQpt; ++r) {
                const uint32_t c = base[r];                       // samples before q[r]
                const uint32_t lo = c ? static_cast<uint32_t>((static_cast<uint64_t>(c - 1) * L) >> kSearchSampleShift) + 1u : 0u;
                const uint32_t hi = c == 0 ? 0u : c < kSearchSamples ? static_cast<uint32_t>((static_cast<uint64_t>(c) * L) >> kSearchSampleShift) : L;
                base[r] = lo;
                len[r] = live[r] ? hi - lo : 0u;
            }
            search_bisect(([&](int, uint32_t i) { return codec_encode(seg[i], ca, cm); }), q, right, base, len);
        } else {
            const Key* seg[kSearchQpt];
#pragma unroll
            for (int r = 0; r < kSearchQpt; ++r) {
                const uint64_t j = tile_start + tid + static_cast<uint32_t>(r) * kSearchThreads;
                uint64_t s = s_first;
                if (live[r] && s_first != s_last) {
                    s = qoff ? search_segment_of(qoff, s_first, s_last, j) : static_cast<uint32_t>(j) / qper;
                }
                const uint64_t h0 = live[r] ? uniq_off(off, s, n) : 0ull;
                seg[r] = keys + h0;
                base[r] = 0;
                len[r] = live[r] ? static_cast<uint32_t>(uniq_off(off, s + 1, n) - h0) : 0u;
            }
            search_bisect(([&](int r, uint32_t i) { return codec_encode(seg[r][i], ca, cm); }), q, right, base, len);
        }
#pragma unroll
        for (int r = 0; r < kSearchQpt; ++r) {
            const uint64_t j = tile_start + tid + static_cast<uint32_t>(r) * kSearchThreads;
            if (live[r]) {
                out[j] = base[r];
            }
        }
        __syncthreads();                                          // the next tile may restage
    }
}

}  // namespace rsx
