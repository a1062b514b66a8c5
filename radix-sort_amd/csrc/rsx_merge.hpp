// rsx_merge.hpp — kernels of rsx_segmented_merge: the stable merge of sorted segment s of A with sorted segment s of B, for every s, in one
// pass over the keys (std::merge, thrust::merge / merge_by_key, cub::DeviceMerge, with ragged rows).  Included by rsx_capi.hip (host side:
// capi_merge.inc).
//
//   (unique_reset_kernel + unique_validate_kernel, unchanged, once per offsets array: the first bad segment of either, one word)
//   merge_split_kernel   one thread per tile boundary: the segment and the merge-path split of output position 4096 t -> split[t];
//                        the same launch writes d_out_offsets and, on bad offsets, zeros there and the report to the status word
//   merge_kernel         per tile of 4096 OUTPUT positions: stages the tile's sources in LDS, every thread merges its 16 positions there,
//                        and the tile leaves as consecutive addresses
//
// THE ORDER.  Keys are compared as plain unsigned numbers after codec_encode with the engine's (A, M) (rsx_common.hpp), the map the sort
// itself uses.  Keys are staged encoded and decoded as they leave (the codec is a bijection: key bits are unchanged).
//
// OUTPUT OFFSETS.  ooff(s) = (aoff[s] - aoff[0]) + (boff[s] - boff[0]), formed on the fly from the two offsets arrays; ooff(S) is the total.
// THE SEGMENT OF OUTPUT POSITION p < ooff(S) is the largest s with ooff(s) <= p (the one with ooff(s) <= p < ooff(s+1): empty segments are
// skipped), found by bisection over s.
//
// THE SPLIT RULE.  In segment s with La keys of A and Lb of B, the first d outputs are A_s[0, i) and B_s[0, d - i) with
//     i = the partition point over [max(0, d - Lb), min(d, La)] of   m  ->  enc(A_s[m]) <= enc(B_s[d - 1 - m])
// found by the bisection (lo, hi) -> pred(mid = (lo + hi) / 2) ? (mid + 1, hi) : (lo, mid).  THE TIE RULE is the <=: an A key comes before
// every B key equal to it.  Every index the bisection forms lies inside the two segments whatever the keys are: on inputs that are not
// sorted the split is unspecified but in range.  split[t] = (s, aoff[s] + i) for p = 4096 t < ooff(S) and (S, aoff[S]) from the total on;
// the B position follows: boff[0] + p - (A position - aoff[0]).  (Measured and rejected for the split kernel: a wave per boundary with 64
// probes a round.  Five rounds where the bisection makes 27, but twelve times the scattered loads: the call went from 0.63 to 0.97 ms
// on 2^27 + 2^27 uint32 keys.)
//
// THE SOURCES OF A TILE.  A's segments follow each other without gaps, and so do B's: the sources of tile t are the contiguous ranges
// A[split[t].a, split[t+1].a) and the matching range of B, kUniqTileKeys keys together, however many segments the tile spans.  (Where both
// boundaries lie in one segment and the keys are not sorted the second split may lie before the first: the A count is clamped to
// [0, the tile's outputs], so that the ranges stay inside the buffers and hold exactly the tile's outputs.)  Both ranges are staged in LDS,
// A first, B behind it: 16-byte loads over the part of a range that is 16-byte aligned, element loads for the head before and the tail
// after; the payload words beside them.  Inside the tile, segment s owns the staged parts A' = A_s cut to the tile's A range and B' likewise,
// and its outputs inside the tile are the merge of A' and B' (|A'| + |B'| of them).
//
// THREAD PATHS.  Thread q owns the 16 consecutive output positions 4096 t + 16 q ...  It walks them in RUNS: a run is the part of its 16
// that lies in one segment.  Per run: the segment (none to find when the whole tile lies in one segment — that is uniform; a bisection
// between the tile's first and last segment otherwise), the split rule over (A', B') in LDS at the run's first rank, then a serial merge
// of the run's positions, one LDS read per step.  A thread whose 16 positions lie in one segment is SERIAL (one search, 16 steps, unrolled
// and without a branch); one with a segment boundary among its 16 is PER-RUN (a search per segment it touches, up to 16).  Each step
// leaves the staged slot of its source (16 bits) in LDS at the output's place; after a barrier the tile is copied out by consecutive
// threads to consecutive addresses: key = decode(staged[src]), payload = staged payload[src].  The index (position in A_s ++ B_s) is computed from the source position: in
// a tile inside one segment at the copy-out (uniform segment data, no LDS); in a tile that spans segments by the thread that merged the
// element, which knows its segment, stored from there.
//
// LDS LAYOUT.  Staged element e lives at e + (e >> 4) (compact_slot).  Threads start their serial merges 16 outputs apart: when one side
// supplies (nearly) everything, the 32 lanes of a half wave read sources 16 apart: without the skew two banks, with it 17 words apart:
// all banks (8-byte keys: 34 words, every second bank twice).  The 16-bit source slots of output r live at halfword r + 2 (r >> 4): thread
// stride 9 words, all banks.  Static LDS: 4352 keys + 9 KiB (26 KiB / 43 KiB), with payload 4352 words more (43 KiB / 60 KiB).
//
// No atomics, no cross-lane operation, no workgroup waits for another: the output is a function of the inputs alone.  One instantiation
// per key width, with and without payload; key kind and direction are the two codec constants among the arguments.
#pragma once

#include "rsx_compact.hpp"

namespace rsx {

constexpr int kMergeThreads = kUniqThreads, kMergeKpt = kUniqKpt;
constexpr int kMergeTileShift = kUniqTileShift;
constexpr uint32_t kMergeTileKeys = kUniqTileKeys;              // output positions of a tile = kMergeThreads * kMergeKpt
constexpr uint32_t kMergeSlots = kCompactSlots;                 // staged elements, skewed by one per 16
constexpr uint32_t kMergeSrcHalves = kMergeTileKeys + 2 * (kMergeTileKeys / 16);
constexpr int kMergeSplitThreads = 256;
static_assert(kMergeTileKeys == kMergeThreads * kMergeKpt, "a thread owns kMergeKpt output positions of a tile");

// one boundary of the tile grid: the segment of output position 4096 t and the A position of its merge-path split
struct MergeSplit {
    uint32_t s, a;
};

// the two offsets arrays (both NULL: one segment [0, na), [0, nb)) and their first entries
struct MergeOffsets {
    const uint64_t* aoff;
    const uint64_t* boff;
    uint64_t na, nb, a0, b0;
};

__device__ __forceinline__ uint64_t merge_ooff(const MergeOffsets& o, uint64_t s)
{
    return (uniq_off(o.aoff, s, o.na) - o.a0) + (uniq_off(o.boff, s, o.nb) - o.b0);
}

// largest s in [lo, hi] with ooff(s) <= p (ooff(lo) <= p is the caller's)
__device__ __forceinline__ uint64_t merge_segment_of(const MergeOffsets& o, uint64_t lo, uint64_t hi, uint64_t p)
{
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (merge_ooff(o, mid) <= p) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return lo;
}

// THE SPLIT RULE: a(m) / b(m) = the encoded key m of the A / B range (na / nb keys), d <= na + nb the diagonal
template <typename AtA, typename AtB>
__device__ __forceinline__ uint32_t merge_diagonal(AtA&& a, AtB&& b, uint32_t na, uint32_t nb, uint32_t d)
{
    uint32_t lo = d > nb ? d - nb : 0u, hi = min(d, na);
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a(mid) <= b(d - 1u - mid)) {
            lo = mid + 1u;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// Boundary t of the tile grid, t = 0 .. ntiles; and out_offsets[s], s = 0 .. nseg.  On bad offsets: zeros and the report, no split.
template <typename Key>
__global__ __launch_bounds__(kMergeSplitThreads) void merge_split_kernel(const Key* __restrict__ ka, const Key* __restrict__ kb, MergeOffsets o,
                                                                         uint64_t nseg, Key ca, Key cm, const uint32_t* __restrict__ bad,
                                                                         uint32_t* status_host, uint32_t call_id, uint32_t ntiles,
                                                                         MergeSplit* __restrict__ split, uint64_t* __restrict__ ooff_out)
{
    const uint32_t b = *bad;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kMergeSplitThreads;
    const uint64_t first = static_cast<uint64_t>(blockIdx.x) * kMergeSplitThreads + threadIdx.x;
    if (b != kUniqNoBad) {
        if (ooff_out) {
            for (uint64_t s = first; s <= nseg; s += stride) {
                ooff_out[s] = 0ull;
            }
        }
        if (first == 0 && __hip_atomic_load(status_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
            __hip_atomic_store(status_host + 1, call_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(status_host, b + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);        // (after the call's id)
        }
        return;
    }
    o.a0 = uniq_off(o.aoff, 0, o.na);
    o.b0 = uniq_off(o.boff, 0, o.nb);
    if (ooff_out) {
        for (uint64_t s = first; s <= nseg; s += stride) {
            ooff_out[s] = merge_ooff(o, s);
        }
    }
    const uint64_t total = merge_ooff(o, nseg);
    for (uint64_t t = first; t <= ntiles; t += stride) {
        const uint64_t p = t << kMergeTileShift;
        MergeSplit sp;
        if (p >= total) {
            sp.s = static_cast<uint32_t>(nseg);
            sp.a = static_cast<uint32_t>(uniq_off(o.aoff, nseg, o.na));
        } else {
            const uint64_t s = merge_segment_of(o, 0, nseg - 1, p);
            const uint64_t as = uniq_off(o.aoff, s, o.na), bs = uniq_off(o.boff, s, o.nb);
            const uint32_t la = static_cast<uint32_t>(uniq_off(o.aoff, s + 1, o.na) - as), lb = static_cast<uint32_t>(uniq_off(o.boff, s + 1, o.nb) - bs);
            const uint32_t d = static_cast<uint32_t>(p - ((as - o.a0) + (bs - o.b0)));
            const Key* sa = ka + as;
            const Key* sb = kb + bs;
            const uint32_t i = merge_diagonal([&](uint32_t m) { return codec_encode(sa[m], ca, cm); }, [&](uint32_t m) { return codec_encode(sb[m], ca, cm); },
                                              la, lb, d);
            sp.s = static_cast<uint32_t>(s);
            sp.a = static_cast<uint32_t>(as) + i;
        }
        split[t] = sp;
    }
}

template <typename Key, bool PAYLOAD>
struct MergeShared {
    Key skey[kMergeSlots];
    uint32_t spay[PAYLOAD ? kMergeSlots : 1];
    uint16_t ssrc[kMergeSrcHalves];
};

// g[start, start + count) -> lds[compact_slot(lbase + i)] = f(g[start + i]): 16-byte loads over the aligned middle, element loads at the ends
template <typename T, typename F>
__device__ __forceinline__ void merge_stage(const T* __restrict__ g, uint64_t start, uint32_t count, T* lds, uint32_t lbase, F&& f)
{
    constexpr uint32_t VEC = 16 / sizeof(T);
    const uint32_t tid = threadIdx.x;
    const T* src = g + start;
    const uint32_t mis = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(src) & 15u) / sizeof(T));
    const uint32_t head = min(mis ? VEC - mis : 0u, count);
    const uint32_t nvec = (count - head) / VEC;
    for (uint32_t v = tid; v < nvec; v += kMergeThreads) {
        const KeyVec<T> kv = load_keys16(src + head + v * VEC);
#pragma unroll
        for (uint32_t c = 0; c < VEC; ++c) {
            lds[compact_slot(lbase + head + v * VEC + c)] = f(kv.k[c]);
        }
    }
    const uint32_t body_end = head + nvec * VEC;
    if (tid < head) {
        lds[compact_slot(lbase + tid)] = f(src[tid]);
    } else if (tid >= kWave && body_end + (tid - kWave) < count) {          // (the tail has fewer than VEC elements)
        lds[compact_slot(lbase + body_end + (tid - kWave))] = f(src[body_end + (tid - kWave)]);
    }
}

// pa / pb / pout: the payloads (PAYLOAD).  kout / pout / iout: NULL to skip (not all: the host does not launch then).
template <typename Key, bool PAYLOAD>
__global__ __launch_bounds__(kMergeThreads) void merge_kernel(const Key* __restrict__ ka, const uint32_t* __restrict__ pa, const Key* __restrict__ kb,
                                                              const uint32_t* __restrict__ pb, MergeOffsets o, uint64_t nseg, Key ca, Key cm,
                                                              const uint32_t* __restrict__ bad, const MergeSplit* __restrict__ split,
                                                              uint32_t ntiles, uint32_t chunk, Key* __restrict__ kout, uint32_t* __restrict__ pout,
                                                              uint32_t* __restrict__ iout)
{
    __shared__ MergeShared<Key, PAYLOAD> sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    o.a0 = uniq_off(o.aoff, 0, o.na);
    o.b0 = uniq_off(o.boff, 0, o.nb);
    const uint32_t total = static_cast<uint32_t>(merge_ooff(o, nseg));
    const uint32_t a0 = static_cast<uint32_t>(o.a0), b0 = static_cast<uint32_t>(o.b0);
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t p0 = t << kMergeTileShift;
        if (p0 >= total) break;                                   // (uniform) the tiles behind the total are dead
        const uint32_t p1 = min(p0 + kMergeTileKeys, total), cnt = p1 - p0;
        const MergeSplit sp0 = split[t], sp1 = split[t + 1];
        // the tile's sources: A[ai0, ai0 + nA) and B[bi0, bi0 + nB), nA + nB = cnt
        const uint32_t ai0 = sp0.a, bi0 = b0 + (p0 - (ai0 - a0));
        const uint32_t nA = sp1.a > ai0 ? min(sp1.a - ai0, cnt) : 0u, nB = cnt - nA;
        const uint32_t ai1 = ai0 + nA, bi1 = bi0 + nB;
        const uint32_t s0 = sp0.s, s_hi = min(sp1.s, static_cast<uint32_t>(nseg - 1));
        const bool single = merge_ooff(o, static_cast<uint64_t>(s0) + 1) >= p1;       // (uniform) the tile lies inside segment s0
        merge_stage(ka, ai0, nA, sh.skey, 0u, [=](Key k) { return codec_encode(k, ca, cm); });
        merge_stage(kb, bi0, nB, sh.skey, nA, [=](Key k) { return codec_encode(k, ca, cm); });
        if constexpr (PAYLOAD) {
            merge_stage(pa, ai0, nA, sh.spay, 0u, [](uint32_t v) { return v; });
            merge_stage(pb, bi0, nB, sh.spay, nA, [](uint32_t v) { return v; });
        }
        __syncthreads();
        // segment s0's ranges (uniform): all a tile inside one segment needs
        const uint32_t as0 = static_cast<uint32_t>(uniq_off(o.aoff, s0, o.na)), ae0 = static_cast<uint32_t>(uniq_off(o.aoff, static_cast<uint64_t>(s0) + 1, o.na));
        const uint32_t bs0 = static_cast<uint32_t>(uniq_off(o.boff, s0, o.nb)), be0 = static_cast<uint32_t>(uniq_off(o.boff, static_cast<uint64_t>(s0) + 1, o.nb));
        uint32_t q = p0 + tid * kMergeKpt;
        const uint32_t qe = min(q + kMergeKpt, p1);
        uint32_t s_from = s0;
#pragma unroll 1
        while (q < qe) {
            // the run's segment and its staged parts A' = [la, la + na) and B' = [lb, lb + nb) (slots before the skew)
            uint32_t s = s0, as = as0, ae = ae0, bs = bs0, be = be0;
            if (!single) {
                s = static_cast<uint32_t>(merge_segment_of(o, s_from, s_hi, q));
                as = static_cast<uint32_t>(uniq_off(o.aoff, s, o.na));
                ae = static_cast<uint32_t>(uniq_off(o.aoff, static_cast<uint64_t>(s) + 1, o.na));
                bs = static_cast<uint32_t>(uniq_off(o.boff, s, o.nb));
                be = static_cast<uint32_t>(uniq_off(o.boff, static_cast<uint64_t>(s) + 1, o.nb));
            }
            const uint32_t a_lo = max(as, ai0), a_hi = max(min(ae, ai1), a_lo), b_lo = max(bs, bi0), b_hi = max(min(be, bi1), b_lo);
            const uint32_t la = a_lo - ai0, na = a_hi - a_lo, lb = nA + (b_lo - bi0), nb = b_hi - b_lo;
            const uint32_t first = max((as - a0) + (bs - b0), p0);                  // the segment's first output inside the tile
            const uint32_t r = min(q - first, na + nb);                             // (q - first < na + nb on valid splits)
            uint32_t i = merge_diagonal([&](uint32_t m) { return sh.skey[compact_slot(la + m)]; }, [&](uint32_t m) { return sh.skey[compact_slot(lb + m)]; },
                                        na, nb, r);
            uint32_t j = r - i;
            const uint32_t run = max(min(qe - q, na + nb - r), 1u);
            Key xa = i < na ? sh.skey[compact_slot(la + i)] : Key{0};
            Key xb = j < nb ? sh.skey[compact_slot(lb + j)] : Key{0};
            if (run == kMergeKpt) {
                // SERIAL: the thread's 16 positions, unrolled and without a branch; two source slots leave as one word (q - p0 = 16 tid)
                u32_alias* pair = reinterpret_cast<u32_alias*>(sh.ssrc) + (((q - p0) + 2u * ((q - p0) >> 4)) >> 1);
                uint32_t even = 0;
#pragma unroll
                for (uint32_t k = 0; k < kMergeKpt; ++k) {
                    const bool take_a = j >= nb || (i < na && xa <= xb);
                    const uint32_t src = take_a ? la + i : lb + j;                  // (below cnt: 16 elements are left)
                    if (iout && !single) {
                        iout[q + k] = take_a ? (a_lo + i) - as : (ae - as) + (b_lo + j) - bs;
                    }
                    if (k & 1u) {
                        pair[k >> 1] = even | (src << 16);
                    } else {
                        even = src;
                    }
                    i += take_a ? 1u : 0u;
                    j += take_a ? 0u : 1u;
                    const Key x = sh.skey[compact_slot(min(take_a ? la + i : lb + j, cnt - 1u))];      // the next of that side (unused past its end)
                    xa = take_a ? x : xa;
                    xb = take_a ? xb : x;
                }
                break;
            }
#pragma unroll 1
            for (uint32_t k = 0; k < run; ++k) {
                const bool take_a = j >= nb || (i < na && xa <= xb);
                const uint32_t src = take_a ? la + i : lb + j;
                const uint32_t l = q + k - p0;
                sh.ssrc[l + 2u * (l >> 4)] = static_cast<uint16_t>(min(src, cnt - 1u));
                if (iout && !single) {
                    iout[q + k] = take_a ? (a_lo + i) - as : (ae - as) + (b_lo + j) - bs;
                }
                if (take_a) {
                    ++i;
                    xa = i < na ? sh.skey[compact_slot(la + i)] : Key{0};
                } else {
                    ++j;
                    xb = j < nb ? sh.skey[compact_slot(lb + j)] : Key{0};
                }
            }
            q += run;
            s_from = min(s + 1u, s_hi);
        }
        __syncthreads();
        // the copy-out: consecutive threads, consecutive addresses
        for (uint32_t r = tid; r < cnt; r += kMergeThreads) {
            const uint32_t src = sh.ssrc[r + 2u * (r >> 4)];
            const uint32_t slot = compact_slot(src);
            if (kout) {
                kout[p0 + r] = codec_decode(sh.skey[slot], ca, cm);
            }
            if constexpr (PAYLOAD) {
                pout[p0 + r] = sh.spay[slot];
            }
            if (iout && single) {
                iout[p0 + r] = src < nA ? (ai0 + src) - as0 : (ae0 - as0) + (bi0 + (src - nA)) - bs0;
            }
        }
        __syncthreads();                                          // the next tile stages again
    }
}

}  // namespace rsx
