// rsx_setop.hpp — kernels of rsx_segmented_set_op: intersection, difference, union and symmetric difference of sorted segment s of A with
// sorted segment s of B, for every s, with the multiset rule of std::set_* (thrust::set_*_by_key with ragged rows).  A set operation is
// the merge whose outputs pass a predicate: two passes over the keys.  Included by rsx_capi.hip (host side: capi_setop.inc).
//
//   (unique_reset_kernel + unique_validate_kernel, unchanged, once per offsets array: the first bad segment of either, one word)
//   (merge_split_kernel, unchanged: the segment and merge-path split of merged position 4096 t -> split[t]; the report on bad offsets)
//   setop_count_kernel     per tile of 4096 MERGED positions: stages the tile's sources, merges, evaluates the predicate; kept elements
//                          -> flat [tile] table; for every merged offset ooff(s) inside the tile the kept elements of the tile before it
//                          -> koff[s] (tile-local for now): compact_count_kernel's walk
//   (scan_blocks_kernel + paste_scan_kernel, unchanged: the flat exclusive scan of that table)
//   setop_offsets_kernel   unique_offsets_kernel's twin over the merged offsets: koff[s] += table[tile of ooff(s)], capped at the output
//                          size; zeros on bad offsets
//   setop_write_kernel     per tile: the same staging, merge and predicate (setop_tile_bits: ONE function for both passes), ranks the kept
//                          elements (popcount of the thread's 16 keep bits + a block scan), moves their source slot, index and match to
//                          their rank in LDS and stores slots r, r + 256, ... to consecutive addresses.
//
// WHICH ELEMENTS ARE KEPT.  Key x occurs m times in A_s and n times in B_s; occurrence r = 0, 1, ... on each side in input order.
// Intersection: the A occurrences r < n.  Difference: the A occurrences r >= n.  Union: every A occurrence and the B occurrences r >= m.
// Symmetric difference: the A occurrences r >= n and the B occurrences r >= m.  Order: the stable merge's (A before equal B).
//
// THE PROBE RULE.  The serial merge of a thread holds the pointers (i, j) into A_s and B_s.  When it takes A[i] = x: every B key before x
// is taken and no B key equal to x is (A comes first), so B's run of x starts at j; with r = i - (start of x's run in A_s) the element
// has a partner iff j + r < boff[s+1] and B[j + r] == x (HIT).  When it takes B[j] = x: every A key not after x is taken, so A's run of x
// ends at i; with r = j - (start of x's run in B_s): HIT iff i - 1 - r >= aoff[s] and A[i - 1 - r] == x.  Intersection keeps A on a hit,
// difference and symmetric difference keep A on a miss, union keeps every A; union and symmetric difference keep B on a miss.  The match
// output of a kept A element of the intersection is j + r - boff[s].  One probe per merged element; a probe position outside the tile's
// staged range is read from global memory, guarded by the segment's bounds: these are the probes of the first and last
// key value of a tile's range, and nothing depends on their being rare.
//
// RUN STARTS.  A thread carries the start of the run of A[i] and of B[j]: after a step the start moves to the new position iff the key
// changed.  At the first element of a thread's run (one per segment it touches) the start is a bisection over the staged part of the
// side before the pointer; where that reaches the front of the staged range and the segment began before it, the run may reach back
// into earlier tiles: thread 0 (A) and thread 64 (B) find the start of the range's first key once per tile, galloping back in global
// memory from the range's first position (1, 2, 4, ... then a bisection: one load where the predecessor differs).
//
// INPUTS THAT ARE NOT SORTED.  Every position the code forms is clamped or guarded to its segment, so no access leaves the buffers; the
// two passes run the same function on the same data and so agree on every keep bit.  What unsorted keys can break is the COUNT: thread
// paths need not partition the sources then, an A element may be taken twice, and the A-sourced elements may outnumber na.  The offsets
// kernel therefore caps koff at the output size (na for intersection and difference, na + nb otherwise) and the write kernel drops
// destinations at or past the cap: koff stays non-decreasing and exactly [0, koff[S]) is written.  On sorted inputs the cap never acts.
//
// LDS LAYOUT (write kernel).  Staged source e at e + (e >> 4) (compact_slot), as the merge.  Per merged position l: the source slot (16
// bits) at halfword l + 2 (l >> 4) (thread stride 9 words), and with AUX >= 1 the index, with AUX == 2 the match, at compact_slot(l).  After the
// scan a thread takes its 16 entries into registers, a barrier, and the kept ones go back into the SAME arrays at their rank (rank <= l;
// every thread has read its own by then): no second set of arrays.  Bytes, 4- / 8-byte keys: keys only 26 / 43 KiB, + payload 43 / 60,
// + index 60 / 77, + match 77 / 94.  The count kernel holds the staged keys and one word per thread: 18 / 35 KiB.
//
// No atomic decides a destination and no workgroup waits for another: the output is a function of the inputs alone.
#pragma once

#include "rsx_merge.hpp"

namespace rsx {

constexpr uint32_t kSetIntersection = 0u, kSetDifference = 1u, kSetUnion = 2u, kSetSymmetricDifference = 3u;        // RSX_SET_*

// THE PREDICATE, given the probe's answer
__device__ __forceinline__ bool setop_keep(uint32_t op, bool from_a, bool hit)
{
    if (from_a) {
        return op == kSetUnion || (op == kSetIntersection ? hit : !hit);
    }
    return (op == kSetUnion || op == kSetSymmetricDifference) && !hit;
}

// smallest p in [lo, pos] with g[p .. pos) all equal to x, on a sorted g: gallops back from pos, then bisects.  Reads only [lo, pos).
template <typename Key>
__device__ __forceinline__ uint32_t setop_run_start_global(const Key* __restrict__ g, uint32_t lo, uint32_t pos, Key x)
{
    uint32_t hi = pos, step = 1;
    while (hi > lo) {
        const uint32_t probe = hi - lo >= step ? hi - step : lo;
        if (g[probe] == x) {
            hi = probe;
            step <<= 1;
        } else {
            uint32_t l = probe + 1u, h = hi;
            while (l < h) {
                const uint32_t mid = (l + h) >> 1;
                if (g[mid] == x) {
                    h = mid;
                } else {
                    l = mid + 1u;
                }
            }
            return l;
        }
    }
    return hi;
}

template <typename Key, bool PAYLOAD, int AUX, bool WRITE>
struct SetopShared {
    Key skey[kMergeSlots];
    uint32_t spay[(WRITE && PAYLOAD) ? kMergeSlots : 1];
    uint16_t ssrc[WRITE ? kMergeSrcHalves : 2];
    uint32_t sidx[(WRITE && AUX >= 1) ? kMergeSlots : 1];
    uint32_t smatch[(WRITE && AUX >= 2) ? kMergeSlots : 1];
    uint32_t tinfo[WRITE ? 1 : kMergeThreads];
    uint32_t wtot[kMergeThreads / kWave];
    uint32_t run0[2];                                             // the run starts of the staged ranges' first keys (A, B)
};

// what both passes are given
template <typename Key>
struct SetopArgs {
    const Key* ka;
    const uint32_t* pa;
    const Key* kb;
    const uint32_t* pb;
    MergeOffsets o;                                               // (a0 and b0 filled in by the kernel)
    uint64_t nseg;
    Key ca, cm;
    uint32_t op;
    const MergeSplit* split;
};

// One tile of merged positions [p0, p0 + cnt), cnt >= 1: stages the sources, merges, evaluates the predicate.  Returns the thread's keep
// bits (bit k = merged position p0 + 16 tid + k).  WRITE: also leaves per position the source slot and (AUX) index and match in LDS.
// Contains one barrier after the staging; the caller separates the next tile's staging from this one's readers.
template <typename Key, bool PAYLOAD, int AUX, bool WRITE>
__device__ __forceinline__ uint32_t setop_tile_bits(SetopShared<Key, PAYLOAD, AUX, WRITE>& sh, const SetopArgs<Key>& g, uint32_t t, uint32_t p0, uint32_t cnt)
{
    const uint32_t tid = threadIdx.x;
    const MergeOffsets& o = g.o;
    const Key ca = g.ca, cm = g.cm;
    const uint32_t a0 = static_cast<uint32_t>(o.a0), b0 = static_cast<uint32_t>(o.b0);
    const uint32_t p1 = p0 + cnt;
    const MergeSplit sp0 = g.split[t], sp1 = g.split[t + 1];
    // the tile's sources: A[ai0, ai0 + nA) and B[bi0, bi0 + nB), nA + nB = cnt (rsx_merge.hpp)
    const uint32_t ai0 = sp0.a, bi0 = b0 + (p0 - (ai0 - a0));
    const uint32_t nA = sp1.a > ai0 ? min(sp1.a - ai0, cnt) : 0u, nB = cnt - nA;
    const uint32_t ai1 = ai0 + nA, bi1 = bi0 + nB;
    const uint32_t s0 = sp0.s, s_hi = min(sp1.s, static_cast<uint32_t>(g.nseg - 1));
    const bool single = merge_ooff(o, static_cast<uint64_t>(s0) + 1) >= p1;       // (uniform) the tile lies inside segment s0
    merge_stage(g.ka, ai0, nA, sh.skey, 0u, [=](Key k) { return codec_encode(k, ca, cm); });
    merge_stage(g.kb, bi0, nB, sh.skey, nA, [=](Key k) { return codec_encode(k, ca, cm); });
    if constexpr (WRITE && PAYLOAD) {
        merge_stage(g.pa, ai0, nA, sh.spay, 0u, [](uint32_t v) { return v; });
        merge_stage(g.pb, bi0, nB, sh.spay, nA, [](uint32_t v) { return v; });
    }
    // segment s0's ranges (uniform)
    const uint32_t as0 = static_cast<uint32_t>(uniq_off(o.aoff, s0, o.na)), ae0 = static_cast<uint32_t>(uniq_off(o.aoff, static_cast<uint64_t>(s0) + 1, o.na));
    const uint32_t bs0 = static_cast<uint32_t>(uniq_off(o.boff, s0, o.nb)), be0 = static_cast<uint32_t>(uniq_off(o.boff, static_cast<uint64_t>(s0) + 1, o.nb));
    // the run starts of the ranges' first keys, where segment s0 began before the range
    if (tid == 0) {
        sh.run0[0] = nA > 0 && as0 < ai0 && ai0 < ae0 ? setop_run_start_global(g.ka, as0, ai0, g.ka[ai0]) : ai0;
    } else if (tid == kWave) {
        sh.run0[1] = nB > 0 && bs0 < bi0 && bi0 < be0 ? setop_run_start_global(g.kb, bs0, bi0, g.kb[bi0]) : bi0;
    }
    __syncthreads();
    const uint32_t run0a = sh.run0[0], run0b = sh.run0[1];
    uint32_t q = p0 + tid * kMergeKpt;
    const uint32_t q0 = q, qe = min(q + kMergeKpt, p1);
    uint32_t s_from = s0, bits = 0;
#pragma unroll 1
    while (q < qe) {
        // the run's segment and its staged parts A' = [la, la + na) and B' = [lb, lb + nb) (slots before the skew): as merge_kernel
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
        const uint32_t first = max((as - a0) + (bs - b0), p0);                  // the segment's first merged position inside the tile
        const uint32_t r0 = min(q - first, na + nb);
        uint32_t i = merge_diagonal([&](uint32_t m) { return sh.skey[compact_slot(la + m)]; }, [&](uint32_t m) { return sh.skey[compact_slot(lb + m)]; },
                                    na, nb, r0);
        uint32_t j = r0 - i;
        const uint32_t run = max(min(qe - q, na + nb - r0), 1u);
        Key xa = i < na ? sh.skey[compact_slot(la + i)] : Key{0};
        Key xb = j < nb ? sh.skey[compact_slot(lb + j)] : Key{0};
        // the starts (global positions) of the runs of A[i] and B[j]: the first staged key of the side before the pointer that is not before it
        uint32_t ra = a_lo + i, rb = b_lo + j;
        if (i < na) {
            uint32_t lo = 0, hi = i;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (sh.skey[compact_slot(la + mid)] < xa) {
                    lo = mid + 1u;
                } else {
                    hi = mid;
                }
            }
            ra = lo == 0 && a_lo > as ? run0a : a_lo + lo;
        }
        if (j < nb) {
            uint32_t lo = 0, hi = j;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (sh.skey[compact_slot(lb + mid)] < xb) {
                    lo = mid + 1u;
                } else {
                    hi = mid;
                }
            }
            rb = lo == 0 && b_lo > bs ? run0b : b_lo + lo;
        }
        // one merged position: selects, not branches, but for the rare probe outside the staged range
        auto step = [&](uint32_t k) {
            const bool take_a = j >= nb || (i < na && xa <= xb);
            const Key x = take_a ? xa : xb;
            const uint32_t src = min(take_a ? la + i : lb + j, cnt - 1u);
            const uint32_t ga = a_lo + i, gb = b_lo + j;          // the pointers as global positions
            const uint32_t probe = take_a ? gb + (ga - ra) : ga - 1u - (gb - rb);
            const bool inseg = probe >= (take_a ? bs : as) && probe < (take_a ? be : ae);
            const uint32_t pl = probe - (take_a ? bi0 : ai0);     // the probe inside the other side's staged range, if below its length
            Key pk = sh.skey[compact_slot(min((take_a ? nA : 0u) + pl, cnt - 1u))];
            if (inseg && pl >= (take_a ? nB : nA)) {
                pk = codec_encode((take_a ? g.kb : g.ka)[probe], ca, cm);
            }
            const bool hit = inseg && pk == x;
            const uint32_t l = q + k - p0;
            bits |= setop_keep(g.op, take_a, hit) ? 1u << (q + k - q0) : 0u;
            if constexpr (WRITE) {
                sh.ssrc[l + 2u * (l >> 4)] = static_cast<uint16_t>(src);
                if constexpr (AUX >= 1) {
                    sh.sidx[compact_slot(l)] = take_a ? ga - as : (ae - as) + (gb - bs);
                }
                if constexpr (AUX >= 2) {
                    sh.smatch[compact_slot(l)] = probe - bs;
                }
            }
            i += take_a ? 1u : 0u;
            j += take_a ? 0u : 1u;
            // the next key of that side (unused once the side is exhausted); its run starts here iff it differs
            const Key nx = sh.skey[compact_slot(min(take_a ? la + i : lb + j, cnt - 1u))];
            ra = take_a && nx != x ? a_lo + i : ra;
            rb = !take_a && nx != x ? b_lo + j : rb;
            xa = take_a ? nx : xa;
            xb = take_a ? xb : nx;
        };
        if (run == kMergeKpt) {                                   // the thread's 16 positions lie in one segment: unrolled
#pragma unroll
            for (uint32_t k = 0; k < kMergeKpt; ++k) {
                step(k);
            }
        } else {
#pragma unroll 1
            for (uint32_t k = 0; k < run; ++k) {
                step(k);
            }
        }
        q += run;
        s_from = min(s + 1u, s_hi);
    }
    return bits;
}

// first s in [0, nseg] with ooff(s) >= x, nseg + 1 if there is none
__device__ __forceinline__ uint64_t setop_ooff_lower_bound(const MergeOffsets& o, uint64_t nseg, uint64_t x)
{
    uint64_t lo = 0, hi = nseg + 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (merge_ooff(o, mid) < x) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// Workgroup b counts the tiles [b * chunk, (b + 1) * chunk) of a table of `ntab` = tiles + 1 entries padded with zeros to `npad`
// (compact_count_kernel's table: the extra tile is empty and gives ooff(s) == total a tile when the total is a multiple of 4096).
template <typename Key>
__global__ __launch_bounds__(kMergeThreads) void setop_count_kernel(SetopArgs<Key> g, const uint32_t* __restrict__ bad, uint32_t* __restrict__ table,
                                                                    uint32_t ntab, uint32_t npad, uint32_t chunk, uint64_t* __restrict__ koff)
{
    __shared__ SetopShared<Key, false, 0, false> sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, npad);
    if (*bad != kUniqNoBad) {
        for (uint32_t t = t0 + tid; t < t1; t += kMergeThreads) {
            table[t] = 0;
        }
        return;
    }
    g.o.a0 = uniq_off(g.o.aoff, 0, g.o.na);
    g.o.b0 = uniq_off(g.o.boff, 0, g.o.nb);
    const uint64_t total = merge_ooff(g.o, g.nseg);
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        if (t >= ntab) {
            if (tid == 0) {
                table[t] = 0;
            }
            continue;
        }
        const uint64_t tile_start = static_cast<uint64_t>(t) << kMergeTileShift;
        uint32_t kbits = 0;
        if (tile_start < total) {                                 // (uniform; t < ntab - 1 here: the split has its two boundaries)
            const uint32_t p0 = static_cast<uint32_t>(tile_start);
            kbits = setop_tile_bits(sh, g, t, p0, static_cast<uint32_t>(min(total - tile_start, static_cast<uint64_t>(kMergeTileKeys))));
        }
        uint32_t kept;
        const uint32_t before = block_exclusive_scan<kMergeThreads, false>(static_cast<uint32_t>(__popc(kbits)), sh.wtot, kept);
        sh.tinfo[tid] = (before << 16) | kbits;
        if (tid == 0) {
            table[t] = kept;
        }
        __syncthreads();
        // every ooff(s) inside the tile (empty segments and ooff(S) too): the kept elements of the tile before it
        for (uint64_t s = setop_ooff_lower_bound(g.o, g.nseg, tile_start) + tid; s <= g.nseg; s += kMergeThreads) {
            const uint64_t x = merge_ooff(g.o, s);
            if (x >= tile_start + kMergeTileKeys) break;
            const uint32_t l = static_cast<uint32_t>(x - tile_start);
            const uint32_t ti = sh.tinfo[l >> 4];
            koff[s] = (ti >> 16) + static_cast<uint32_t>(__popc(ti & ((1u << (l & 15u)) - 1u)));
        }
        __syncthreads();                                          // the next tile stages and scans again
    }
}

// koff[s] = kept elements before merged offset ooff(s): the scanned table entry of its tile + the tile-local count, capped at the output
// size (which only inputs that are not sorted can reach).  With bad offsets every entry is 0 (the split kernel has reported).
__global__ __launch_bounds__(kUniqSmallThreads) void setop_offsets_kernel(MergeOffsets o, uint64_t nseg, const uint32_t* __restrict__ bad,
                                                                           const uint32_t* __restrict__ table, uint64_t cap, uint64_t* __restrict__ koff)
{
    const uint32_t b = *bad;
    if (b == kUniqNoBad) {
        o.a0 = uniq_off(o.aoff, 0, o.na);
        o.b0 = uniq_off(o.boff, 0, o.nb);
    }
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kUniqSmallThreads;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kUniqSmallThreads + threadIdx.x; s <= nseg; s += stride) {
        koff[s] = b != kUniqNoBad ? 0ull : min(table[merge_ooff(o, s) >> kMergeTileShift] + koff[s], cap);
    }
}

// kout / pout / iout / mout: NULL to skip (not all: the host does not launch then).  PAYLOAD: pout.  AUX: 0 neither iout nor mout, 1 iout
// at most, 2 mout (and iout if given).  `table` is scanned; destinations at or past `cap` are dropped (the offsets kernel's cap).
template <typename Key, bool PAYLOAD, int AUX>
__global__ __launch_bounds__(kMergeThreads) void setop_write_kernel(SetopArgs<Key> g, const uint32_t* __restrict__ bad, const uint32_t* __restrict__ table,
                                                                    uint32_t ntiles, uint32_t chunk, uint32_t cap, Key* __restrict__ kout,
                                                                    uint32_t* __restrict__ pout, uint32_t* __restrict__ iout, uint32_t* __restrict__ mout)
{
    __shared__ SetopShared<Key, PAYLOAD, AUX, true> sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    g.o.a0 = uniq_off(g.o.aoff, 0, g.o.na);
    g.o.b0 = uniq_off(g.o.boff, 0, g.o.nb);
    const uint32_t total = static_cast<uint32_t>(merge_ooff(g.o, g.nseg));
    const Key ca = g.ca, cm = g.cm;
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t p0 = t << kMergeTileShift;
        if (p0 >= total) break;                                   // (uniform) the tiles behind the total are dead
        const uint32_t tbase = table[t];
        const uint32_t kbits = setop_tile_bits(sh, g, t, p0, min(total - p0, kMergeTileKeys));
        // the thread's own 16 entries, then (after the scan's barrier: every thread has read) back at their rank
        uint32_t src[kMergeKpt], idx[AUX >= 1 ? kMergeKpt : 1], mat[AUX >= 2 ? kMergeKpt : 1];
#pragma unroll
        for (uint32_t k = 0; k < kMergeKpt; ++k) {
            const uint32_t l = tid * kMergeKpt + k;
            src[k] = sh.ssrc[l + 2u * (l >> 4)];
            if constexpr (AUX >= 1) {
                idx[k] = sh.sidx[compact_slot(l)];
            }
            if constexpr (AUX >= 2) {
                mat[k] = sh.smatch[compact_slot(l)];
            }
        }
        uint32_t kept;
        const uint32_t before = block_exclusive_scan<kMergeThreads>(static_cast<uint32_t>(__popc(kbits)), sh.wtot, kept);
#pragma unroll
        for (uint32_t k = 0; k < kMergeKpt; ++k) {
            if (((kbits >> k) & 1u) != 0) {
                const uint32_t r = before + static_cast<uint32_t>(__popc(kbits & ((1u << k) - 1u)));
                sh.ssrc[r + 2u * (r >> 4)] = static_cast<uint16_t>(src[k]);
                if constexpr (AUX >= 1) {
                    sh.sidx[compact_slot(r)] = idx[k];
                }
                if constexpr (AUX >= 2) {
                    sh.smatch[compact_slot(r)] = mat[k];
                }
            }
        }
        __syncthreads();
        // the copy-out: consecutive threads, consecutive addresses
        for (uint32_t r = tid; r < kept; r += kMergeThreads) {
            const uint32_t d = tbase + r;
            if (d >= cap) break;
            const uint32_t slot = compact_slot(sh.ssrc[r + 2u * (r >> 4)]);
            if (kout) {
                kout[d] = codec_decode(sh.skey[slot], ca, cm);
            }
            if constexpr (PAYLOAD) {
                pout[d] = sh.spay[slot];
            }
            if constexpr (AUX >= 1) {
                if (iout) {
                    iout[d] = sh.sidx[compact_slot(r)];
                }
            }
            if constexpr (AUX >= 2) {
                mout[d] = sh.smatch[compact_slot(r)];
            }
        }
        __syncthreads();                                          // the next tile stages again
    }
}

}  // namespace rsx
