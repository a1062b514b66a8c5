// rsx_expand.hpp — kernels of rsx_segmented_expand: from offsets back to elements.  For every position i of [off[0], off[S]) the segment
// s(i) that owns it (the largest s with off[s] <= i), its rank i - off[s(i)] and a value: d_values[s(i)] (fill form) or
// d_values[starts[s(i)] + rank] (gather form).  Included by rsx_kernels.hpp (host side: capi_expand.inc).
//
//   (unique_reset_kernel + unique_validate_kernel, unchanged: the first bad segment of the offsets, one word)
//   expand_starts_kernel   gather form: per segment starts[s] + len_s > num_values -> the same word
//   expand_split_kernel    one thread per boundary t of the ABSOLUTE grid of 4096 output positions: split[t] = the number of offsets below
//                          4096 * t (a bisection; rsx_expand_math.hpp).  The segments that start inside tile t are [split[t], split[t+1]),
//                          and split[t] is the owner + 1 that the tile inherits.  Reports bad input and leaves.
//   expand_tile_kernel     per tile.  No start inside the tile: one owner, a pure fill.  Else the workgroup walks the offsets
//                          [split[t], split[t+1]), 1024 per trip (four loads in flight per thread), as often as it takes (empty
//                          segments are unbounded: such a tile is slow but correct), and marks slot off[s] - tile_start of a 4096-slot LDS array with s + 1 by an LDS max: of equal
//                          offsets the last segment wins, in whatever order the lanes arrive.  An inclusive max-scan over the slots (16 per
//                          thread, the wave level by DPP as wave_inclusive_scan does for sums, the four wave totals through LDS) turns the
//                          marks into owner + 1 per slot; the rank is 0 at a mark and counts up behind it, so it costs one load of off[]
//                          per thread, not per element.  Owners and ranks go back to LDS, and each output is then stored from there
//                          lane-contiguously: 16-byte stores over the aligned body of the tile's part of [off[0], off[S]), element stores
//                          at its ragged ends (rsx_expand_math.hpp: tile_stores).  The outputs need no common alignment.
//
// The tile grid is absolute (position 4096 * t of the output buffers, not of [off[0], ...)), so the 16-byte body of a tile starts within 3
// elements of the tile's base whatever off[0] is.  Grids come from n and S alone; nothing is read back; no global atomic on the value path
// (the checks use atomicMin on the first-bad-segment word, as unique_validate_kernel does): the output is a function of the inputs alone.
// Which of the segment and rank outputs exist is a kernel ARGUMENT (a null pointer, wave-uniform), not a template parameter: the branch
// is uniform and free next to the stores, and the instantiations stay at four (4 and 8 bytes x fill and gather; without values the
// 4-byte fill kernel runs).
#pragma once

#include "rsx_expand_math.hpp"
#include "rsx_unique.hpp"

namespace rsx {

constexpr int kExpandThreads = 256, kExpandPerThread = 16;        // one tile = 256 x 16 slots; thread q scans slots 16q .. 16q+15
constexpr int kExpandSmallThreads = 256;
static_assert(kExpandThreads * kExpandPerThread == static_cast<int>(rsx_expand::kTileSlots), "one tile is 4096 slots");

// Inclusive running maximum across the 64 lanes of a wave: wave_inclusive_scan's DPP steps with max for +.  An absent source lane reads
// as 0, which is the identity of the unsigned maximum as it is of the sum.
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t v)
{
    v = max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x111, 0xf, 0xf, false)));
    v = max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x112, 0xf, 0xf, false)));
    v = max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x114, 0xf, 0xf, false)));
    v = max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x118, 0xf, 0xf, false)));
    v = max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x142, 0xa, 0xf, false)));
    v = max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x143, 0xc, 0xf, false)));
    return v;
}

// gather form: a segment that would read past the end of d_values is bad input, into the word that the offsets check fills
__global__ __launch_bounds__(kExpandSmallThreads) void expand_starts_kernel(const uint64_t* __restrict__ off, const uint64_t* __restrict__ starts,
                                                                           uint64_t nseg, uint64_t num_values, uint32_t* __restrict__ bad)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kExpandSmallThreads;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kExpandSmallThreads + threadIdx.x; s < nseg; s += stride) {
        const uint64_t a = off[s], b = off[s + 1], st = starts[s];
        if (b >= a && (st > num_values || b - a > num_values - st)) {       // (b < a: the offsets check reports it)
            atomicMin(bad, static_cast<uint32_t>(s));
        }
    }
}

// split[t] for t in [0, ntiles]; with bad input the first bad segment + 1 goes to the mapped host words with the call's id, unless an
// earlier report is still pending there (as segreduce_join_kernel does), and nothing else happens in this call
__global__ __launch_bounds__(kExpandSmallThreads) void expand_split_kernel(const uint64_t* __restrict__ off, uint64_t nseg, const uint32_t* __restrict__ bad,
                                                                          uint32_t ntiles, uint32_t* __restrict__ split, uint32_t* status_host,
                                                                          uint32_t call_id)
{
    const uint32_t b = *bad;
    if (b != kUniqNoBad) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && __hip_atomic_load(status_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
            __hip_atomic_store(status_host + 1, call_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(status_host, b + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);        // (after the call's id)
        }
        return;
    }
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kExpandSmallThreads;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kExpandSmallThreads + threadIdx.x; t <= ntiles; t += stride) {
        split[t] = static_cast<uint32_t>(rsx_expand::tile_split(off, nseg, t));      // <= S + 1 < 2^32
    }
}

// LDS of the tile kernel: owner + 1 and rank of every slot, the scan's wave totals
struct alignas(16) ExpandShared {
    uint32_t own[rsx_expand::kTileSlots];
    uint32_t rank[rsx_expand::kTileSlots];
    uint32_t wtot[kExpandThreads / kWave];
};

template <typename T>
struct alignas(16) ExpandVec {
    T x[16 / sizeof(T)];
};

// out[i] = f(i) for i in [a, b): element stores up to the first 16-byte boundary of `out`, 16-byte stores, element stores
template <typename T, typename F>
__device__ __forceinline__ void expand_emit(T* __restrict__ out, uint64_t a, uint64_t b, F&& f)
{
    constexpr uint32_t PER = 16 / sizeof(T);
    const uint32_t tid = threadIdx.x;
    const rsx_expand::Stores st = rsx_expand::tile_stores(reinterpret_cast<uintptr_t>(out), sizeof(T), a, b);
    const uint64_t body = a + st.head, rest = body + st.nvec * PER;
    if (tid < st.head) {
        out[a + tid] = f(a + tid);
    }
    if (tid < st.tail) {
        out[rest + tid] = f(rest + tid);
    }
    // Four 16-byte stores per thread and step, their elements fetched first: f may load from global memory (two dependent loads in
    // gather form), and one store at a time left a tile waiting for each of them in turn.  A lane past the end fetches the last
    // vector again (a valid address, no branch around the loads) and stores nothing.
    constexpr uint32_t BATCH = 4;
    const uint32_t nvec = static_cast<uint32_t>(st.nvec);
    for (uint32_t v0 = tid; v0 < nvec; v0 += BATCH * kExpandThreads) {         // (nvec > 0 inside)
        ExpandVec<T> w[BATCH];
#pragma unroll
        for (uint32_t k = 0; k < BATCH; ++k) {
            const uint64_t p = body + static_cast<uint64_t>(min(v0 + k * kExpandThreads, nvec - 1u)) * PER;
#pragma unroll
            for (uint32_t j = 0; j < PER; ++j) {
                w[k].x[j] = f(p + j);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < BATCH; ++k) {
            const uint32_t v = v0 + k * kExpandThreads;
            if (v < nvec) {
                *reinterpret_cast<ExpandVec<T>*>(out + body + static_cast<uint64_t>(v) * PER) = w[k];
            }
        }
    }
}

// Val: uint32_t or uint64_t, the opaque bits of a value (with values == nullptr no value is read or written, whatever Val is).
// Workgroup b takes the tiles [b * chunk, (b + 1) * chunk) of the absolute grid.
template <typename Val, bool GATHER>
__global__ __launch_bounds__(kExpandThreads) void expand_tile_kernel(const Val* __restrict__ values, const uint64_t* __restrict__ off, uint64_t nseg,
                                                                    const uint64_t* __restrict__ starts, const uint32_t* __restrict__ bad,
                                                                    const uint32_t* __restrict__ split, uint32_t ntiles, uint32_t chunk,
                                                                    Val* __restrict__ vout, uint32_t* __restrict__ sout, uint32_t* __restrict__ rout)
{
    __shared__ ExpandShared sh;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    const uint64_t lo = off[0], hi = off[nseg];
    const bool need_rank = rout != nullptr || (GATHER && vout != nullptr);      // (uniform)
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const rsx_expand::Range r = rsx_expand::tile_range(t, lo, hi);
        if (r.a >= r.b) continue;                                               // (uniform) nothing of [off[0], off[S]) in this tile
        const uint64_t tile_start = static_cast<uint64_t>(t) << rsx_expand::kTileShift;
        const uint32_t s_lo = split[t], s_hi = split[t + 1];                    // (uniform) the starts inside the tile
        if (s_lo == s_hi) {
            // ---- fill path: the whole of [a, b) belongs to segment s_lo - 1 (r.a < r.b implies 1 <= s_lo <= S)
            const uint32_t s = s_lo - 1u;
            const uint64_t base = off[s];
            if (sout) {
                expand_emit(sout, r.a, r.b, [s](uint64_t) { return s; });
            }
            if (rout) {
                expand_emit(rout, r.a, r.b, [base](uint64_t i) { return static_cast<uint32_t>(i - base); });
            }
            if (vout) {
                if constexpr (GATHER) {
                    const Val* __restrict__ src = values + starts[s];
                    expand_emit(vout, r.a, r.b, [src, base](uint64_t i) { return src[i - base]; });
                } else {
                    const Val v = values[s];
                    expand_emit(vout, r.a, r.b, [v](uint64_t) { return v; });
                }
            }
            continue;
        }
        // ---- general path
        // 1. clear the marks
        {
            uint4* z = reinterpret_cast<uint4*>(sh.own + tid * kExpandPerThread);
#pragma unroll
            for (int j = 0; j < kExpandPerThread / 4; ++j) {
                z[j] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        __syncthreads();
        // 2. the walk: every start of the tile marks its slot with its id + 1; of equal offsets the largest id stays
        //    (four loads in flight per thread: a lane past the end reads off[s_hi - 1] again and marks nothing)
#pragma unroll 1
        for (uint64_t s = static_cast<uint64_t>(s_lo) + tid; s < s_hi; s += 4 * kExpandThreads) {
            uint64_t x[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                x[k] = off[min(s + k * kExpandThreads, static_cast<uint64_t>(s_hi) - 1u)] - tile_start;
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint64_t sk = s + k * kExpandThreads;
                if (sk < s_hi && x[k] < rsx_expand::kTileSlots) {               // (the second: always, with offsets that passed the check)
                    atomicMax(&sh.own[x[k]], static_cast<uint32_t>(sk) + 1u);
                }
            }
        }
        __syncthreads();
        // 3. the inclusive max-scan over the slots; what the tile inherits is s_lo
        uint32_t m[kExpandPerThread];
        {
            const uint4* q = reinterpret_cast<const uint4*>(sh.own + tid * kExpandPerThread);
#pragma unroll
            for (int j = 0; j < kExpandPerThread / 4; ++j) {
                const uint4 w = q[j];
                m[4 * j] = w.x;
                m[4 * j + 1] = w.y;
                m[4 * j + 2] = w.z;
                m[4 * j + 3] = w.w;
            }
        }
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < kExpandPerThread; ++j) {
            mine = max(mine, m[j]);
        }
        const uint32_t incl = wave_inclusive_max(mine);
        if (lane == kWave - 1) {
            sh.wtot[wave] = incl;
        }
        __syncthreads();
        uint32_t run = s_lo;
#pragma unroll
        for (uint32_t w = 0; w < kExpandThreads / kWave; ++w) {
            run = max(run, w < wave ? sh.wtot[w] : 0u);
        }
        const uint32_t left = __shfl_up(incl, 1);
        if (lane != 0) {
            run = max(run, left);
        }
        // run = owner + 1 of the slot before the thread's first.  Its rank comes from the offsets, every later one from the marks.
        uint32_t rk = 0;
        if (need_rank && run >= 1u && run <= nseg) {
            rk = static_cast<uint32_t>(tile_start + static_cast<uint64_t>(tid) * kExpandPerThread - off[run - 1u]) - 1u;     // (of the slot before; wraps to -1 at a start)
        }
        uint32_t rnk[kExpandPerThread];
#pragma unroll
        for (int j = 0; j < kExpandPerThread; ++j) {
            rk = m[j] != 0u ? 0u : rk + 1u;
            run = max(run, m[j]);
            m[j] = run;
            rnk[j] = rk;
        }
        {
            uint4* q = reinterpret_cast<uint4*>(sh.own + tid * kExpandPerThread);
#pragma unroll
            for (int j = 0; j < kExpandPerThread / 4; ++j) {
                q[j] = make_uint4(m[4 * j], m[4 * j + 1], m[4 * j + 2], m[4 * j + 3]);
            }
            if (need_rank) {
                uint4* p = reinterpret_cast<uint4*>(sh.rank + tid * kExpandPerThread);
#pragma unroll
                for (int j = 0; j < kExpandPerThread / 4; ++j) {
                    p[j] = make_uint4(rnk[4 * j], rnk[4 * j + 1], rnk[4 * j + 2], rnk[4 * j + 3]);
                }
            }
        }
        __syncthreads();
        // 4. the outputs, each by its own alignment.  Every position of [a, b) has an owner in [0, S).
        const uint32_t* own = sh.own;
        const uint32_t* rank = sh.rank;
        if (sout) {
            expand_emit(sout, r.a, r.b, [own, tile_start](uint64_t i) { return own[i - tile_start] - 1u; });
        }
        if (rout) {
            expand_emit(rout, r.a, r.b, [rank, tile_start](uint64_t i) { return rank[i - tile_start]; });
        }
        if (vout) {
            if constexpr (GATHER) {
                expand_emit(vout, r.a, r.b, [=](uint64_t i) { return values[starts[own[i - tile_start] - 1u] + rank[i - tile_start]]; });
            } else {
                expand_emit(vout, r.a, r.b, [=](uint64_t i) { return values[own[i - tile_start] - 1u]; });
            }
        }
        __syncthreads();                                                        // (the next tile clears the slots)
    }
}

}  // namespace rsx
