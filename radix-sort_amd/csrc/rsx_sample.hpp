// rsx_sample.hpp — kernels of rsx_segmented_sample: for every (segment, draw) the smallest index i of the segment, in INPUT order, whose
// running mass P_i = m_0 + ... + m_i reaches the draw's target (torch.multinomial with replacement, top-k / top-p / min-p sampling, per
// segment).  Included by rsx_capi.hip (host side: capi_sample.inc).  The mass of a weight and the target rule: rsx_mass_math.hpp, exactly
// rsx_segmented_weighted_select's; the predicate of the bound form: rsx_segmented_compact's; the walk and the crossing rule:
// rsx_sample_math.hpp, pure, run on the host by sample_selftest.
//
//   (unique_reset_kernel + unique_validate_kernel, unchanged: the first bad segment, one word)
//   sample_tile_kernel  per 4096-element tile of the global grid, a workgroup walks `chunk` consecutive tiles.  Only what crosses a tile
//                       edge is summed: lead[t] = the mass of the tile's elements that belong to the segment of its first element, if that
//                       segment began in an earlier tile; tail[t] = the mass of those that belong to the segment of its last element, if
//                       that segment goes on behind the tile.  A tile inside one long segment is read once, in 16-byte loads, and gives
//                       both.  A tile that holds whole segments only is not read at all.  Sums are 64-bit integer adds in any order.
//   sample_draw_kernel  one WAVE per slot (s, q), grid-stride.  total: a segment inside one tile is summed from its elements, a longer one
//                       from its pieces, tail[ta] + lead[ta+1 .. tb].  Then T (rsx_mass::target_of), the walk over the pieces in chunks of
//                       kWalkTiles = 256 tiles (a lane sums 4 consecutive ones, one wave scan per chunk) to the tile that holds the crossing
//                       and the mass before it, and the same step over the 256-element groups of that one piece, masses recomputed.  The
//                       lane whose element has before < T <= before + m stores index and P.  Lane 0 of draw 0 stores the total; with bad
//                       offsets nothing is stored and the call is reported.
//
// What is read: the pass reads the weights (and the keys where a bound or self-weights need them) of the tiles that long segments touch,
// once; a draw reads one tile's piece (a segment inside one tile: its elements twice, for the total and for the crossing, both from
// cache).  What is written: 16 bytes per tile and the outputs.  No atomic, no float add: equal input gives equal bits on any grid.
// Instantiations: {uint32, uint64 keys} x {uint32, float32, float64 weights, self} x {no bound, bound} where they differ.  No scratch memory.
#pragma once

#include "rsx_compact.hpp"
#include "rsx_sample_math.hpp"
#include "rsx_wselect.hpp"

namespace rsx {

constexpr int kSampleThreads = 256;                                  // sample_draw_kernel: 4 waves, a slot each
constexpr uint32_t kSampleGroup = kWave * rsx_sample::kWalkLane;     // elements per step inside a piece: a lane holds 4 consecutive ones
static_assert(rsx_sample::kTileShift == kUniqTileShift && rsx_sample::kTileKeys == kUniqTileKeys, "the pure header's tile is the family's");
static_assert(rsx_sample::kWalkTiles == kWave * rsx_sample::kWalkLane, "a chunk of the walk is one wave step");

// What is uniform over a call.  keys: read with BOUND or self-weights only.  benc below: the segment's bound, encoded.
template <typename Key>
struct SampleIn {
    const Key* keys;
    const void* weights;
    const Key* bounds;
    int32_t wexp;
    bool strict, invert;
    Key ca, cm;
};

template <typename Key, int WK, bool BOUND>
__device__ __forceinline__ uint32_t sample_mass_of(const SampleIn<Key>& in, Key k, uint64_t wbits, Key benc)
{
    uint32_t m;
    if constexpr (WK == kWselSelf) {
        m = sizeof(Key) == 4 ? rsx_mass::mass_f32_bits(static_cast<uint32_t>(k), in.wexp) : rsx_mass::mass_f64_bits(static_cast<uint64_t>(k), in.wexp);
    } else {
        m = rsx_mass::mass_of_bits(wbits, static_cast<uint32_t>(WK), in.wexp);
    }
    if constexpr (BOUND) {
        const Key x = codec_encode(k, in.ca, in.cm);
        const bool keep = (in.strict ? x < benc : x <= benc) != in.invert;
        m = keep ? m : 0u;
    }
    return m;
}

// the mass of element idx (idx < n is the caller's)
template <typename Key, int WK, bool BOUND>
__device__ __forceinline__ uint32_t sample_mass_at(const SampleIn<Key>& in, uint64_t idx, Key benc)
{
    Key k = 0;
    uint64_t wbits = 0;
    if constexpr (BOUND || WK == kWselSelf) {
        k = in.keys[idx];
    }
    if constexpr (WK != kWselSelf) {
        wbits = static_cast<const typename WselWord<WK>::type*>(in.weights)[idx];
    }
    return sample_mass_of<Key, WK, BOUND>(in, k, wbits, benc);
}

// four consecutive elements from a 16-byte aligned address
template <typename T>
__device__ __forceinline__ void sample_load4(const T* __restrict__ p, T (&out)[4])
{
    constexpr int VEC = 16 / static_cast<int>(sizeof(T));
#pragma unroll
    for (int q = 0; q < 4 / VEC; ++q) {
        const WselVec<T, VEC> v = *reinterpret_cast<const WselVec<T, VEC>*>(p + q * VEC);
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            out[q * VEC + c] = v.w[c];
        }
    }
}

__device__ __forceinline__ uint64_t sample_wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        v += __shfl_xor(v, d);
    }
    return v;
}

// The thread's share of the mass of [x, y), a range inside the tile at tile_start, under the bound benc: the sum has no order, so the loads
// are coalesced ones, 16 bytes per lane where the range is the whole tile and `vec` (16-byte aligned weights).
template <typename Key, int WK, bool BOUND>
__device__ __forceinline__ uint64_t sample_range_share(const SampleIn<Key>& in, bool vec, uint64_t tile_start, uint64_t x, uint64_t y, Key benc)
{
    using WT = typename WselWord<WK>::type;
    constexpr bool KEYS = BOUND || WK == kWselSelf;
    const uint32_t tid = threadIdx.x;
    uint64_t sum = 0;
    if (vec && x == tile_start && y == tile_start + kUniqTileKeys) {
#pragma unroll
        for (int q = 0; q < kUniqKpt / 4; ++q) {
            const uint64_t base = tile_start + (static_cast<uint64_t>(q) * kUniqThreads + tid) * 4u;
            Key k[4] = {0, 0, 0, 0};
            WT w[4] = {0, 0, 0, 0};
            if constexpr (KEYS) {
                sample_load4<Key>(in.keys + base, k);
            }
            if constexpr (WK != kWselSelf) {
                sample_load4<WT>(static_cast<const WT*>(in.weights) + base, w);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                sum += sample_mass_of<Key, WK, BOUND>(in, k[c], w[c], benc);
            }
        }
    } else {
#pragma unroll 4
        for (int j = 0; j < kUniqKpt; ++j) {
            const uint64_t idx = tile_start + static_cast<uint64_t>(j) * kUniqThreads + tid;
            if (idx >= x && idx < y) {
                sum += sample_mass_at<Key, WK, BOUND>(in, idx, benc);
            }
        }
    }
    return sum;
}

// Workgroup b takes the tiles [b * chunk, (b + 1) * chunk).  lead / tail: ntiles 8-byte slots each; a slot that no walk will read is not written.
template <typename Key, int WK, bool BOUND>
__global__ __launch_bounds__(kUniqThreads) void sample_tile_kernel(SampleIn<Key> in, bool wvec, uint64_t n, const uint64_t* __restrict__ off, uint64_t nseg,
                                                                   const uint32_t* __restrict__ bad, uint32_t ntiles, uint32_t chunk,
                                                                   uint64_t* __restrict__ lead, uint64_t* __restrict__ tail)
{
    __shared__ uint64_t wsum[kUniqThreads / kWave];
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    if (*bad != kUniqNoBad || t0 >= t1) return;
    const uint64_t lo = uniq_off(off, 0, n), hi = uniq_off(off, nseg, n);
    // the workgroup's sum of the threads' shares (uniform result)
    auto block_sum = [&](uint64_t v) {
        v = sample_wave_sum(v);
        if ((tid & (kWave - 1)) == 0) {
            wsum[tid / kWave] = v;
        }
        __syncthreads();
        uint64_t all = 0;
#pragma unroll
        for (int w = 0; w < kUniqThreads / kWave; ++w) {
            all += wsum[w];
        }
        __syncthreads();
        return all;
    };
    uint64_t from = 0;
#pragma unroll 1
    for (uint32_t t = t0; t < t1; ++t) {
        const uint64_t tile_start = static_cast<uint64_t>(t) << kUniqTileShift;
        const uint64_t tile_end = tile_start + kUniqTileKeys;
        if (tile_start >= hi || tile_end <= lo) continue;                               // (uniform, as everything up to the shares)
        // the segment of the tile's first element, if it began before the tile; the segment of its last one, if it goes on behind it
        bool need_lead = false, need_tail = false;
        uint64_t sl = 0, st = 0, lead_end = 0, tail_start = 0;
        if (tile_start > lo) {                                                          // (tile_start < hi)
            sl = compact_seg_upper(off, from, nseg, n, tile_start) - 1;
            from = sl;
            need_lead = uniq_off(off, sl, n) < tile_start;
            lead_end = min(uniq_off(off, sl + 1, n), tile_end);
        }
        if (tile_end < hi) {                                                            // (tile_end > lo; hi <= n: the tile is whole)
            st = compact_seg_upper(off, from, nseg, n, tile_end - 1) - 1;
            from = st;
            need_tail = uniq_off(off, st + 1, n) > tile_end;
            tail_start = max(uniq_off(off, st, n), tile_start);
        }
        if (need_lead) {
            const Key benc = BOUND ? codec_encode(in.bounds[sl], in.ca, in.cm) : Key{0};
            const uint64_t m = block_sum(sample_range_share<Key, WK, BOUND>(in, wvec, tile_start, tile_start, lead_end, benc));
            if (tid == 0) {
                lead[t] = m;
                if (need_tail && st == sl) {
                    tail[t] = m;                                                        // the tile lies inside one segment
                }
            }
        }
        if (need_tail && !(need_lead && st == sl)) {
            const Key benc = BOUND ? codec_encode(in.bounds[st], in.ca, in.cm) : Key{0};
            const uint64_t m = block_sum(sample_range_share<Key, WK, BOUND>(in, wvec, tile_start, tail_start, tile_end, benc));
            if (tid == 0) {
                tail[t] = m;
            }
        }
    }
}

// One step of a wave over 256 consecutive values in order, lane l holding v[0..3] = values 4l .. 4l+3, `before` = the mass before them.
// false: T is not crossed here and `before` has moved on behind them.  true: on the one lane that holds the crossing hit = its j and
// at = the mass before that value; hit = -1 on every other lane.  (uniform return)
__device__ __forceinline__ bool sample_wave_step(const uint64_t (&v)[rsx_sample::kWalkLane], uint64_t& before, uint64_t T, int& hit, uint64_t& at)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t mine = v[0] + v[1] + v[2] + v[3];
    uint64_t x = mine;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t y = __shfl_up(x, d);
        x += lane >= static_cast<uint32_t>(d) ? y : 0ull;
    }
    const uint64_t sum = __shfl(x, kWave - 1);
    hit = -1;
    if (!rsx_sample::crosses(before, sum, T)) {
        before += sum;
        return false;
    }
    uint64_t p = before + x - mine;
#pragma unroll
    for (int j = 0; j < static_cast<int>(rsx_sample::kWalkLane); ++j) {
        if (rsx_sample::crosses(p, v[j], T)) {
            hit = j;
            at = p;
        }
        p += v[j];
    }
    return true;
}

// Any grid: the slots are taken wave by wave, grid-stride.  With bad offsets nothing is written and the first bad segment + 1 goes to
// the mapped host words with the call's id, unless an earlier report is still pending there (as segreduce_join_kernel does).
template <typename Key, int WK, bool BOUND>
__global__ __launch_bounds__(kSampleThreads) void sample_draw_kernel(SampleIn<Key> in, uint64_t n, const uint64_t* __restrict__ off, uint64_t nseg,
                                                                     const void* __restrict__ targets, uint32_t R, bool fraction,
                                                                     const uint32_t* __restrict__ bad, const uint64_t* __restrict__ lead,
                                                                     const uint64_t* __restrict__ tail, uint32_t* __restrict__ iout,
                                                                     uint64_t* __restrict__ mout, uint64_t* __restrict__ tout, uint32_t* status_host,
                                                                     uint32_t call_id)
{
    constexpr uint32_t WAVES = kSampleThreads / kWave, LANE = rsx_sample::kWalkLane;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t b = *bad;
    if (b != kUniqNoBad) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && __hip_atomic_load(status_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
            __hip_atomic_store(status_host + 1, call_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(status_host, b + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);        // (after the call's id)
        }
        return;
    }
    const uint64_t slots = nseg * R, stride = static_cast<uint64_t>(gridDim.x) * WAVES;
#pragma unroll 1
    for (uint64_t slot = static_cast<uint64_t>(blockIdx.x) * WAVES + threadIdx.x / kWave; slot < slots; slot += stride) {      // (wave-uniform)
        const uint64_t s = slot / R;
        const uint32_t q = static_cast<uint32_t>(slot - s * R);
        const uint64_t sb = uniq_off(off, s, n), se = uniq_off(off, s + 1, n);
        const Key benc = BOUND ? codec_encode(in.bounds[s], in.ca, in.cm) : Key{0};
        const bool one_tile = sb == se || rsx_sample::first_tile(sb) == rsx_sample::last_tile(se);
        const uint32_t ta = sb == se ? 0u : rsx_sample::first_tile(sb), tb = sb == se ? 0u : rsx_sample::last_tile(se);
        // the masses of the pieces of the 4 tiles c + 4 lane .. of a long segment
        auto pieces = [&](uint64_t c, uint64_t (&v)[LANE]) {
#pragma unroll
            for (uint32_t j = 0; j < LANE; ++j) {
                const uint64_t t = c + static_cast<uint64_t>(lane) * LANE + j;
                v[j] = t <= tb ? rsx_sample::piece_mass(lead, tail, ta, static_cast<uint32_t>(t)) : 0ull;
            }
        };
        // 1. the total
        uint64_t total = 0;
        if (one_tile) {
#pragma unroll 4
            for (uint64_t i = sb + lane; i < se; i += kWave) {
                total += sample_mass_at<Key, WK, BOUND>(in, i, benc);
            }
        } else {
#pragma unroll 1
            for (uint64_t c = ta; c <= tb; c += rsx_sample::kWalkTiles) {
                uint64_t v[LANE];
                pieces(c, v);
                total += v[0] + v[1] + v[2] + v[3];
            }
        }
        total = sample_wave_sum(total);
        if (q == 0 && tout && lane == 0) {
            tout[s] = total;
        }
        // 2. the target, then the tile whose piece holds the crossing and the mass before it
        const uint64_t T = wsel_target(targets, slot, fraction, total);
        if (T == 0) continue;
        uint64_t before = 0;
        uint32_t tile = ta;
        if (!one_tile) {
            tile = rsx_sample::kNoTile;
#pragma unroll 1
            for (uint64_t c = ta; c <= tb; c += rsx_sample::kWalkTiles) {
                uint64_t v[LANE], at = 0;
                int hit;
                pieces(c, v);
                if (!sample_wave_step(v, before, T, hit, at)) continue;
                const int src = __ffsll(static_cast<long long>(__ballot(hit >= 0))) - 1;          // (one lane; T <= total: there is one)
                tile = __shfl(static_cast<uint32_t>(c + static_cast<uint64_t>(lane) * LANE + static_cast<uint32_t>(max(hit, 0))), src);
                before = __shfl(at, src);
                break;
            }
            if (tile == rsx_sample::kNoTile) continue;                                            // (not reached with consistent partials)
        }
        // 3. that piece, 256 elements a step
        const rsx_sample::Piece pc = rsx_sample::piece_of(sb, se, tile);
#pragma unroll 1
        for (uint64_t base = pc.start; base < pc.end; base += kSampleGroup) {
            uint64_t v[LANE], at = 0;
            int hit;
#pragma unroll
            for (uint32_t j = 0; j < LANE; ++j) {
                const uint64_t i = base + static_cast<uint64_t>(lane) * LANE + j;
                v[j] = i < pc.end ? static_cast<uint64_t>(sample_mass_at<Key, WK, BOUND>(in, i, benc)) : 0ull;
            }
            if (!sample_wave_step(v, before, T, hit, at)) continue;
            if (hit >= 0) {
                const uint64_t i = base + static_cast<uint64_t>(lane) * LANE + static_cast<uint32_t>(hit);
                uint64_t m = v[0];
#pragma unroll
                for (int j = 1; j < static_cast<int>(LANE); ++j) {
                    m = hit == j ? v[j] : m;
                }
                iout[slot] = static_cast<uint32_t>(i - sb);
                if (mout) {
                    mout[slot] = at + m;
                }
            }
            break;
        }
    }
}

}  // namespace rsx
