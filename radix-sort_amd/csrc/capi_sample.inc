// capi_sample.inc — C ABI of the categorical draw (rsx_segmented_sample, include/radixsort_hip.h): validate the offsets -> the masses that
// cross tile edges, per 4096-element tile of the global grid -> one wave per (segment, draw): total, target, the tile of the crossing, the
// element.  Kernels: rsx_sample.hpp; the walk and the crossing rule: rsx_sample_math.hpp; the mass of a weight and the target:
// rsx_mass_math.hpp.  Nothing of the engine's sort state is read or written: the call needs the first-bad-segment word, the status words
// and 2 * tiles 8-byte slots of per-tile scratch (the segmented reduction's buffer, grown on demand and never inside a capture).
// Included by rsx_capi.hip inside its extern "C" block, after capi_whistogram.inc.

extern "C++" {
namespace {

struct SampleArgs {
    const void* keys;
    const void* weights;
    const void* bounds;
    const void* targets;
    uint32_t R;
    uint32_t flags;
    int32_t wexp;
    uint32_t* iout;
    uint64_t* mout;
    uint64_t* tout;
};

template <typename Key, int WK, bool BOUND>
int sample_enqueue(rsx_engine* e, const SampleArgs& a, uint64_t n, const uint64_t* off, uint64_t nseg)
{
    const uint64_t cus = cus_of(e);
    const uint32_t ntiles = static_cast<uint32_t>((n + rsx::kUniqTileKeys - 1) >> rsx::kUniqTileShift);
    int rc = ensure_status_words(e);
    if (rc == RSX_OK) rc = seg_grow(e, &e->red_part, &e->red_part_cap, 4 * static_cast<uint64_t>(ntiles) + 2, "the per-tile partials of the sample");
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, off, n);
    rsx::SampleIn<Key> in;
    in.keys = static_cast<const Key*>(a.keys);
    in.weights = a.weights;
    in.bounds = static_cast<const Key*>(a.bounds);
    in.wexp = a.wexp;
    in.strict = (a.flags & RSX_COMPACT_STRICT) != 0;
    in.invert = (a.flags & RSX_COMPACT_INVERT) != 0;
    in.ca = 0;
    in.cm = 0;
    order_consts<Key>(e, &in.ca, &in.cm);
    uint64_t* lead = e->red_part;
    uint64_t* tail = e->red_part + ntiles;
    const bool wvec = a.weights ? aligned16(a.weights) : true;          // (keys are 16-byte aligned wherever they are read)
    const TileChunks c = tile_chunks(ntiles, cus);
    hipLaunchKernelGGL((rsx::sample_tile_kernel<Key, WK, BOUND>), dim3(c.grid), dim3(rsx::kUniqThreads), 0, e->stream, in, wvec, n, off, nseg, bad, ntiles, c.chunk,
                       lead, tail);
    // one wave per slot, bounded by residency
    constexpr uint64_t waves = rsx::kSampleThreads / rsx::kWave;
    const uint64_t slots = nseg * a.R;
    const uint32_t dgrid = static_cast<uint32_t>(std::min<uint64_t>((slots + waves - 1) / waves, cus * 32));
    hipLaunchKernelGGL((rsx::sample_draw_kernel<Key, WK, BOUND>), dim3(dgrid), dim3(rsx::kSampleThreads), 0, e->stream, in, n, off, nseg, a.targets, a.R,
                       (a.flags & RSX_WSELECT_FRACTION) != 0, bad, lead, tail, a.iout, a.mout, a.tout, e->seg_status, kStatusCallSample);
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

// Without a bound and with weights of their own the keys are not read: one key width serves.
template <typename Key, bool BOUND>
int sample_by_weight(rsx_engine* e, const SampleArgs& a, uint32_t weight_kind, uint64_t n, const uint64_t* off, uint64_t nseg)
{
    if (!a.weights) return sample_enqueue<Key, rsx::kWselSelf, BOUND>(e, a, n, off, nseg);
    if (weight_kind == RSX_WEIGHT_UINT32) return sample_enqueue<Key, RSX_WEIGHT_UINT32, BOUND>(e, a, n, off, nseg);
    if (weight_kind == RSX_WEIGHT_FLOAT32) return sample_enqueue<Key, RSX_WEIGHT_FLOAT32, BOUND>(e, a, n, off, nseg);
    return sample_enqueue<Key, RSX_WEIGHT_FLOAT64, BOUND>(e, a, n, off, nseg);
}

}  // namespace
}  // extern "C++"

int rsx_segmented_sample(rsx_engine* e, const void* d_keys, const void* d_weights, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments,
                         const void* d_bounds, const void* d_targets, uint32_t draws_per_segment, uint32_t flags, uint32_t weight_kind, int32_t weight_exp,
                         uint32_t* d_index_out, uint64_t* d_mass_out, uint64_t* d_total_out)
{
    const uint32_t R = draws_per_segment;
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sample: null engine");
    if (flags & ~static_cast<uint32_t>(RSX_WSELECT_FRACTION | RSX_COMPACT_STRICT | RSX_COMPACT_INVERT))
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sample: flags may hold RSX_WSELECT_FRACTION, RSX_COMPACT_STRICT and RSX_COMPACT_INVERT and nothing else");
    if (!d_bounds && (flags & (RSX_COMPACT_STRICT | RSX_COMPACT_INVERT)) != 0)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sample: RSX_COMPACT_STRICT and RSX_COMPACT_INVERT belong to the bound form (d_bounds is NULL)");
    if (weight_kind > RSX_WEIGHT_FLOAT64) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sample: weight_kind must be RSX_WEIGHT_UINT32 (0), RSX_WEIGHT_FLOAT32 (1) or RSX_WEIGHT_FLOAT64 (2)");
    if (weight_kind == RSX_WEIGHT_UINT32 ? weight_exp != 0 : (weight_exp > rsx_mass::kMaxWeightExp || weight_exp < -rsx_mass::kMaxWeightExp))
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sample: weight_exp must be 0 for RSX_WEIGHT_UINT32 and within +-2048 for the float kinds");
    if (!d_weights && (e->key_kind != RSX_KEY_FLOAT || weight_kind != (e->key_bytes == 4 ? RSX_WEIGHT_FLOAT32 : RSX_WEIGHT_FLOAT64)))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sample: without weights the keys are the weights: the engine must have RSX_KEY_FLOAT keys and weight_kind must be the float kind of their width");
    if (R == 0 || n == 0 || (d_offsets && num_segments == 0)) return RSX_OK;
    if (!d_offsets) num_segments = 1;
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sample: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sample: at most 2^31 elements");
    if (num_segments * R > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sample: at most 2^31 draws (num_segments x draws_per_segment)");
    const uint64_t kb = static_cast<uint64_t>(e->key_bytes), wb = weight_kind == RSX_WEIGHT_FLOAT64 ? 8u : 4u;
    const bool reads_keys = d_bounds || !d_weights;
    if (reads_keys && (!d_keys || !aligned16(d_keys))) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sample: keys must be a 16-byte aligned device pointer (they are read with d_bounds, and as the weights when d_weights is NULL)");
    if (!aligned(d_weights, wb)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sample: weights must be aligned to their element size");
    if (!aligned(d_bounds, kb)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sample: bounds must be aligned to the key size");
    if (!d_targets || !aligned(d_targets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sample: targets must be an 8-byte aligned device pointer");
    if (!d_index_out || !aligned(d_index_out, 4)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sample: the index output must be a 4-byte aligned device pointer");
    if (!aligned(d_mass_out, 8) || !aligned(d_total_out, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sample: the mass and total outputs must be 8-byte aligned");
    if (!aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sample: offsets must be an 8-byte aligned device pointer");
    const uint64_t slots = num_segments * R;
    if (check_buffers(e, "rsx_segmented_sample",
                      {{d_index_out, slots * 4}, {d_mass_out, d_mass_out ? slots * 8 : 0}, {d_total_out, d_total_out ? num_segments * 8 : 0}},
                      {{d_keys, reads_keys ? n * kb : 0}, {d_weights, d_weights ? n * wb : 0}, {d_offsets, d_offsets ? (num_segments + 1) * 8 : 0},
                       {d_bounds, d_bounds ? num_segments * kb : 0}, {d_targets, slots * 8}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    const SampleArgs a{d_keys, d_weights, d_bounds, d_targets, R, flags, weight_exp, d_index_out, d_mass_out, d_total_out};
    if (!reads_keys) return sample_by_weight<uint32_t, false>(e, a, weight_kind, n, d_offsets, num_segments);
    return by_key(e, [&](auto key) {
        using Key = decltype(key);
        if (d_bounds) return sample_by_weight<Key, true>(e, a, weight_kind, n, d_offsets, num_segments);
        return sample_by_weight<Key, false>(e, a, weight_kind, n, d_offsets, num_segments);
    });
}
