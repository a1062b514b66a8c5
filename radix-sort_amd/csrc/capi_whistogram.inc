// capi_whistogram.inc — C ABI of the weighted histogram (rsx_segmented_weighted_histogram, include/radixsort_hip.h): validate the offsets ->
// zero the S x B 64-bit sums (bins_zero_kernel over 2 * S * B words) -> one kernel over the 4096-key tiles of the global grid.  Kernel:
// rsx_wbins.hpp; the bin of a key: rsx_bin_math.hpp; the mass of a weight: rsx_mass_math.hpp.  Nothing of the engine's sort state is read or
// written: the call needs the first-bad-segment word and the status words, and no scratch at all.
// Included by rsx_capi.hip inside its extern "C" block, after capi_histogram.inc.

extern "C++" {
namespace {

struct WhistArgs {
    const void* weights;
    int32_t wexp;
    bool is_signed;
};

template <typename Key, int WK>
void whistogram_launch(rsx_engine* e, const TileChunks& c, const Key* keys, const WhistArgs& w, uint64_t n, const uint64_t* off, uint64_t nseg, const Key* edges,
                       const rsx_bins::EvenArgs<Key>& ev, int form, uint32_t nbins, const uint32_t* bad, uint32_t ntiles, uint64_t* sums)
{
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    const bool wvec = aligned16(w.weights);
    if (form == rsx_bins::kFormEdges) {
        hipLaunchKernelGGL((rsx::wbins_tile_kernel<Key, rsx_bins::kFormEdges, WK>), dim3(c.grid), dim3(rsx::kUniqThreads), 0, e->stream, keys, w.weights, wvec, n, off,
                           nseg, edges, ev, a, m, nbins, w.wexp, w.is_signed, bad, ntiles, c.chunk, sums);
    } else if (form == rsx_bins::kFormEvenFloat) {
        hipLaunchKernelGGL((rsx::wbins_tile_kernel<Key, rsx_bins::kFormEvenFloat, WK>), dim3(c.grid), dim3(rsx::kUniqThreads), 0, e->stream, keys, w.weights, wvec, n,
                           off, nseg, edges, ev, a, m, nbins, w.wexp, w.is_signed, bad, ntiles, c.chunk, sums);
    } else {
        hipLaunchKernelGGL((rsx::wbins_tile_kernel<Key, rsx_bins::kFormEvenInt, WK>), dim3(c.grid), dim3(rsx::kUniqThreads), 0, e->stream, keys, w.weights, wvec, n,
                           off, nseg, edges, ev, a, m, nbins, w.wexp, w.is_signed, bad, ntiles, c.chunk, sums);
    }
}

template <typename Key>
int whistogram_enqueue(rsx_engine* e, const Key* keys, const WhistArgs& w, uint32_t weight_kind, uint64_t n, const uint64_t* off, uint64_t nseg, const Key* edges,
                       const rsx_bins::EvenArgs<Key>& ev, int form, uint32_t nbins, uint64_t* sums)
{
    const uint64_t cus = cus_of(e);
    const uint32_t ntiles = static_cast<uint32_t>((n + rsx::kUniqTileKeys - 1) >> rsx::kUniqTileShift);
    const int rc = ensure_status_words(e);
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, off, n);
    const uint64_t words = 2 * nseg * nbins;          // (2^31 at most) the 64-bit sums as 32-bit words; 8-byte aligned, so the zeroing's head is even
    const uint32_t zgrid = static_cast<uint32_t>(std::min<uint64_t>((words / 4 + rsx::kBinsZeroThreads - 1) / rsx::kBinsZeroThreads + 1, cus * 16));
    hipLaunchKernelGGL(rsx::bins_zero_kernel, dim3(zgrid), dim3(rsx::kBinsZeroThreads), 0, e->stream, reinterpret_cast<uint32_t*>(sums), words, bad, e->seg_status,
                       kStatusCallWhistogram);
    if (ntiles != 0) {
        const TileChunks c = tile_chunks(ntiles, cus);
        if (weight_kind == RSX_WEIGHT_UINT32)
            whistogram_launch<Key, RSX_WEIGHT_UINT32>(e, c, keys, w, n, off, nseg, edges, ev, form, nbins, bad, ntiles, sums);
        else if (weight_kind == RSX_WEIGHT_FLOAT32)
            whistogram_launch<Key, RSX_WEIGHT_FLOAT32>(e, c, keys, w, n, off, nseg, edges, ev, form, nbins, bad, ntiles, sums);
        else
            whistogram_launch<Key, RSX_WEIGHT_FLOAT64>(e, c, keys, w, n, off, nseg, edges, ev, form, nbins, bad, ntiles, sums);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_weighted_histogram(rsx_engine* e, const void* d_keys, const void* d_weights, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments,
                                     const void* d_edges, uint64_t lo_bits, uint64_t hi_bits, uint32_t width_shift, uint64_t num_bins, uint32_t flags,
                                     uint32_t weight_kind, int32_t weight_exp, uint64_t* d_sums_out)
{
    constexpr uint64_t kMaxSums = 1ull << 30;
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: null engine");
    if (flags & ~static_cast<uint32_t>(RSX_WHIST_SIGNED)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: flags may hold RSX_WHIST_SIGNED and nothing else");
    if (weight_kind > RSX_WEIGHT_FLOAT64) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: weight_kind must be RSX_WEIGHT_UINT32 (0), RSX_WEIGHT_FLOAT32 (1) or RSX_WEIGHT_FLOAT64 (2)");
    if (weight_kind == RSX_WEIGHT_UINT32 ? weight_exp != 0 : (weight_exp > rsx_mass::kMaxWeightExp || weight_exp < -rsx_mass::kMaxWeightExp))
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: weight_exp must be 0 for RSX_WEIGHT_UINT32 and within +-2048 for the float kinds");
    if ((flags & RSX_WHIST_SIGNED) && weight_kind == RSX_WEIGHT_UINT32)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: RSX_WHIST_SIGNED belongs to the float weight kinds (a uint32 mass has no sign)");
    if (num_bins == 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: num_bins must be at least 1");
    if (d_edges && num_bins > rsx::kWbinsEdgesMax) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: at most 4096 bins in the edges form");
    if (d_edges && (lo_bits != 0 || hi_bits != 0 || width_shift != 0))
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: lo_bits, hi_bits and width_shift must be 0 in the edges form");
    if (num_bins > kMaxSums) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: at most 2^30 sums (num_segments x num_bins)");
    rsx_bins::EvenArgs<uint32_t> ev32{};
    rsx_bins::EvenArgs<uint64_t> ev64{};
    if (!d_edges) {
        const char* what = nullptr;
        const bool is_float = e->key_kind == RSX_KEY_FLOAT;
        const bool ok = e->key_bytes == 4 ? rsx_bins::make_even_args<uint32_t>(is_float, e->is_signed, e->descending, lo_bits, hi_bits, width_shift, num_bins, &ev32, &what)
                                          : rsx_bins::make_even_args<uint64_t>(is_float, e->is_signed, e->descending, lo_bits, hi_bits, width_shift, num_bins, &ev64, &what);
        if (!ok) return fail(RSX_CALCULATION_FAILED, (std::string("rsx_segmented_weighted_histogram: ") + what).c_str());
    }
    if (d_offsets && num_segments == 0) return RSX_OK;
    if (!d_offsets) num_segments = 1;
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: at most 2^31 elements");
    if (num_bins > kMaxSums / num_segments) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_weighted_histogram: at most 2^30 sums (num_segments x num_bins)");
    const uint64_t kb = static_cast<uint64_t>(e->key_bytes), wb = weight_kind == RSX_WEIGHT_FLOAT64 ? 8u : 4u;
    if ((n > 0 && !d_keys) || !aligned16(d_keys)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_weighted_histogram: keys must be a 16-byte aligned device pointer");
    if (!d_weights) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_weighted_histogram: weights must be a device pointer (keys as their own weights are not offered here)");
    if (!aligned(d_weights, wb)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_weighted_histogram: weights must be aligned to their element size");
    if (!aligned(d_edges, kb)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_weighted_histogram: edges must be aligned to the key size");
    if (!d_sums_out || !aligned(d_sums_out, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_weighted_histogram: the sums must be an 8-byte aligned device pointer");
    if (!aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_weighted_histogram: offsets must be an 8-byte aligned device pointer");
    const uint64_t kbytes = n * kb, wbytes = n * wb, obytes = (num_segments + 1) * 8, sbytes = num_segments * num_bins * 8, ebytes = d_edges ? (num_bins + 1) * kb : 0;
    if (check_buffers(e, "rsx_segmented_weighted_histogram", {{d_sums_out, sbytes}}, {{d_keys, kbytes}, {d_weights, wbytes}, {d_offsets, obytes}, {d_edges, ebytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    const int form = d_edges ? rsx_bins::kFormEdges : e->key_kind == RSX_KEY_FLOAT ? rsx_bins::kFormEvenFloat : rsx_bins::kFormEvenInt;
    const uint32_t nbins = static_cast<uint32_t>(num_bins);       // (2^30 at most)
    const WhistArgs w{d_weights, weight_exp, (flags & RSX_WHIST_SIGNED) != 0};
    if (e->key_bytes == 4)
        return whistogram_enqueue<uint32_t>(e, static_cast<const uint32_t*>(d_keys), w, weight_kind, n, d_offsets, num_segments, static_cast<const uint32_t*>(d_edges),
                                            ev32, form, nbins, d_sums_out);
    return whistogram_enqueue<uint64_t>(e, static_cast<const uint64_t*>(d_keys), w, weight_kind, n, d_offsets, num_segments, static_cast<const uint64_t*>(d_edges), ev64,
                                        form, nbins, d_sums_out);
}
