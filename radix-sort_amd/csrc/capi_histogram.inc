// capi_histogram.inc — C ABI of the histogram (rsx_segmented_histogram, include/radixsort_hip.h): validate the offsets -> zero the S x B
// counters -> one kernel over the 4096-key tiles of the global grid.  Kernels: rsx_bins.hpp; the bin of a key: rsx_bin_math.hpp.  Nothing of
// the engine's sort state is read or written: the call needs the first-bad-segment word and the status words, and no scratch at all.
// Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc.

extern "C++" {
namespace {

template <typename Key>
int histogram_enqueue(rsx_engine* e, const Key* keys, uint64_t n, const uint64_t* off, uint64_t nseg, const Key* edges, const rsx_bins::EvenArgs<Key>& ev,
                      int form, uint32_t nbins, uint32_t* counts)
{
    const uint64_t cus = cus_of(e);
    const uint32_t ntiles = static_cast<uint32_t>((n + rsx::kUniqTileKeys - 1) >> rsx::kUniqTileShift);
    const int rc = ensure_status_words(e);
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, off, n);
    const uint64_t total = nseg * nbins;
    const uint32_t zgrid = static_cast<uint32_t>(std::min<uint64_t>((total / 4 + rsx::kBinsZeroThreads - 1) / rsx::kBinsZeroThreads + 1, cus * 16));
    hipLaunchKernelGGL(rsx::bins_zero_kernel, dim3(zgrid), dim3(rsx::kBinsZeroThreads), 0, e->stream, counts, total, bad, e->seg_status, kStatusCallHistogram);
    if (ntiles != 0) {
        const TileChunks c = tile_chunks(ntiles, cus);
        Key a = 0, m = 0;
        order_consts<Key>(e, &a, &m);
        if (form == rsx_bins::kFormEdges) {
            hipLaunchKernelGGL((rsx::bins_tile_kernel<Key, rsx_bins::kFormEdges>), dim3(c.grid), dim3(rsx::kUniqThreads), 0, e->stream, keys, n, off, nseg, edges, ev,
                               a, m, nbins, bad, ntiles, c.chunk, counts);
        } else if (form == rsx_bins::kFormEvenFloat) {
            hipLaunchKernelGGL((rsx::bins_tile_kernel<Key, rsx_bins::kFormEvenFloat>), dim3(c.grid), dim3(rsx::kUniqThreads), 0, e->stream, keys, n, off, nseg, edges,
                               ev, a, m, nbins, bad, ntiles, c.chunk, counts);
        } else {
            hipLaunchKernelGGL((rsx::bins_tile_kernel<Key, rsx_bins::kFormEvenInt>), dim3(c.grid), dim3(rsx::kUniqThreads), 0, e->stream, keys, n, off, nseg, edges, ev,
                               a, m, nbins, bad, ntiles, c.chunk, counts);
        }
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_histogram(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, const void* d_edges,
                            uint64_t lo_bits, uint64_t hi_bits, uint32_t width_shift, uint64_t num_bins, uint32_t flags, uint32_t* d_counts_out)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_histogram: null engine");
    if (flags != 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_histogram: unknown flag bits (flags must be 0)");
    if (num_bins == 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_histogram: num_bins must be at least 1");
    if (d_edges && num_bins > rsx::kBinsLdsMax) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_histogram: at most 4096 bins in the edges form");
    if (d_edges && (lo_bits != 0 || hi_bits != 0 || width_shift != 0))
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_histogram: lo_bits, hi_bits and width_shift must be 0 in the edges form");
    if (num_bins > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_histogram: at most 2^31 counters (num_segments x num_bins)");
    rsx_bins::EvenArgs<uint32_t> ev32{};
    rsx_bins::EvenArgs<uint64_t> ev64{};
    if (!d_edges) {
        const char* what = nullptr;
        const bool is_float = e->key_kind == RSX_KEY_FLOAT;
        const bool ok = e->key_bytes == 4 ? rsx_bins::make_even_args<uint32_t>(is_float, e->is_signed, e->descending, lo_bits, hi_bits, width_shift, num_bins, &ev32, &what)
                                          : rsx_bins::make_even_args<uint64_t>(is_float, e->is_signed, e->descending, lo_bits, hi_bits, width_shift, num_bins, &ev64, &what);
        if (!ok) return fail(RSX_CALCULATION_FAILED, (std::string("rsx_segmented_histogram: ") + what).c_str());
    }
    if (d_offsets && num_segments == 0) return RSX_OK;
    if (!d_offsets) num_segments = 1;
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_histogram: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_histogram: at most 2^31 elements");
    if (num_bins > (1ull << 31) / num_segments) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_histogram: at most 2^31 counters (num_segments x num_bins)");
    const uint64_t kb = static_cast<uint64_t>(e->key_bytes);
    if ((n > 0 && !d_keys) || !aligned16(d_keys)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_histogram: keys must be a 16-byte aligned device pointer");
    if (!aligned(d_edges, kb)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_histogram: edges must be aligned to the key size");
    if (!d_counts_out || !aligned(d_counts_out, 4)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_histogram: the counters must be a 4-byte aligned device pointer");
    if (!aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_histogram: offsets must be an 8-byte aligned device pointer");
    const uint64_t kbytes = n * kb, obytes = (num_segments + 1) * 8, cbytes = num_segments * num_bins * 4, ebytes = d_edges ? (num_bins + 1) * kb : 0;
    if (check_buffers(e, "rsx_segmented_histogram", {{d_counts_out, cbytes}}, {{d_keys, kbytes}, {d_offsets, obytes}, {d_edges, ebytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    const int form = d_edges ? rsx_bins::kFormEdges : e->key_kind == RSX_KEY_FLOAT ? rsx_bins::kFormEvenFloat : rsx_bins::kFormEvenInt;
    const uint32_t nbins = static_cast<uint32_t>(num_bins);       // (2^31 at most)
    if (e->key_bytes == 4)
        return histogram_enqueue<uint32_t>(e, static_cast<const uint32_t*>(d_keys), n, d_offsets, num_segments, static_cast<const uint32_t*>(d_edges), ev32, form, nbins,
                                           d_counts_out);
    return histogram_enqueue<uint64_t>(e, static_cast<const uint64_t*>(d_keys), n, d_offsets, num_segments, static_cast<const uint64_t*>(d_edges), ev64, form, nbins,
                                       d_counts_out);
}
