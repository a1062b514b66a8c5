// capi_segmented.inc — C ABI of the segmented sort (rsx_segmented_sort, include/radixsort_hip.h): classify -> small segments in LDS ->
// one 4-bit LSD chain over the tiles of all large segments together.  Kernels: rsx_segmented.hpp.
// Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc (the shared front end: SegShape, seg_grow, ensure_segmented).

extern "C++" {
namespace {

template <typename Key>
int segmented_enqueue(rsx_engine* e, const Key* kin, const uint32_t* pin, uint64_t n, const uint64_t* off, uint64_t nseg, Key* kout,
                      uint32_t* pout, bool carry_payload = true, bool small_segments = true)
{
    const SegShape s = seg_shape(n, nseg);
    int rc = ensure_segmented(e, s, nseg);
    if (rc != RSX_OK) return rc;
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    const rsx::KeyCodec<Key> both{a, m, a, m}, enc{a, m, Key{0}, Key{0}}, dec{Key{0}, Key{0}, a, m}, none{};
    const bool payload = e->has_payload && carry_payload;      // (rsx_segmented_unique without positions: keys alone, even on a payload engine)
    if (!payload) {
        pin = nullptr;
        pout = nullptr;
    }
    const int passes = static_cast<int>(e->passes());
    const uint64_t cus = cus_of(e);

    // 1. classify: block sums -> one-workgroup scan (header, first bad segment) -> every segment's place
    hipLaunchKernelGGL((rsx::seg_classify_kernel<Key, false>), dim3(static_cast<uint32_t>(s.nblocks)), dim3(rsx::kSegClassifyThreads), 0, e->stream,
                       off, nseg, n, e->seg_bsum, e->seg_hdr, e->seg_list, e->seg_large, e->seg_tstart, kin, kout, pin, pout);
    hipLaunchKernelGGL(rsx::seg_scan_kernel, dim3(1), dim3(rsx::kSegScanThreads), 0, e->stream, e->seg_bsum, static_cast<uint32_t>(s.nblocks), e->seg_hdr,
                       e->seg_tstart, n, s.max_large, s.max_tiles, e->seg_status);
    // (small_segments = false, rsx_segmented_rank: the caller ranks the segments of at most one tile itself, from the list; the chain alone
    // runs here, and the top-k's writing classify, which copies no one-key segment)
    if (small_segments) {
        hipLaunchKernelGGL((rsx::seg_classify_kernel<Key, true>), dim3(static_cast<uint32_t>(s.nblocks)), dim3(rsx::kSegClassifyThreads), 0, e->stream,
                           off, nseg, n, e->seg_bsum, e->seg_hdr, e->seg_list, e->seg_large, e->seg_tstart, kin, kout, pin, pout);
    } else {
        hipLaunchKernelGGL((rsx::seg_classify_kernel<Key, true, true>), dim3(static_cast<uint32_t>(s.nblocks)), dim3(rsx::kSegClassifyThreads), 0, e->stream,
                           off, nseg, n, e->seg_bsum, e->seg_hdr, e->seg_list, e->seg_large, e->seg_tstart, kin, kout, pin, pout);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);

    // 2. small segments: one workgroup per segment, all passes in LDS; grids bounded by what could exist and by residency
    if (small_segments) for_each_small_class(nseg, n, cus, [&](int c, uint64_t grid, auto shape) {
        constexpr int T = decltype(shape)::THREADS, K = decltype(shape)::KPT;
        constexpr size_t lds = rsx::SegSortLayout<Key, T, K>::BYTES;
        if (payload) {
            hipLaunchKernelGGL((rsx::seg_small_sort_kernel<Key, T, K, true>), dim3(static_cast<uint32_t>(grid)), dim3(T), lds, e->stream, kin, kout, pin, pout, off,
                               e->seg_list, e->seg_hdr, c, passes, both);
        } else {
            hipLaunchKernelGGL((rsx::seg_small_sort_kernel<Key, T, K, false>), dim3(static_cast<uint32_t>(grid)), dim3(T), lds, e->stream, kin, kout, pin, pout, off,
                               e->seg_list, e->seg_hdr, c, passes, both);
        }
    });
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);

    // 3. large segments: one chain over all their tiles; each pass writes back into the segments' own index ranges
    if (s.max_large) {
        const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(s.max_tiles, cus * 8));
        const uint32_t ntab = static_cast<uint32_t>(s.max_tiles);
        const uint32_t ngroups = (ntab + rsx::kScanTiles - 1) / rsx::kScanTiles;
        constexpr size_t lds = rsx::SegSortLayout<Key, rsx::kSegChainThreads, rsx::kSegChainKpt>::BYTES;
        for (int p = 0; p < passes; ++p) {
            const bool first = p == 0, last = p + 1 == passes;
            const Key* src = first ? kin : static_cast<const Key*>(e->keys[(p + 1) & 1]);
            Key* dst = last ? kout : static_cast<Key*>(e->keys[p & 1]);
            const uint32_t* psrc = first ? pin : e->perm[(p + 1) & 1];
            uint32_t* pdst = last ? pout : e->perm[p & 1];
            const rsx::KeyCodec<Key> cx = first && last ? both : first ? enc : last ? dec : none;
            const int shift = p * rsx::kRadixBits;
            hipLaunchKernelGGL((rsx::seg_histogram_kernel<Key>), dim3(grid), dim3(rsx::kSegChainThreads), 0, e->stream, src, e->seg_table, e->seg_hdr,
                               e->seg_large, e->seg_tstart, shift, cx);
            launch_table_scan(e, ntab, ngroups);
            if (payload) {
                hipLaunchKernelGGL((rsx::seg_reorder_kernel<Key, true>), dim3(grid), dim3(rsx::kSegChainThreads), lds, e->stream, src, dst, psrc, pdst,
                                   e->seg_table, e->seg_hdr, e->seg_large, e->seg_tstart, shift, cx);
            } else {
                hipLaunchKernelGGL((rsx::seg_reorder_kernel<Key, false>), dim3(grid), dim3(rsx::kSegChainThreads), lds, e->stream, src, dst, psrc, pdst,
                                   e->seg_table, e->seg_hdr, e->seg_large, e->seg_tstart, shift, cx);
            }
        }
        RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    }
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_sort(rsx_engine* e, const void* d_keys, const uint32_t* d_payload, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments,
                       void* d_keys_out, uint32_t* d_payload_out)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sort: null engine");
    if (n > e->capacity) return fail(RSX_RESIZE_FAILED, "rsx_segmented_sort: beyond capacity");
    if (n == 0 || num_segments == 0) return RSX_OK;
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sort: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sort: at most 2^31 keys (32-bit table slots, at most 2^20 chain tiles)");
    const SegShape shape = seg_shape(n, num_segments);
    if (shape.max_tiles > static_cast<uint64_t>(rsx::kMaxScanGroups) * rsx::kScanTiles)      // (cannot happen for n <= 2^31: kept as the scan's own bound)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sort: too many keys for one table scan (at most 2^20 tiles of the large-segment chain)");
    if (!d_keys || !aligned16(d_keys)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sort: keys must be a 16-byte aligned device pointer");
    if (!d_keys_out) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sort: no output buffer");
    if (!d_offsets || !aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sort: offsets must be an 8-byte aligned device pointer");
    if (e->has_payload && (!d_payload || !aligned16(d_payload))) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sort: payload engine needs a 16-byte aligned payload pointer");
    if (e->has_payload && !d_payload_out) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sort: payload engine needs a payload output buffer");
    // (without a payload engine the payload pointers are ignored: zero bytes)
    const uint64_t kbytes = n * static_cast<uint64_t>(e->key_bytes), pbytes = e->has_payload ? n * 4 : 0, obytes = (num_segments + 1) * 8;
    if (check_buffers(e, "rsx_segmented_sort", {{d_keys_out, kbytes}, {d_payload_out, pbytes}}, {{d_keys, kbytes}, {d_payload, pbytes}, {d_offsets, obytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    const int rc = by_key(e, [&](auto key) {
        using Key = decltype(key);
        return segmented_enqueue<Key>(e, static_cast<const Key*>(d_keys), d_payload, n, d_offsets, num_segments, static_cast<Key*>(d_keys_out), d_payload_out);
    });
    if (rc != RSX_OK) return rc;
    result_is_external(e, n);
    return RSX_OK;
}
