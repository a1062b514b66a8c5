// capi_segmented.inc — C ABI of the segmented sort (rsx_segmented_sort, include/radixsort_hip.h): classify -> small segments in LDS ->
// one 4-bit LSD chain over the tiles of all large segments together.  Kernels: rsx_segmented.hpp.
// Included by rsx_capi.hip inside its extern "C" block (the helpers below are templates: C++ linkage).

extern "C++" {
namespace {

// Launch bounds that depend on n and the segment count only (the host never reads the offsets).
struct SegShape {
    uint64_t nblocks;       // classify workgroups
    uint64_t max_large;     // large segments (> 4096 keys) there can be
    uint64_t max_tiles;     // tiles of the chain: the 4096-key grid plus at most one partial tile per large segment
};

SegShape seg_shape(uint64_t n, uint64_t nseg)
{
    SegShape s;
    s.nblocks = (nseg + rsx::kSegPerBlock - 1) / rsx::kSegPerBlock;
    s.max_large = std::min<uint64_t>(nseg, n / (rsx::kSegTileKeys + 1));
    s.max_tiles = s.max_large ? (n + rsx::kSegTileKeys - 1) / rsx::kSegTileKeys + s.max_large : 0;
    return s;
}

// One scratch buffer of the segmented sort: grown to `want` elements on demand, never inside a stream capture.
template <typename T>
int seg_grow(rsx_engine* e, T** p, uint64_t* cap, uint64_t want, const char* what)
{
    if (want <= *cap && *p) return RSX_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (e->stream && hipStreamIsCapturing(e->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return fail(RSX_CALCULATION_FAILED, (std::string("rsx_segmented_sort: ") + what + " must grow, which cannot happen inside a stream capture (run one call of this size first)").c_str());
    if (*p) {
        RSX_TRY(hipStreamSynchronize(e->stream), RSX_CALCULATION_FAILED);      // a pending call may still use the old buffer
        RSX_TRY(hipFree(*p), RSX_CLEANUP_FAILED);
        *p = nullptr;
        *cap = 0;
    }
    const uint64_t n = std::max<uint64_t>(want, 1);
    RSX_TRY(hipMalloc(reinterpret_cast<void**>(p), static_cast<size_t>(n) * sizeof(T)), RSX_INITIALIZATION_FAILED);
    *cap = n;
    return RSX_OK;
}

int ensure_segmented(rsx_engine* e, const SegShape& s, uint64_t nseg)
{
    int rc = RSX_OK;
    if (!e->seg_status_host) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (e->stream && hipStreamIsCapturing(e->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sort: the first call of an engine cannot run inside a stream capture (it allocates)");
        RSX_TRY(hipMalloc(reinterpret_cast<void**>(&e->seg_hdr), sizeof(rsx::SegHeader)), RSX_INITIALIZATION_FAILED);
        RSX_TRY(hipMalloc(reinterpret_cast<void**>(&e->seg_temp), 64), RSX_INITIALIZATION_FAILED);
        RSX_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->seg_status_host), 64, hipHostMallocMapped), RSX_HOST_BUFFERS_FAILED);
        e->seg_status_host[0] = 0;
        e->seg_status_host[1] = 0;       // (which call reported: capi_merge.inc)
        RSX_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&e->seg_status), e->seg_status_host, 0), RSX_HOST_BUFFERS_FAILED);
    }
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_bsum, &e->seg_bsum_cap, s.nblocks * rsx::SF_STRIDE, "the classify block sums");
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_list, &e->seg_list_cap, nseg, "the small-segment list");
    if (rc == RSX_OK && s.max_large) {
        const uint64_t groups = (s.max_tiles + rsx::kScanTiles - 1) / rsx::kScanTiles;
        rc = seg_grow(e, &e->seg_large, &e->seg_large_cap, s.max_large, "the large-segment table");
        if (rc == RSX_OK) rc = seg_grow(e, &e->seg_tstart, &e->seg_tstart_cap, s.max_large + 1, "the tile starts");
        if (rc == RSX_OK) rc = seg_grow(e, &e->seg_table, &e->seg_table_cap, rsx::kRadix * s.max_tiles, "the segmented table");
        if (rc == RSX_OK) rc = seg_grow(e, &e->seg_gsum, &e->seg_gsum_cap, rsx::kRadix * groups, "the group sums");
        if (rc == RSX_OK) rc = seg_grow(e, &e->seg_gsum2, &e->seg_gsum2_cap, rsx::kRadix * groups, "the scanned group sums");
    }
    return rc;
}

template <typename Key>
int segmented_enqueue(rsx_engine* e, const Key* kin, const uint32_t* pin, uint64_t n, const uint64_t* off, uint64_t nseg, Key* kout,
                      uint32_t* pout, bool carry_payload = true)
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
    const uint64_t cus = e->num_cus > 0 ? static_cast<uint64_t>(e->num_cus) : 256u;

    // 1. classify: block sums -> one-workgroup scan (header, first bad segment) -> every segment's place
    hipLaunchKernelGGL((rsx::seg_classify_kernel<Key, false>), dim3(static_cast<uint32_t>(s.nblocks)), dim3(rsx::kSegClassifyThreads), 0, e->stream,
                       off, nseg, n, e->seg_bsum, e->seg_hdr, e->seg_list, e->seg_large, e->seg_tstart, kin, kout, pin, pout);
    hipLaunchKernelGGL(rsx::seg_scan_kernel, dim3(1), dim3(rsx::kSegScanThreads), 0, e->stream, e->seg_bsum, static_cast<uint32_t>(s.nblocks), e->seg_hdr,
                       e->seg_tstart, n, s.max_large, s.max_tiles, e->seg_status);
    hipLaunchKernelGGL((rsx::seg_classify_kernel<Key, true>), dim3(static_cast<uint32_t>(s.nblocks)), dim3(rsx::kSegClassifyThreads), 0, e->stream,
                       off, nseg, n, e->seg_bsum, e->seg_hdr, e->seg_list, e->seg_large, e->seg_tstart, kin, kout, pin, pout);
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);

    // 2. small segments: one workgroup per segment, all passes in LDS; grids bounded by what could exist and by residency
    {
        const uint64_t min_len[rsx::kSegClasses] = {2, rsx::kSegClass0Max + 1, rsx::kSegClass1Max + 1};
        const uint64_t per_cu[rsx::kSegClasses] = {32, 16, 4};
        for (int c = 0; c < rsx::kSegClasses; ++c) {
            const uint64_t grid = std::min<uint64_t>({nseg, n / min_len[c], cus * per_cu[c]});
            if (grid == 0) continue;
            if (c == 0) {
                constexpr size_t lds = rsx::SegSortLayout<Key, 64, 4>::BYTES;
                if (payload) hipLaunchKernelGGL((rsx::seg_small_sort_kernel<Key, 64, 4, true>), dim3(static_cast<uint32_t>(grid)), dim3(64), lds, e->stream, kin, kout, pin, pout, off, e->seg_list, e->seg_hdr, c, passes, both);
                else hipLaunchKernelGGL((rsx::seg_small_sort_kernel<Key, 64, 4, false>), dim3(static_cast<uint32_t>(grid)), dim3(64), lds, e->stream, kin, kout, pin, pout, off, e->seg_list, e->seg_hdr, c, passes, both);
            } else if (c == 1) {
                constexpr size_t lds = rsx::SegSortLayout<Key, 64, 16>::BYTES;
                if (payload) hipLaunchKernelGGL((rsx::seg_small_sort_kernel<Key, 64, 16, true>), dim3(static_cast<uint32_t>(grid)), dim3(64), lds, e->stream, kin, kout, pin, pout, off, e->seg_list, e->seg_hdr, c, passes, both);
                else hipLaunchKernelGGL((rsx::seg_small_sort_kernel<Key, 64, 16, false>), dim3(static_cast<uint32_t>(grid)), dim3(64), lds, e->stream, kin, kout, pin, pout, off, e->seg_list, e->seg_hdr, c, passes, both);
            } else {
                constexpr size_t lds = rsx::SegSortLayout<Key, 256, 16>::BYTES;
                if (payload) hipLaunchKernelGGL((rsx::seg_small_sort_kernel<Key, 256, 16, true>), dim3(static_cast<uint32_t>(grid)), dim3(256), lds, e->stream, kin, kout, pin, pout, off, e->seg_list, e->seg_hdr, c, passes, both);
                else hipLaunchKernelGGL((rsx::seg_small_sort_kernel<Key, 256, 16, false>), dim3(static_cast<uint32_t>(grid)), dim3(256), lds, e->stream, kin, kout, pin, pout, off, e->seg_list, e->seg_hdr, c, passes, both);
            }
        }
        RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    }

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
            hipLaunchKernelGGL((rsx::scan_blocks_kernel<false, false>), dim3(ngroups), dim3(rsx::kScanTiles), 0, e->stream, e->seg_table, e->seg_gsum,
                               ntab, ngroups, static_cast<uint32_t*>(nullptr));
            hipLaunchKernelGGL(rsx::paste_scan_kernel, dim3(ngroups), dim3(rsx::kScanTiles), 0, e->stream, e->seg_table, e->seg_gsum, e->seg_gsum2,
                               e->seg_temp, ntab, ngroups);
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
    if (!d_offsets || (reinterpret_cast<uintptr_t>(d_offsets) & 7u) != 0) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sort: offsets must be an 8-byte aligned device pointer");
    if (e->has_payload && (!d_payload || !aligned16(d_payload))) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sort: payload engine needs a 16-byte aligned payload pointer");
    if (e->has_payload && !d_payload_out) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sort: payload engine needs a payload output buffer");
    const uint64_t kbytes = n * static_cast<uint64_t>(e->key_bytes), pbytes = n * 4, obytes = (num_segments + 1) * 8;
    const uint64_t ebytes = e->capacity * static_cast<uint64_t>(e->key_bytes), epbytes = e->capacity * 4;
    const void* pi = e->has_payload ? d_payload : nullptr;
    const void* po = e->has_payload ? d_payload_out : nullptr;
    for (int i = 0; i < 2; ++i) {
        const void* eb[2] = {e->keys[i], e->perm[i]};
        const uint64_t eby[2] = {ebytes, epbytes};
        for (int j = 0; j < 2; ++j) {
            if (overlaps(d_keys, kbytes, eb[j], eby[j]) || overlaps(pi, pbytes, eb[j], eby[j]) || overlaps(d_keys_out, kbytes, eb[j], eby[j]) ||
                overlaps(po, pbytes, eb[j], eby[j]) || overlaps(d_offsets, obytes, eb[j], eby[j]))
                return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sort: an input or output overlaps the engine's own buffers");
        }
    }
    const void* outs[2] = {d_keys_out, po};
    const uint64_t outb[2] = {kbytes, pbytes};
    for (int j = 0; j < 2; ++j) {
        if (overlaps(outs[j], outb[j], d_keys, kbytes) || overlaps(outs[j], outb[j], pi, pbytes) || overlaps(outs[j], outb[j], d_offsets, obytes))
            return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sort: an output overlaps an input");
    }
    if (overlaps(d_keys_out, kbytes, po, pbytes)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_sort: the key and payload outputs overlap");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    const int rc = RSX_BY_KEY(e,
                              segmented_enqueue<uint32_t>(e, static_cast<const uint32_t*>(d_keys), d_payload, n, d_offsets, num_segments,
                                                          static_cast<uint32_t*>(d_keys_out), d_payload_out),
                              segmented_enqueue<uint64_t>(e, static_cast<const uint64_t*>(d_keys), d_payload, n, d_offsets, num_segments,
                                                          static_cast<uint64_t*>(d_keys_out), d_payload_out));
    if (rc != RSX_OK) return rc;
    // as after rsx_sort_from_to: the result lives in the caller's buffers only, and the engine's tables are not this call's
    e->n = n;
    e->result_external = true;
    e->counted_keys = nullptr;
    e->table_valid = false;
    e->globsum_valid = false;
    return RSX_OK;
}
