// capi_topk.inc — C ABI of the segmented top-k (rsx_segmented_topk, include/radixsort_hip.h): the segmented sort's classify chain ->
// small segments sorted in LDS (ranks < k stored) -> radix select over the tiles of all large segments, compaction of k candidates per
// segment, their LDS sort.  Kernels: rsx_topk.hpp.
// Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc and capi_segmented.inc.

extern "C++" {
namespace {

// Tiles per histogram group of the select rounds: enough groups for about 8 workgroups per CU, at most 64 tiles per group.
uint32_t topk_group_tiles(const SegShape& s, uint64_t cus)
{
    const uint64_t want = cus * 8;
    const uint64_t g = (s.max_tiles + want - 1) / want;
    return static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(g, 1), 64));
}

int ensure_topk(rsx_engine* e, const SegShape& s, uint32_t gtiles)
{
    int rc = RSX_OK;
    if (!s.max_large) return rc;
    const uint64_t groups = (s.max_tiles + gtiles - 1) / gtiles;
    rc = seg_grow(e, &e->topk_state, &e->topk_state_cap, s.max_large, "the top-k select state");
    if (rc == RSX_OK) rc = seg_grow(e, &e->topk_start, &e->topk_start_cap, s.max_large * rsx::kTopkBins, "the top-k segment counts");
    if (rc == RSX_OK) rc = seg_grow(e, &e->topk_cont, &e->topk_cont_cap, groups * rsx::kTopkBins, "the top-k group counts");
    return rc;
}

// The LDS sort of topk_sort_kernel in one of the segmented sort's three shapes (64 x 4, 64 x 16, 256 x 16).
template <typename Key, int THREADS, int KPT, bool FINAL>
void topk_sort_launch(rsx_engine* e, uint64_t grid, const Key* in, const uint32_t* cidx, Key* kout, uint32_t* iout, const uint64_t* off, int cls,
                      uint32_t k, const rsx::KeyCodec<Key>& codec)
{
    constexpr size_t lds = rsx::SegSortLayout<Key, THREADS, KPT>::BYTES;
    hipLaunchKernelGGL((rsx::topk_sort_kernel<Key, THREADS, KPT, FINAL>), dim3(static_cast<uint32_t>(grid)), dim3(THREADS), lds, e->stream, in, cidx, kout,
                       iout, off, e->seg_list, e->seg_hdr, e->seg_large, cls, static_cast<int>(e->passes()), k, codec);
}

template <typename Key>
int topk_enqueue(rsx_engine* e, const Key* kin, uint64_t n, const uint64_t* off, uint64_t nseg, uint32_t k, Key* kout, uint32_t* iout)
{
    const SegShape s = seg_shape(n, nseg);
    const uint64_t cus = cus_of(e);
    const uint32_t gtiles = topk_group_tiles(s, cus);
    int rc = ensure_segmented(e, s, nseg);
    if (rc == RSX_OK) rc = ensure_topk(e, s, gtiles);
    if (rc != RSX_OK) return rc;
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    const rsx::KeyCodec<Key> both{a, m, a, m};

    // 1. classify (the segmented sort's chain; the writing pass records the large segments' ids), then one-key segments and the
    //    select state of the large ones
    hipLaunchKernelGGL((rsx::seg_classify_kernel<Key, false>), dim3(static_cast<uint32_t>(s.nblocks)), dim3(rsx::kSegClassifyThreads), 0, e->stream,
                       off, nseg, n, e->seg_bsum, e->seg_hdr, e->seg_list, e->seg_large, e->seg_tstart, kin, static_cast<Key*>(nullptr),
                       static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr));
    hipLaunchKernelGGL(rsx::seg_scan_kernel, dim3(1), dim3(rsx::kSegScanThreads), 0, e->stream, e->seg_bsum, static_cast<uint32_t>(s.nblocks), e->seg_hdr,
                       e->seg_tstart, n, s.max_large, s.max_tiles, e->seg_status);
    hipLaunchKernelGGL((rsx::seg_classify_kernel<Key, true, true>), dim3(static_cast<uint32_t>(s.nblocks)), dim3(rsx::kSegClassifyThreads), 0, e->stream,
                       off, nseg, n, e->seg_bsum, e->seg_hdr, e->seg_list, e->seg_large, e->seg_tstart, kin, static_cast<Key*>(nullptr),
                       static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr));
    {
        const uint64_t items = std::max<uint64_t>(nseg, s.max_large);
        const uint64_t grid = std::min<uint64_t>((items + rsx::kTopkInitThreads - 1) / rsx::kTopkInitThreads, cus * 4);
        hipLaunchKernelGGL((rsx::topk_init_kernel<Key>), dim3(static_cast<uint32_t>(grid)), dim3(rsx::kTopkInitThreads), 0, e->stream, off, nseg, n, kin,
                           kout, iout, k, e->seg_hdr, e->topk_state);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);

    // 2. small segments: one workgroup per segment, every pass in LDS, ranks < k stored
    for_each_small_class(nseg, n, cus, [&](int c, uint64_t grid, auto shape) {
        topk_sort_launch<Key, decltype(shape)::THREADS, decltype(shape)::KPT, false>(e, grid, kin, nullptr, kout, iout, off, c, k, both);
    });
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);

    // 3. large segments: select rounds, compaction to k candidates per segment (engine buffers keys[0] / keys[1]), their LDS sort
    if (s.max_large) {
        const uint32_t ntab = static_cast<uint32_t>(s.max_tiles);
        const uint32_t ngroups = (ntab + rsx::kScanTiles - 1) / rsx::kScanTiles;
        const uint32_t hgrid = static_cast<uint32_t>((s.max_tiles + gtiles - 1) / gtiles);
        const uint32_t pgrid = static_cast<uint32_t>(std::min<uint64_t>(s.max_large, cus * 2));
        const uint32_t tgrid = static_cast<uint32_t>(std::min<uint64_t>(s.max_tiles, cus * 8));
        Key* cand = static_cast<Key*>(e->keys[0]);
        uint32_t* cidx = static_cast<uint32_t*>(e->keys[1]);
        const int rounds = static_cast<int>(sizeof(Key)) * 8 / rsx::kTopkDigitBits;
        for (int r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL((rsx::topk_hist_kernel<Key>), dim3(hgrid), dim3(rsx::kTopkThreads), 0, e->stream, kin, e->seg_hdr, e->seg_large, e->seg_tstart,
                               e->topk_state, e->topk_start, e->topk_cont, gtiles, r, both);
            hipLaunchKernelGGL((rsx::topk_pick_kernel<Key>), dim3(pgrid), dim3(rsx::kTopkPickThreads), 0, e->stream, e->seg_hdr, e->seg_tstart, e->topk_state,
                               e->topk_start, e->topk_cont, gtiles, r);
        }
        hipLaunchKernelGGL((rsx::topk_count_kernel<Key>), dim3(tgrid), dim3(rsx::kTopkThreads), 0, e->stream, kin, e->seg_table, e->seg_hdr, e->seg_large,
                           e->seg_tstart, e->topk_state, both);
        launch_table_scan(e, ntab, ngroups);
        hipLaunchKernelGGL((rsx::topk_compact_kernel<Key>), dim3(tgrid), dim3(rsx::kTopkThreads), 0, e->stream, kin, e->seg_table, e->seg_hdr, e->seg_large,
                           e->seg_tstart, e->topk_state, k, cand, cidx, both);
        if (k <= rsx::kSegClass0Max) topk_sort_launch<Key, 64, 4, true>(e, std::min<uint64_t>(s.max_large, cus * 32), cand, cidx, kout, iout, off, 0, k, both);
        else if (k <= rsx::kSegClass1Max) topk_sort_launch<Key, 64, 16, true>(e, std::min<uint64_t>(s.max_large, cus * 16), cand, cidx, kout, iout, off, 0, k, both);
        else topk_sort_launch<Key, 256, 16, true>(e, std::min<uint64_t>(s.max_large, cus * 4), cand, cidx, kout, iout, off, 0, k, both);
        RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    }
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_topk(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, uint32_t k, void* d_keys_out,
                       uint32_t* d_index_out)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_topk: null engine");
    if (n > e->capacity) return fail(RSX_RESIZE_FAILED, "rsx_segmented_topk: beyond capacity");
    if (k == 0 || n == 0 || num_segments == 0) return RSX_OK;
    if (k > rsx::kTopkMaxK) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_topk: k must be at most 4096 (one LDS tile); sort the segments instead (rsx_segmented_sort) and keep their first k keys");
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_topk: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_topk: at most 2^31 keys");
    const SegShape shape = seg_shape(n, num_segments);
    if (shape.max_tiles > static_cast<uint64_t>(rsx::kMaxScanGroups) * rsx::kScanTiles)      // (cannot happen for n <= 2^31: kept as the scan's own bound)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_topk: too many keys for one table scan");
    if (!d_keys || !aligned16(d_keys)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_topk: keys must be a 16-byte aligned device pointer");
    if (!d_keys_out || !d_index_out) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_topk: no output buffer");
    if (!aligned(d_keys_out, e->key_bytes) || !aligned(d_index_out, 4))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_topk: the outputs must be aligned to their element size");
    if (!d_offsets || !aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_topk: offsets must be an 8-byte aligned device pointer");
    const uint64_t kbytes = n * static_cast<uint64_t>(e->key_bytes), obytes = (num_segments + 1) * 8;
    const uint64_t okbytes = num_segments * k * static_cast<uint64_t>(e->key_bytes), oibytes = num_segments * k * 4;
    if (check_buffers(e, "rsx_segmented_topk", {{d_keys_out, okbytes}, {d_index_out, oibytes}}, {{d_keys, kbytes}, {d_offsets, obytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    const int rc = by_key(e, [&](auto key) {
        using Key = decltype(key);
        return topk_enqueue<Key>(e, static_cast<const Key*>(d_keys), n, d_offsets, num_segments, k, static_cast<Key*>(d_keys_out), d_index_out);
    });
    if (rc != RSX_OK) return rc;
    result_is_external(e, n);
    return RSX_OK;
}
