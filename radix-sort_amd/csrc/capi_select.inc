// capi_select.inc — C ABI of the segmented select (rsx_segmented_select, include/radixsort_hip.h): the segmented sort's classify chain ->
// small segments sorted in LDS (the image slots named by the ranks stored) -> radix select over the tiles of all large segments for up
// to 8 ranks per segment at once, a tie count per tile, the table scan, and a locate pass.  Kernels: rsx_select.hpp.
// Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc and capi_topk.inc (whose group sizing and scratch fields it shares).

extern "C++" {
namespace {

// The top-k's scratch, R times: one select state and one START row per (large segment, q), one CONT row per (group, q).
int ensure_select(rsx_engine* e, const SegShape& s, uint32_t gtiles, uint32_t R)
{
    int rc = RSX_OK;
    if (!s.max_large) return rc;
    const uint64_t groups = (s.max_tiles + gtiles - 1) / gtiles;
    rc = seg_grow(e, &e->topk_state, &e->topk_state_cap, s.max_large * R, "the select state");
    if (rc == RSX_OK) rc = seg_grow(e, &e->topk_start, &e->topk_start_cap, s.max_large * R * rsx::kTopkBins, "the select segment counts");
    if (rc == RSX_OK) rc = seg_grow(e, &e->topk_cont, &e->topk_cont_cap, groups * R * rsx::kTopkBins, "the select group counts");
    return rc;
}

template <typename Key, int THREADS, int KPT>
void select_sort_launch(rsx_engine* e, uint64_t grid, const Key* in, const uint32_t* ranks, uint32_t R, Key* kout, uint32_t* iout, const uint64_t* off,
                        int cls, const rsx::KeyCodec<Key>& codec)
{
    constexpr size_t lds = rsx::SegSortLayout<Key, THREADS, KPT>::BYTES;
    hipLaunchKernelGGL((rsx::select_sort_kernel<Key, THREADS, KPT>), dim3(static_cast<uint32_t>(grid)), dim3(THREADS), lds, e->stream, in, ranks, R, kout,
                       iout, off, e->seg_list, e->seg_hdr, cls, static_cast<int>(e->passes()), codec);
}

// The per-key kernels of the large-segment chain for a compiled rank capacity RC >= R.
template <typename Key, int RC>
void select_large_launch(rsx_engine* e, const Key* kin, uint32_t R, uint32_t gtiles, uint32_t hgrid, uint32_t pgrid, uint32_t tgrid, uint32_t ntab,
                         Key* kout, uint32_t* iout, const rsx::KeyCodec<Key>& both)
{
    const uint32_t ngroups = (ntab + rsx::kScanTiles - 1) / rsx::kScanTiles;
    const int rounds = static_cast<int>(sizeof(Key)) * 8 / rsx::kTopkDigitBits;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL((rsx::select_hist_kernel<Key, RC>), dim3(hgrid), dim3(rsx::kTopkThreads), 0, e->stream, kin, e->seg_hdr, e->seg_large,
                           e->seg_tstart, e->topk_state, e->topk_start, e->topk_cont, gtiles, r, R, both);
        hipLaunchKernelGGL((rsx::select_pick_kernel<Key>), dim3(pgrid), dim3(rsx::kTopkPickThreads), 0, e->stream, e->seg_hdr, e->seg_tstart,
                           e->topk_state, e->topk_start, e->topk_cont, gtiles, r, R);
    }
    hipLaunchKernelGGL((rsx::select_count_kernel<Key, RC>), dim3(tgrid), dim3(rsx::kTopkThreads), 0, e->stream, kin, e->seg_table, e->seg_hdr,
                       e->seg_large, e->seg_tstart, e->topk_state, R, both);
    launch_table_scan(e, ntab, ngroups);
    hipLaunchKernelGGL((rsx::select_locate_kernel<Key>), dim3(tgrid), dim3(rsx::kTopkThreads), 0, e->stream, kin, e->seg_table, e->seg_hdr, e->seg_large,
                       e->seg_tstart, e->topk_state, R, kout, iout, both);
}

template <typename Key>
int select_enqueue(rsx_engine* e, const Key* kin, uint64_t n, const uint64_t* off, uint64_t nseg, const uint32_t* ranks, uint32_t R, Key* kout,
                   uint32_t* iout)
{
    const SegShape s = seg_shape(n, nseg);
    const uint64_t cus = cus_of(e);
    const uint32_t gtiles = topk_group_tiles(s, cus);
    int rc = ensure_segmented(e, s, nseg);
    if (rc == RSX_OK) rc = ensure_select(e, s, gtiles, R);
    if (rc != RSX_OK) return rc;
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    const rsx::KeyCodec<Key> both{a, m, a, m};

    // 1. classify as the top-k does, then one-key segments and the select state of every (large segment, q)
    hipLaunchKernelGGL((rsx::seg_classify_kernel<Key, false>), dim3(static_cast<uint32_t>(s.nblocks)), dim3(rsx::kSegClassifyThreads), 0, e->stream,
                       off, nseg, n, e->seg_bsum, e->seg_hdr, e->seg_list, e->seg_large, e->seg_tstart, kin, static_cast<Key*>(nullptr),
                       static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr));
    hipLaunchKernelGGL(rsx::seg_scan_kernel, dim3(1), dim3(rsx::kSegScanThreads), 0, e->stream, e->seg_bsum, static_cast<uint32_t>(s.nblocks), e->seg_hdr,
                       e->seg_tstart, n, s.max_large, s.max_tiles, e->seg_status);
    hipLaunchKernelGGL((rsx::seg_classify_kernel<Key, true, true>), dim3(static_cast<uint32_t>(s.nblocks)), dim3(rsx::kSegClassifyThreads), 0, e->stream,
                       off, nseg, n, e->seg_bsum, e->seg_hdr, e->seg_list, e->seg_large, e->seg_tstart, kin, static_cast<Key*>(nullptr),
                       static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr));
    {
        const uint64_t items = std::max<uint64_t>(nseg, s.max_large * R);
        const uint64_t grid = std::min<uint64_t>((items + rsx::kTopkInitThreads - 1) / rsx::kTopkInitThreads, cus * 4);
        hipLaunchKernelGGL((rsx::select_init_kernel<Key>), dim3(static_cast<uint32_t>(grid)), dim3(rsx::kTopkInitThreads), 0, e->stream, off, nseg, n, kin,
                           ranks, R, kout, iout, e->seg_hdr, e->seg_large, e->topk_state);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);

    // 2. small segments: one workgroup per segment, every pass in LDS, the ranked image slots stored
    for_each_small_class(nseg, n, cus, [&](int c, uint64_t grid, auto shape) {
        select_sort_launch<Key, decltype(shape)::THREADS, decltype(shape)::KPT>(e, grid, kin, ranks, R, kout, iout, off, c, both);
    });
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);

    // 3. large segments: select rounds for all R ranks at once, tie counts per tile, the table scan, locate
    if (s.max_large) {
        const uint32_t ntab = static_cast<uint32_t>(s.max_tiles);
        const uint32_t hgrid = static_cast<uint32_t>((s.max_tiles + gtiles - 1) / gtiles);
        const uint32_t pgrid = static_cast<uint32_t>(std::min<uint64_t>(s.max_large * R, cus * 2));
        const uint32_t tgrid = static_cast<uint32_t>(std::min<uint64_t>(s.max_tiles, cus * 8));
        if (R == 1) select_large_launch<Key, 1>(e, kin, R, gtiles, hgrid, pgrid, tgrid, ntab, kout, iout, both);
        else if (R == 2) select_large_launch<Key, 2>(e, kin, R, gtiles, hgrid, pgrid, tgrid, ntab, kout, iout, both);
        else if (R <= 4) select_large_launch<Key, 4>(e, kin, R, gtiles, hgrid, pgrid, tgrid, ntab, kout, iout, both);
        else select_large_launch<Key, 8>(e, kin, R, gtiles, hgrid, pgrid, tgrid, ntab, kout, iout, both);
        RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    }
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_select(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, const uint32_t* d_ranks,
                         uint32_t ranks_per_segment, void* d_keys_out, uint32_t* d_index_out)
{
    const uint32_t R = ranks_per_segment;
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_select: null engine");
    if (n > e->capacity) return fail(RSX_RESIZE_FAILED, "rsx_segmented_select: beyond capacity");
    if (R == 0 || n == 0 || num_segments == 0) return RSX_OK;
    if (R > rsx::kSelectMaxRanks) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_select: at most 8 ranks per segment; call again for further ranks, or sort the segments instead (rsx_segmented_sort) and index the result");
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_select: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_select: at most 2^31 keys");
    const SegShape shape = seg_shape(n, num_segments);
    if (shape.max_tiles > static_cast<uint64_t>(rsx::kMaxScanGroups) * rsx::kScanTiles)      // (cannot happen for n <= 2^31: kept as the scan's own bound)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_select: too many keys for one table scan");
    if (!d_keys || !aligned16(d_keys)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_select: keys must be a 16-byte aligned device pointer");
    if (!d_keys_out || !d_index_out) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_select: no output buffer");
    if (!aligned(d_keys_out, e->key_bytes) || !aligned(d_index_out, 4))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_select: the outputs must be aligned to their element size");
    if (!d_offsets || !aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_select: offsets must be an 8-byte aligned device pointer");
    if (!d_ranks || !aligned(d_ranks, 4)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_select: ranks must be a 4-byte aligned device pointer");
    const uint64_t kbytes = n * static_cast<uint64_t>(e->key_bytes), obytes = (num_segments + 1) * 8, rbytes = num_segments * R * 4;
    const uint64_t okbytes = num_segments * R * static_cast<uint64_t>(e->key_bytes), oibytes = num_segments * R * 4;
    if (check_buffers(e, "rsx_segmented_select", {{d_keys_out, okbytes}, {d_index_out, oibytes}}, {{d_keys, kbytes}, {d_offsets, obytes}, {d_ranks, rbytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    const int rc = by_key(e, [&](auto key) {
        using Key = decltype(key);
        return select_enqueue<Key>(e, static_cast<const Key*>(d_keys), n, d_offsets, num_segments, d_ranks, R, static_cast<Key*>(d_keys_out), d_index_out);
    });
    if (rc != RSX_OK) return rc;
    result_is_external(e, n);
    return RSX_OK;
}
