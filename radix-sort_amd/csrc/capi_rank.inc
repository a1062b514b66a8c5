// capi_rank.inc — C ABI of the segmented rank (rsx_segmented_rank, include/radixsort_hip.h): validate the offsets -> one-key segments ->
// small segments (2..4096 keys) ranked inside LDS, one workgroup each -> large segments grouped by the segmented chain (the flat product
// chain when d_offsets is NULL) with generated positions as payload into the engine's own buffers -> heads per sorted tile -> the carries
// per large segment -> ranks scattered to the positions.  Kernels: rsx_rank.hpp; the rules: rsx_rank_math.hpp.
// Included by rsx_capi.hip inside its extern "C" block, after capi_unique.inc (whose grouping steps it follows).

extern "C++" {
namespace {

template <typename Key>
int rank_enqueue(rsx_engine* e, const Key* kin, uint64_t n, const uint64_t* off, uint64_t nseg, uint32_t method, uint32_t* rout, uint32_t* tout)
{
    const bool flat = !off;
    const uint64_t cus = cus_of(e);
    const SegShape shape = flat ? SegShape{1, 1, (n + rsx::kSegTileKeys - 1) / rsx::kSegTileKeys} : seg_shape(n, nseg);
    int rc = ensure_segmented(e, shape, nseg);
    if (rc == RSX_OK && shape.max_large && (e->uniq_iota_cap < n || !e->uniq_iota)) {          // the positions: as unique_groups_enqueue
        rc = seg_grow(e, &e->uniq_iota, &e->uniq_iota_cap, e->capacity, "the positions");
        if (rc == RSX_OK) {
            const uint64_t grid = std::min<uint64_t>((e->uniq_iota_cap + rsx::kUniqSmallThreads - 1) / rsx::kUniqSmallThreads, cus * 8);
            hipLaunchKernelGGL(rsx::unique_iota_kernel, dim3(static_cast<uint32_t>(grid)), dim3(rsx::kUniqSmallThreads), 0, e->stream, e->uniq_iota,
                               e->uniq_iota_cap);
        }
    }
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, off, n);
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    const int passes = static_cast<int>(e->passes());

    // 1. group the large segments: sorted keys and the positions they came from end up in the engine's own buffers
    const Key* skeys = nullptr;
    const uint32_t* sperm = nullptr;
    if (flat) {
        const SortJob job{kin, e->uniq_iota, n, 0, passes, 0, passes, nullptr, nullptr, true};
        rc = sort_chain<Key>(e, job);
        if (rc != RSX_OK) return rc;
        skeys = static_cast<const Key*>(e->result_keys);
        sperm = e->result_perm;
        hipLaunchKernelGGL(rsx::rank_flat_kernel, dim3(1), dim3(rsx::kWave), 0, e->stream, e->seg_hdr, e->seg_large, e->seg_tstart, n);
    } else {
        // (before the chain, whose scan reports a bad segment without a name when no report is pending)
        hipLaunchKernelGGL(rsx::rank_ones_kernel, dim3(offsets_grid(nseg, cus)), dim3(rsx::kRankSmallThreads), 0, e->stream, off, nseg, bad, rout, tout,
                           e->seg_status, kStatusCallRank);
        rc = segmented_enqueue<Key>(e, kin, e->uniq_iota, n, off, nseg, static_cast<Key*>(e->keys[1]), e->perm[1], true, false);
        if (rc != RSX_OK) return rc;
        skeys = static_cast<const Key*>(e->keys[1]);
        sperm = e->perm[1];

        // 2. small segments: one workgroup per segment, sort and ranks in LDS
        for_each_small_class(nseg, n, cus, [&](int c, uint64_t grid, auto sshape) {
            constexpr int T = decltype(sshape)::THREADS, K = decltype(sshape)::KPT;
            constexpr size_t lds = rsx::SegSortLayout<Key, T, K>::BYTES;
            hipLaunchKernelGGL((rsx::rank_small_kernel<Key, T, K>), dim3(static_cast<uint32_t>(grid)), dim3(T), lds, e->stream, kin, off, e->seg_list, e->seg_hdr,
                               bad, c, passes, a, m, method, rout, tout);
        });
    }

    // 3. large segments: heads per tile, carries per segment, ranks to the positions
    if (shape.max_large) {
        const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(shape.max_tiles, cus * 8));
        const uint32_t jgrid = static_cast<uint32_t>(std::min<uint64_t>(shape.max_large, cus * 8));
        hipLaunchKernelGGL((rsx::rank_edge_kernel<Key>), dim3(grid), dim3(rsx::kRankThreads), 0, e->stream, skeys, bad, e->seg_hdr, e->seg_large, e->seg_tstart,
                           e->seg_table);
        hipLaunchKernelGGL(rsx::rank_join_kernel, dim3(jgrid), dim3(rsx::kRankThreads), 0, e->stream, bad, e->seg_hdr, e->seg_large, e->seg_tstart, e->seg_table);
        hipLaunchKernelGGL((rsx::rank_write_kernel<Key>), dim3(grid), dim3(rsx::kRankThreads), 0, e->stream, skeys, sperm, n, bad, e->seg_hdr, e->seg_large,
                           e->seg_tstart, e->seg_table, method, rout, tout);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_rank(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, uint32_t flags, uint32_t method,
                       uint32_t* d_rank_out, uint32_t* d_ties_out)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_rank: null engine");
    if (flags != 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_rank: flags must be 0");
    if (method > RSX_RANK_AVERAGE) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_rank: method must be RSX_RANK_ORDINAL (0) .. RSX_RANK_AVERAGE (4)");
    if (!e->has_payload)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_rank: the positions travel through the sort of large segments as its payload: "
                                             "the call needs an engine created with has_payload = 1");
    if (n > e->capacity) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_rank: n is beyond the engine's capacity");
    if (n == 0 || (d_offsets && num_segments == 0)) return RSX_OK;
    if (!d_offsets) num_segments = 1;
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_rank: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_rank: at most 2^31 keys");
    if (!d_keys || !aligned16(d_keys)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_rank: keys must be a 16-byte aligned device pointer");
    if (!d_rank_out || !aligned(d_rank_out, 4)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_rank: the rank output must be a 4-byte aligned device pointer");
    if (!aligned(d_ties_out, 4)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_rank: the ties output must be 4-byte aligned");
    if (!aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_rank: offsets must be an 8-byte aligned device pointer");
    const uint64_t kbytes = n * static_cast<uint64_t>(e->key_bytes), obytes = d_offsets ? (num_segments + 1) * 8 : 0, ibytes = n * 4;
    if (check_buffers(e, "rsx_segmented_rank", {{d_rank_out, ibytes}, {d_ties_out, d_ties_out ? ibytes : 0}}, {{d_keys, kbytes}, {d_offsets, obytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    const int rc = by_key(e, [&](auto key) {
        using Key = decltype(key);
        return rank_enqueue<Key>(e, static_cast<const Key*>(d_keys), n, d_offsets, num_segments, method, d_rank_out, d_ties_out);
    });
    result_is_external(e, n);       // (whatever rc says: a chain that failed half way has still used the engine's buffers)
    return rc;
}
