// capi_search.inc — C ABI of the search in sorted segments (rsx_segmented_search, include/radixsort_hip.h): validate the two offsets arrays
// -> one kernel over tiles of 1024 queries.  Kernel: rsx_search.hpp.  Nothing of the engine's sort state is read or written: the call
// needs the first-bad-segment word and the status word, and no scratch at all.
// Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc.

extern "C++" {
namespace {

template <typename Key>
int search_enqueue(rsx_engine* e, const Key* keys, uint64_t n, const uint64_t* off, uint64_t nseg, const Key* queries, uint64_t nq, const uint64_t* qoff,
                   uint32_t flags, uint32_t* out)
{
    const uint64_t cus = cus_of(e);
    const uint32_t ntiles = static_cast<uint32_t>((nq + rsx::kSearchTileQ - 1) >> rsx::kSearchTileShift);
    const TileChunks c = tile_chunks(ntiles, cus);
    const int rc = ensure_status_words(e);
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, off, n, qoff, nq);
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    const uint32_t qper = static_cast<uint32_t>(nq / nseg);       // the even form's queries per segment (nq <= 2^31)
    hipLaunchKernelGGL((rsx::search_kernel<Key>), dim3(c.grid), dim3(rsx::kSearchThreads), 0, e->stream, keys, n, off, nseg, queries, nq, qoff, qper, bad,
                       e->seg_status, ntiles, c.chunk, flags, e->search_sampled ? 0u : rsx::kSearchNoSampled, a, m, out);
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_search(rsx_engine* e, const void* d_sorted, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, const void* d_queries,
                         uint64_t num_queries, const uint64_t* d_query_offsets, uint32_t flags, uint32_t* d_index_out)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_search: null engine");
    if ((flags & ~static_cast<uint32_t>(RSX_SEARCH_RIGHT)) != 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_search: unknown flag bits (RSX_SEARCH_RIGHT or none)");
    if (d_query_offsets && !d_offsets)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_search: query offsets without haystack offsets (d_offsets == NULL is the one segment [0, n) with the queries [0, num_queries))");
    if (num_queries == 0 || (d_offsets && num_segments == 0)) return RSX_OK;
    if (!d_offsets) num_segments = 1;
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_search: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_search: at most 2^31 keys");
    if (num_queries > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_search: at most 2^31 queries");
    if (d_offsets && !d_query_offsets && num_queries % num_segments != 0)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_search: without query offsets every segment has num_queries / num_segments queries, and num_queries is no multiple of num_segments");
    const uint64_t kb = static_cast<uint64_t>(e->key_bytes);
    if ((n > 0 && !d_sorted) || !aligned16(d_sorted)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_search: the sorted keys must be a 16-byte aligned device pointer");
    if (!d_queries || !aligned(d_queries, kb))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_search: queries must be a device pointer aligned to the key size");
    if (!d_index_out || !aligned(d_index_out, 4))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_search: the output must be a 4-byte aligned device pointer");
    if (!aligned(d_offsets, 8) || !aligned(d_query_offsets, 8))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_search: offsets must be 8-byte aligned device pointers");
    const uint64_t kbytes = n * kb, qbytes = num_queries * kb, obytes = (num_segments + 1) * 8, ibytes = num_queries * 4;
    if (check_buffers(e, "rsx_segmented_search", {{d_index_out, ibytes}},
                      {{d_sorted, kbytes}, {d_queries, qbytes}, {d_offsets, obytes}, {d_query_offsets, obytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    return by_key(e, [&](auto key) {
        using Key = decltype(key);
        return search_enqueue<Key>(e, static_cast<const Key*>(d_sorted), n, d_offsets, num_segments, static_cast<const Key*>(d_queries), num_queries,
                                   d_query_offsets, flags, d_index_out);
    });
}
