// capi_search.inc — C ABI of the search in sorted segments (rsx_segmented_search, include/radixsort_hip.h): validate the two offsets arrays
// -> one kernel over tiles of 1024 queries.  Kernel: rsx_search.hpp.  Nothing of the engine's sort state is read or written: the call
// needs the first-bad-segment word and the status word, and no scratch at all.
// Included by rsx_capi.hip inside its extern "C" block, after capi_scan.inc.

extern "C++" {
namespace {

template <typename Key>
int search_enqueue(rsx_engine* e, const Key* keys, uint64_t n, const uint64_t* off, uint64_t nseg, const Key* queries, uint64_t nq, const uint64_t* qoff,
                   uint32_t flags, uint32_t* out)
{
    const uint64_t cus = e->num_cus > 0 ? static_cast<uint64_t>(e->num_cus) : 256u;
    // launch bounds from the query and segment counts alone; a workgroup walks `chunk` consecutive tiles (more than one above cus * 16 tiles)
    const uint32_t ntiles = static_cast<uint32_t>((nq + rsx::kSearchTileQ - 1) >> rsx::kSearchTileShift);
    const uint32_t chunk = static_cast<uint32_t>((ntiles + cus * 16 - 1) / (cus * 16));
    const uint32_t tgrid = (ntiles + chunk - 1) / chunk;
    const int rc = ensure_segmented(e, SegShape{1, 0, 0}, 1);     // the status words; none of the sort's scratch
    if (rc != RSX_OK) return rc;
    uint32_t* bad = e->seg_temp + 1;
    hipLaunchKernelGGL(rsx::unique_reset_kernel, dim3(1), dim3(rsx::kWave), 0, e->stream, bad);
    if (off) {
        const uint32_t sgrid = static_cast<uint32_t>(std::min<uint64_t>((nseg + 1 + rsx::kUniqSmallThreads - 1) / rsx::kUniqSmallThreads, cus * 4));
        hipLaunchKernelGGL(rsx::unique_validate_kernel, dim3(sgrid), dim3(rsx::kUniqSmallThreads), 0, e->stream, off, nseg, n, bad);
        if (qoff) hipLaunchKernelGGL(rsx::unique_validate_kernel, dim3(sgrid), dim3(rsx::kUniqSmallThreads), 0, e->stream, qoff, nseg, nq, bad);
    }
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    const uint32_t qper = static_cast<uint32_t>(nq / nseg);       // the even form's queries per segment (nq <= 2^31)
    hipLaunchKernelGGL((rsx::search_kernel<Key>), dim3(tgrid), dim3(rsx::kSearchThreads), 0, e->stream, keys, n, off, nseg, queries, nq, qoff, qper, bad,
                       e->seg_status, ntiles, chunk, flags, e->search_sampled ? 0u : rsx::kSearchNoSampled, a, m, out);
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
    if (!d_queries || (reinterpret_cast<uintptr_t>(d_queries) % kb) != 0)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_search: queries must be a device pointer aligned to the key size");
    if (!d_index_out || (reinterpret_cast<uintptr_t>(d_index_out) & 3u) != 0)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_search: the output must be a 4-byte aligned device pointer");
    if ((reinterpret_cast<uintptr_t>(d_offsets) & 7u) != 0 || (reinterpret_cast<uintptr_t>(d_query_offsets) & 7u) != 0)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_search: offsets must be 8-byte aligned device pointers");
    const uint64_t kbytes = n * kb, qbytes = num_queries * kb, obytes = (num_segments + 1) * 8, ibytes = num_queries * 4;
    const uint64_t ebytes = e->capacity * kb, epbytes = e->capacity * 4;
    const void* bufs[5] = {d_index_out, d_sorted, d_queries, d_offsets, d_query_offsets};
    const uint64_t bytes[5] = {ibytes, kbytes, qbytes, obytes, obytes};
    for (int b = 0; b < 5; ++b) {
        for (int i = 0; i < 2; ++i) {
            if (overlaps(bufs[b], bytes[b], e->keys[i], ebytes) || overlaps(bufs[b], bytes[b], e->perm[i], epbytes))
                return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_search: an input or output overlaps the engine's own buffers");
        }
    }
    for (int b = 1; b < 5; ++b) {
        if (overlaps(d_index_out, ibytes, bufs[b], bytes[b]))
            return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_search: the output overlaps the keys, the queries or the offsets");
    }
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    return RSX_BY_KEY(e, (search_enqueue<uint32_t>(e, static_cast<const uint32_t*>(d_sorted), n, d_offsets, num_segments, static_cast<const uint32_t*>(d_queries),
                                                   num_queries, d_query_offsets, flags, d_index_out)),
                      (search_enqueue<uint64_t>(e, static_cast<const uint64_t*>(d_sorted), n, d_offsets, num_segments, static_cast<const uint64_t*>(d_queries),
                                                num_queries, d_query_offsets, flags, d_index_out)));
}
