// capi_merge.inc — C ABI of the merge of sorted segments (rsx_segmented_merge, include/radixsort_hip.h): validate the two offsets arrays ->
// the merge-path split of every tile boundary (and the output offsets) -> one pass that stages a tile's sources in LDS, merges and
// stores.  Kernels: rsx_merge.hpp.  Nothing of the engine's sort state is read or written: the call needs the first-bad-segment word, the
// status words and one 8-byte split per tile boundary (grown on demand, outside stream captures).
// Included by rsx_capi.hip inside its extern "C" block, after capi_compact.inc.

extern "C++" {
namespace {

template <typename Key>
int merge_enqueue(rsx_engine* e, const Key* ka, const uint32_t* pa, uint64_t na, const uint64_t* aoff, const Key* kb, const uint32_t* pb, uint64_t nb,
                  const uint64_t* boff, uint64_t nseg, Key* kout, uint32_t* pout, uint32_t* iout, uint64_t* ooff)
{
    const uint64_t cus = e->num_cus > 0 ? static_cast<uint64_t>(e->num_cus) : 256u;
    // launch bounds from na + nb and the segment count alone: tiles of 4096 output positions, a workgroup walks `chunk` consecutive tiles
    // (more than one above cus * 16 tiles); the tiles behind ooff[S] are dead
    const uint32_t ntiles = static_cast<uint32_t>((na + nb + rsx::kMergeTileKeys - 1) >> rsx::kMergeTileShift);
    const uint32_t chunk = static_cast<uint32_t>((ntiles + cus * 16 - 1) / (cus * 16));
    const uint32_t mgrid = (ntiles + chunk - 1) / chunk;
    const uint64_t split_items = std::max<uint64_t>(static_cast<uint64_t>(ntiles) + 1, nseg + 1);
    const uint32_t pgrid = static_cast<uint32_t>(std::min<uint64_t>((split_items + rsx::kMergeSplitThreads - 1) / rsx::kMergeSplitThreads, cus * 16));
    int rc = ensure_segmented(e, SegShape{1, 0, 0}, 1);           // the status words; none of the sort's scratch
    if (rc == RSX_OK) rc = seg_grow(e, &e->merge_split, &e->merge_split_cap, static_cast<uint64_t>(ntiles) + 1, "the per-tile splits of the merge");
    if (rc != RSX_OK) return rc;
    // (a launch, not a non-zero hipMemsetAsync: capi_unique.inc)
    uint32_t* bad = e->seg_temp + 1;
    hipLaunchKernelGGL(rsx::unique_reset_kernel, dim3(1), dim3(rsx::kWave), 0, e->stream, bad);
    if (aoff) {
        const uint32_t sgrid = static_cast<uint32_t>(std::min<uint64_t>((nseg + 1 + rsx::kUniqSmallThreads - 1) / rsx::kUniqSmallThreads, cus * 4));
        hipLaunchKernelGGL(rsx::unique_validate_kernel, dim3(sgrid), dim3(rsx::kUniqSmallThreads), 0, e->stream, aoff, nseg, na, bad);
        hipLaunchKernelGGL(rsx::unique_validate_kernel, dim3(sgrid), dim3(rsx::kUniqSmallThreads), 0, e->stream, boff, nseg, nb, bad);
    }
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    const rsx::MergeOffsets o{aoff, boff, na, nb, 0, 0};
    hipLaunchKernelGGL((rsx::merge_split_kernel<Key>), dim3(pgrid), dim3(rsx::kMergeSplitThreads), 0, e->stream, ka, kb, o, nseg, a, m, bad, e->seg_status,
                       kStatusCallMerge, ntiles, e->merge_split, ooff);
    if (kout || pout || iout) {
        if (pout) {
            hipLaunchKernelGGL((rsx::merge_kernel<Key, true>), dim3(mgrid), dim3(rsx::kMergeThreads), 0, e->stream, ka, pa, kb, pb, o, nseg, a, m, bad,
                               e->merge_split, ntiles, chunk, kout, pout, iout);
        } else {
            hipLaunchKernelGGL((rsx::merge_kernel<Key, false>), dim3(mgrid), dim3(rsx::kMergeThreads), 0, e->stream, ka, pa, kb, pb, o, nseg, a, m, bad,
                               e->merge_split, ntiles, chunk, kout, pout, iout);
        }
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_merge(rsx_engine* e, const void* d_a, const uint32_t* d_a_payload, uint64_t na, const uint64_t* d_a_offsets, const void* d_b,
                        const uint32_t* d_b_payload, uint64_t nb, const uint64_t* d_b_offsets, uint64_t num_segments, uint32_t flags, void* d_keys_out,
                        uint32_t* d_payload_out, uint32_t* d_index_out, uint64_t* d_out_offsets)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_merge: null engine");
    if (flags != 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_merge: unknown flag bits (no flag is defined: flags must be 0)");
    if ((d_a_offsets != nullptr) != (d_b_offsets != nullptr))
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_merge: one offsets array without the other (both NULL is the one segment [0, na) and [0, nb))");
    if (na > (1ull << 31) || nb > (1ull << 31) || na + nb > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_merge: at most 2^31 keys in A, in B and together");
    if (d_a_offsets && num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_merge: at most 2^32 - 2 segments");
    if (!d_keys_out && !d_payload_out && !d_index_out && !d_out_offsets) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_merge: no output requested");
    const int npay = (d_a_payload != nullptr) + (d_b_payload != nullptr) + (d_payload_out != nullptr);
    if (npay != 0 && npay != 3)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_merge: the two payload inputs and the payload output must be all given or all NULL");
    if (!d_a_offsets) num_segments = 1;
    const uint64_t kb = static_cast<uint64_t>(e->key_bytes);
    if ((na > 0 && !d_a) || (nb > 0 && !d_b) || !aligned16(d_a) || !aligned16(d_b))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_merge: d_a and d_b must be 16-byte aligned device pointers");
    if ((reinterpret_cast<uintptr_t>(d_a_payload) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_b_payload) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(d_payload_out) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_index_out) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(d_keys_out) % kb) != 0)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_merge: the payloads and the outputs must be aligned to their element size");
    if ((reinterpret_cast<uintptr_t>(d_a_offsets) & 7u) != 0 || (reinterpret_cast<uintptr_t>(d_b_offsets) & 7u) != 0 ||
        (reinterpret_cast<uintptr_t>(d_out_offsets) & 7u) != 0)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_merge: offsets must be 8-byte aligned device pointers");
    const uint64_t n = na + nb, obytes = (num_segments + 1) * 8;
    const uint64_t ebytes = e->capacity * kb, epbytes = e->capacity * 4;
    const void* bufs[10] = {d_keys_out, d_payload_out, d_index_out, d_out_offsets, d_a, d_b, d_a_payload, d_b_payload, d_a_offsets, d_b_offsets};       // outputs first
    const uint64_t bytes[10] = {n * kb, n * 4, n * 4, obytes, na * kb, nb * kb, na * 4, nb * 4, obytes, obytes};
    for (int b = 0; b < 10; ++b) {
        for (int i = 0; i < 2; ++i) {
            if (overlaps(bufs[b], bytes[b], e->keys[i], ebytes) || overlaps(bufs[b], bytes[b], e->perm[i], epbytes))
                return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_merge: an input or output overlaps the engine's own buffers");
        }
    }
    for (int a = 0; a < 4; ++a) {
        for (int b = a + 1; b < 10; ++b) {
            if (overlaps(bufs[a], bytes[a], bufs[b], bytes[b]))
                return fail(RSX_HOST_BUFFERS_FAILED, b < 4 ? "rsx_segmented_merge: two outputs overlap"
                                                           : "rsx_segmented_merge: an output overlaps an input (there is no in-place form)");
        }
    }
    if (n == 0 || num_segments == 0) return RSX_OK;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    return RSX_BY_KEY(e, (merge_enqueue<uint32_t>(e, static_cast<const uint32_t*>(d_a), d_a_payload, na, d_a_offsets, static_cast<const uint32_t*>(d_b), d_b_payload,
                                                  nb, d_b_offsets, num_segments, static_cast<uint32_t*>(d_keys_out), d_payload_out, d_index_out, d_out_offsets)),
                      (merge_enqueue<uint64_t>(e, static_cast<const uint64_t*>(d_a), d_a_payload, na, d_a_offsets, static_cast<const uint64_t*>(d_b), d_b_payload,
                                               nb, d_b_offsets, num_segments, static_cast<uint64_t*>(d_keys_out), d_payload_out, d_index_out, d_out_offsets)));
}
