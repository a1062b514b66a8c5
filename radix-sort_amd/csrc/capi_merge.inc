// capi_merge.inc — C ABI of the merge of sorted segments (rsx_segmented_merge, include/radixsort_hip.h): validate the two offsets arrays ->
// the merge-path split of every tile boundary (and the output offsets) -> one pass that stages a tile's sources in LDS, merges and
// stores.  Kernels: rsx_merge.hpp.  Nothing of the engine's sort state is read or written: the call needs the first-bad-segment word, the
// status words and one 8-byte split per tile boundary (grown on demand, outside stream captures).
// Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc.

extern "C++" {
namespace {

template <typename Key>
int merge_enqueue(rsx_engine* e, const Key* ka, const uint32_t* pa, uint64_t na, const uint64_t* aoff, const Key* kb, const uint32_t* pb, uint64_t nb,
                  const uint64_t* boff, uint64_t nseg, Key* kout, uint32_t* pout, uint32_t* iout, uint64_t* ooff)
{
    const uint64_t cus = cus_of(e);
    // tiles of 4096 output positions; the tiles behind ooff[S] are dead
    const uint32_t ntiles = static_cast<uint32_t>((na + nb + rsx::kMergeTileKeys - 1) >> rsx::kMergeTileShift);
    const TileChunks c = tile_chunks(ntiles, cus);
    const uint64_t split_items = std::max<uint64_t>(static_cast<uint64_t>(ntiles) + 1, nseg + 1);
    const uint32_t pgrid = static_cast<uint32_t>(std::min<uint64_t>((split_items + rsx::kMergeSplitThreads - 1) / rsx::kMergeSplitThreads, cus * 16));
    int rc = ensure_status_words(e);
    if (rc == RSX_OK) rc = seg_grow(e, &e->merge_split, &e->merge_split_cap, static_cast<uint64_t>(ntiles) + 1, "the per-tile splits of the merge");
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, aoff, na, boff, nb);
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    const rsx::MergeOffsets o{aoff, boff, na, nb, 0, 0};
    hipLaunchKernelGGL((rsx::merge_split_kernel<Key>), dim3(pgrid), dim3(rsx::kMergeSplitThreads), 0, e->stream, ka, kb, o, nseg, a, m, bad, e->seg_status,
                       kStatusCallMerge, ntiles, e->merge_split, ooff);
    if (kout || pout || iout) {
        if (pout) {
            hipLaunchKernelGGL((rsx::merge_kernel<Key, true>), dim3(c.grid), dim3(rsx::kMergeThreads), 0, e->stream, ka, pa, kb, pb, o, nseg, a, m, bad,
                               e->merge_split, ntiles, c.chunk, kout, pout, iout);
        } else {
            hipLaunchKernelGGL((rsx::merge_kernel<Key, false>), dim3(c.grid), dim3(rsx::kMergeThreads), 0, e->stream, ka, pa, kb, pb, o, nseg, a, m, bad,
                               e->merge_split, ntiles, c.chunk, kout, pout, iout);
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
    if (!aligned(d_a_payload, 4) || !aligned(d_b_payload, 4) || !aligned(d_payload_out, 4) || !aligned(d_index_out, 4) || !aligned(d_keys_out, kb))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_merge: the payloads and the outputs must be aligned to their element size");
    if (!aligned(d_a_offsets, 8) || !aligned(d_b_offsets, 8) || !aligned(d_out_offsets, 8))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_merge: offsets must be 8-byte aligned device pointers");
    const uint64_t n = na + nb, obytes = (num_segments + 1) * 8;
    if (check_buffers(e, "rsx_segmented_merge", {{d_keys_out, n * kb}, {d_payload_out, n * 4}, {d_index_out, n * 4}, {d_out_offsets, obytes}},
                      {{d_a, na * kb}, {d_b, nb * kb}, {d_a_payload, na * 4}, {d_b_payload, nb * 4}, {d_a_offsets, obytes}, {d_b_offsets, obytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (n == 0 || num_segments == 0) return RSX_OK;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    return by_key(e, [&](auto key) {
        using Key = decltype(key);
        return merge_enqueue<Key>(e, static_cast<const Key*>(d_a), d_a_payload, na, d_a_offsets, static_cast<const Key*>(d_b), d_b_payload, nb, d_b_offsets, num_segments,
                                  static_cast<Key*>(d_keys_out), d_payload_out, d_index_out, d_out_offsets);
    });
}
