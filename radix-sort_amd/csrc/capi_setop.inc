// capi_setop.inc — C ABI of the set operations on sorted segments (rsx_segmented_set_op, include/radixsort_hip.h): validate the two offsets
// arrays -> the merge's split of every tile boundary -> kept elements per tile of merged positions -> the flat table scan -> kept offsets
// -> the kept elements ranked in LDS and stored.  Kernels: rsx_setop.hpp.  Nothing of the engine's sort state is read or written: the call
// needs the first-bad-segment word, the status words, one 8-byte split per tile boundary and one table entry per tile (the merge's splits
// and the compaction's table and group sums, grown on demand, outside stream captures).
// Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc and capi_merge.inc (whose status ids it continues).

extern "C++" {
namespace {

template <typename Key, bool PAYLOAD>
void setop_write_launch(rsx_engine* e, uint32_t grid, const rsx::SetopArgs<Key>& g, const uint32_t* bad, uint32_t ntiles, uint32_t chunk, uint32_t cap, Key* kout,
                        uint32_t* pout, uint32_t* iout, uint32_t* mout)
{
    if (mout) {
        hipLaunchKernelGGL((rsx::setop_write_kernel<Key, PAYLOAD, 2>), dim3(grid), dim3(rsx::kMergeThreads), 0, e->stream, g, bad, e->seg_table, ntiles, chunk, cap,
                           kout, pout, iout, mout);
    } else if (iout) {
        hipLaunchKernelGGL((rsx::setop_write_kernel<Key, PAYLOAD, 1>), dim3(grid), dim3(rsx::kMergeThreads), 0, e->stream, g, bad, e->seg_table, ntiles, chunk, cap,
                           kout, pout, iout, mout);
    } else {
        hipLaunchKernelGGL((rsx::setop_write_kernel<Key, PAYLOAD, 0>), dim3(grid), dim3(rsx::kMergeThreads), 0, e->stream, g, bad, e->seg_table, ntiles, chunk, cap,
                           kout, pout, iout, mout);
    }
}

template <typename Key>
int setop_enqueue(rsx_engine* e, const Key* ka, const uint32_t* pa, uint64_t na, const uint64_t* aoff, const Key* kb, const uint32_t* pb, uint64_t nb,
                  const uint64_t* boff, uint64_t nseg, uint32_t op, uint64_t cap, Key* kout, uint32_t* pout, uint32_t* iout, uint32_t* mout, uint64_t* koff)
{
    const uint64_t cus = cus_of(e);
    // the merge's tiles of 4096 merged positions, the compaction's table of one entry per tile and one more
    const TileTable t = tile_table(na + nb, rsx::kMergeTileShift, cus);
    const uint64_t split_items = std::max<uint64_t>(static_cast<uint64_t>(t.ntiles) + 1, nseg + 1);
    const uint32_t pgrid = static_cast<uint32_t>(std::min<uint64_t>((split_items + rsx::kMergeSplitThreads - 1) / rsx::kMergeSplitThreads, cus * 16));
    int rc = ensure_status_words(e);
    if (rc == RSX_OK) rc = seg_grow(e, &e->merge_split, &e->merge_split_cap, static_cast<uint64_t>(t.ntiles) + 1, "the per-tile splits of the set operation");
    if (rc == RSX_OK) rc = grow_tile_table(e, t, "the per-tile table of the set operation");
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, aoff, na, boff, nb);
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    const rsx::MergeOffsets o{aoff, boff, na, nb, 0, 0};
    // the merge's split, unchanged; it writes no offsets here (the kept offsets are this call's) and reports a bad segment under this call's id
    hipLaunchKernelGGL((rsx::merge_split_kernel<Key>), dim3(pgrid), dim3(rsx::kMergeSplitThreads), 0, e->stream, ka, kb, o, nseg, a, m, bad, e->seg_status,
                       kStatusCallSetop, t.ntiles, e->merge_split, static_cast<uint64_t*>(nullptr));
    const rsx::SetopArgs<Key> g{ka, pa, kb, pb, o, nseg, a, m, op, e->merge_split};
    // 1. kept elements per tile, their flat exclusive scan, the kept offsets (zeros on a bad segment)
    hipLaunchKernelGGL((rsx::setop_count_kernel<Key>), dim3(t.tgrid), dim3(rsx::kMergeThreads), 0, e->stream, g, bad, e->seg_table, t.ntab, t.npad, t.chunk, koff);
    launch_table_scan(e, t.nrow, t.ngroups);
    hipLaunchKernelGGL(rsx::setop_offsets_kernel, dim3(offsets_grid(nseg, cus)), dim3(rsx::kUniqSmallThreads), 0, e->stream, o, nseg, bad, e->seg_table, cap, koff);
    // 2. the kept elements, ranked and stored
    if (kout || pout || iout || mout) {
        if (pout) setop_write_launch<Key, true>(e, t.wgrid, g, bad, t.ntiles, t.chunk, static_cast<uint32_t>(cap), kout, pout, iout, mout);
        else setop_write_launch<Key, false>(e, t.wgrid, g, bad, t.ntiles, t.chunk, static_cast<uint32_t>(cap), kout, pout, iout, mout);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_set_op(rsx_engine* e, const void* d_a, const uint32_t* d_a_payload, uint64_t na, const uint64_t* d_a_offsets, const void* d_b,
                         const uint32_t* d_b_payload, uint64_t nb, const uint64_t* d_b_offsets, uint64_t num_segments, uint32_t op, uint32_t flags,
                         void* d_keys_out, uint32_t* d_payload_out, uint32_t* d_index_out, uint32_t* d_match_out, uint64_t* d_out_offsets)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_set_op: null engine");
    if (op > RSX_SET_SYMMETRIC_DIFFERENCE)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_set_op: unknown op (RSX_SET_INTERSECTION, _DIFFERENCE, _UNION or _SYMMETRIC_DIFFERENCE)");
    if (flags != 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_set_op: unknown flag bits (no flag is defined: flags must be 0)");
    if (d_match_out && op != RSX_SET_INTERSECTION)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_set_op: d_match_out belongs to RSX_SET_INTERSECTION (no other op pairs its outputs with B)");
    if ((d_a_offsets != nullptr) != (d_b_offsets != nullptr))
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_set_op: one offsets array without the other (both NULL is the one segment [0, na) and [0, nb))");
    if (na > (1ull << 31) || nb > (1ull << 31) || na + nb > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_set_op: at most 2^31 keys in A, in B and together");
    if (d_a_offsets && num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_set_op: at most 2^32 - 2 segments");
    const int npay = (d_a_payload != nullptr) + (d_b_payload != nullptr) + (d_payload_out != nullptr);
    if (npay != 0 && npay != 3)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_set_op: the two payload inputs and the payload output must be all given or all NULL");
    if (!d_out_offsets) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_set_op: d_out_offsets is required (it alone says how many elements were kept)");
    if (!d_a_offsets) num_segments = 1;
    const uint64_t kb = static_cast<uint64_t>(e->key_bytes);
    if ((na > 0 && !d_a) || (nb > 0 && !d_b) || !aligned16(d_a) || !aligned16(d_b))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_set_op: d_a and d_b must be 16-byte aligned device pointers");
    if (!aligned(d_a_payload, 4) || !aligned(d_b_payload, 4) || !aligned(d_payload_out, 4) || !aligned(d_index_out, 4) || !aligned(d_match_out, 4) ||
        !aligned(d_keys_out, kb))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_set_op: the payloads and the outputs must be aligned to their element size");
    if (!aligned(d_a_offsets, 8) || !aligned(d_b_offsets, 8) || !aligned(d_out_offsets, 8))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_set_op: offsets must be 8-byte aligned device pointers");
    // what the caller provides: na elements for what only A can supply, na + nb otherwise
    const uint64_t cap = op == RSX_SET_INTERSECTION || op == RSX_SET_DIFFERENCE ? na : na + nb;
    const uint64_t obytes = (num_segments + 1) * 8;
    if (check_buffers(e, "rsx_segmented_set_op",
                      {{d_keys_out, cap * kb}, {d_payload_out, cap * 4}, {d_index_out, cap * 4}, {d_match_out, cap * 4}, {d_out_offsets, obytes}},
                      {{d_a, na * kb}, {d_b, nb * kb}, {d_a_payload, na * 4}, {d_b_payload, nb * 4}, {d_a_offsets, obytes}, {d_b_offsets, obytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (na + nb == 0 || num_segments == 0) return RSX_OK;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    return by_key(e, [&](auto key) {
        using Key = decltype(key);
        return setop_enqueue<Key>(e, static_cast<const Key*>(d_a), d_a_payload, na, d_a_offsets, static_cast<const Key*>(d_b), d_b_payload, nb, d_b_offsets,
                                  num_segments, op, cap, static_cast<Key*>(d_keys_out), d_payload_out, d_index_out, d_match_out, d_out_offsets);
    });
}
