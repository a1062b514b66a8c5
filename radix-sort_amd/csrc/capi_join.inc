// capi_join.inc — C ABI of the equi-join of sorted segments (rsx_segmented_join, include/radixsort_hip.h): validate the two offsets arrays
// -> rows per A element and their 64-bit prefix inside every tile of 4096 A positions -> the 64-bit scan of the tile totals -> the row
// offsets -> (unless the call only counts) the owner of every boundary of the 4096-row output grid -> per output tile the A position and
// the rank of every row.  Kernels: rsx_join.hpp.  Nothing of the engine's sort state is read or written: the call needs the
// first-bad-segment word, the status words and scratch of its own (12 to 16 bytes per A position, 8 per A tile, 4 per output tile), grown
// on demand, outside stream captures.  Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc.

extern "C++" {
namespace {

template <typename Key>
int join_enqueue(rsx_engine* e, const Key* ka, uint64_t na, const uint64_t* aoff, const Key* kb, uint64_t nb, const uint64_t* boff, uint64_t nseg, uint32_t op,
                 uint64_t cap, Key* kout, uint32_t* aout, uint32_t* bout, uint64_t* ooff)
{
    const uint64_t cus = cus_of(e);
    const bool write = kout || aout || bout;
    const uint32_t ntiles = static_cast<uint32_t>((na + rsx_join::kTileSlots - 1) >> rsx_join::kTileShift);
    const uint64_t npos = static_cast<uint64_t>(ntiles) << rsx_join::kTileShift;
    // output tiles: from the capacity and from what na and nb allow, never from the data
    const uint64_t rows = write ? std::min<uint64_t>(cap, rsx_join::row_bound(na, nb, op)) : 0;
    const uint32_t nout = static_cast<uint32_t>((rows + rsx_join::kTileSlots - 1) >> rsx_join::kTileShift);
    const bool want_first = bout != nullptr, want_arel = aout != nullptr && aoff != nullptr;
    int rc = ensure_status_words(e);
    if (rc == RSX_OK) rc = seg_grow(e, &e->join_pre, &e->join_pre_cap, npos, "the row prefixes of the segmented join");
    if (rc == RSX_OK) rc = seg_grow(e, &e->join_tbase, &e->join_tbase_cap, static_cast<uint64_t>(ntiles) + 1, "the tile bases of the segmented join");
    if (rc == RSX_OK && want_first) rc = seg_grow(e, &e->join_first, &e->join_first_cap, npos, "the first partners of the segmented join");
    if (rc == RSX_OK && want_arel) rc = seg_grow(e, &e->join_arel, &e->join_arel_cap, npos, "the A positions of the segmented join");
    if (rc == RSX_OK && write) rc = seg_grow(e, &e->join_split, &e->join_split_cap, static_cast<uint64_t>(nout) + 1, "the output tile splits of the segmented join");
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, aoff, na, boff, nb);
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    // 1. rows per A element, in-tile prefixes, tile totals; their scan; the offsets (zeros and the report on a bad segment)
    if (ntiles) {
        const TileChunks c = tile_chunks(ntiles, cus);
        hipLaunchKernelGGL((rsx::join_count_kernel<Key>), dim3(c.grid), dim3(rsx::kJoinThreads), 0, e->stream, ka, na, aoff, kb, nb, boff, nseg, bad, ntiles, c.chunk,
                           op, a, m, want_first ? e->join_first : static_cast<uint32_t*>(nullptr), e->join_pre,
                           want_arel ? e->join_arel : static_cast<uint32_t*>(nullptr), e->join_tbase);
    }
    hipLaunchKernelGGL(rsx::join_scan_kernel, dim3(1), dim3(rsx::kJoinScanThreads), 0, e->stream, e->join_tbase, ntiles, bad);
    hipLaunchKernelGGL(rsx::join_offsets_kernel, dim3(offsets_grid(nseg, cus)), dim3(rsx::kExpandSmallThreads), 0, e->stream, aoff, na, nseg, bad, e->join_tbase,
                       e->join_pre, ntiles, ooff, e->seg_status, kStatusCallJoin);
    // 2. the rows
    if (nout) {
        const uint32_t sgrid = static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(nout) + rsx::kExpandSmallThreads) / rsx::kExpandSmallThreads, cus * 4));
        hipLaunchKernelGGL(rsx::join_split_kernel, dim3(sgrid), dim3(rsx::kExpandSmallThreads), 0, e->stream, e->join_tbase, e->join_pre, ntiles, bad, nout,
                           e->join_split);
        const TileChunks c = tile_chunks(nout, cus);
        hipLaunchKernelGGL((rsx::join_write_kernel<Key>), dim3(c.grid), dim3(rsx::kJoinThreads), 0, e->stream, ka, bad, e->join_tbase, e->join_pre,
                           want_first ? e->join_first : static_cast<const uint32_t*>(nullptr), want_arel ? e->join_arel : static_cast<const uint32_t*>(nullptr),
                           ntiles, e->join_split, nout, c.chunk, rows, kout, aout, bout);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_join(rsx_engine* e, const void* d_a, uint64_t na, const uint64_t* d_a_offsets, const void* d_b, uint64_t nb, const uint64_t* d_b_offsets,
                       uint64_t num_segments, uint32_t op, uint32_t flags, uint64_t out_capacity, void* d_keys_out, uint32_t* d_a_index_out,
                       uint32_t* d_b_index_out, uint64_t* d_out_offsets)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_join: null engine");
    if (op > RSX_JOIN_ANTI) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_join: unknown op (RSX_JOIN_INNER, _LEFT, _SEMI or _ANTI)");
    if (flags != 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_join: unknown flag bits (no flag is defined: flags must be 0)");
    if ((d_a_offsets != nullptr) != (d_b_offsets != nullptr))
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_join: one offsets array without the other (both NULL is the one segment [0, na) and [0, nb))");
    if (na > (1ull << 31) || nb > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_join: at most 2^31 keys in A and in B");
    if (d_a_offsets && num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_join: at most 2^32 - 2 segments");
    const bool write = d_keys_out || d_a_index_out || d_b_index_out;
    if (write && out_capacity > (1ull << 34))
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_join: out_capacity above 2^34 (the output tile grid is 32-bit; join in pieces)");
    if (d_b_index_out && op == RSX_JOIN_ANTI)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_join: d_b_index_out does not go with RSX_JOIN_ANTI (its rows have no partner in B)");
    if (!d_out_offsets) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_join: d_out_offsets is required (it alone says how many rows there are)");
    if (!d_a_offsets) num_segments = 1;
    const uint64_t kb = static_cast<uint64_t>(e->key_bytes);
    if ((na > 0 && !d_a) || (nb > 0 && !d_b) || !aligned16(d_a) || !aligned16(d_b))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_join: d_a and d_b must be 16-byte aligned device pointers");
    if (!aligned(d_a_index_out, 4) || !aligned(d_b_index_out, 4) || !aligned(d_keys_out, kb))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_join: the outputs must be aligned to their element size");
    if (!aligned(d_a_offsets, 8) || !aligned(d_b_offsets, 8) || !aligned(d_out_offsets, 8))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_join: offsets must be 8-byte aligned device pointers");
    const uint64_t cap = write ? out_capacity : 0;
    const uint64_t obytes = (num_segments + 1) * 8;
    if (check_buffers(e, "rsx_segmented_join", {{d_keys_out, cap * kb}, {d_a_index_out, cap * 4}, {d_b_index_out, cap * 4}, {d_out_offsets, obytes}},
                      {{d_a, na * kb}, {d_b, nb * kb}, {d_a_offsets, obytes}, {d_b_offsets, obytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (num_segments == 0) return RSX_OK;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    return by_key(e, [&](auto key) {
        using Key = decltype(key);
        return join_enqueue<Key>(e, static_cast<const Key*>(d_a), na, d_a_offsets, static_cast<const Key*>(d_b), nb, d_b_offsets, num_segments, op, cap,
                                 static_cast<Key*>(d_keys_out), d_a_index_out, d_b_index_out, d_out_offsets);
    });
}
