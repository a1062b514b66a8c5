// capi_unique.inc — C ABI of the segmented unique (rsx_segmented_unique, include/radixsort_hip.h): sort (the segmented chain, or the flat
// product chain when d_offsets is NULL; nothing in consecutive mode) into the engine's own buffers -> heads per tile of the global grid ->
// the flat table scan -> run offsets -> keys / first positions / inverse map -> counts.  Kernels: rsx_unique.hpp.
// Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc and capi_segmented.inc (whose segmented_enqueue it calls).

extern "C++" {
namespace {

template <typename Key, bool POS, bool PERM>
void unique_write_launch(rsx_engine* e, uint32_t grid, const Key* keys, const uint32_t* perm, uint64_t n, const uint64_t* off, uint64_t nseg,
                         const uint32_t* bad, uint32_t ntiles, uint32_t chunk, const uint64_t* uoff, Key* kout, uint32_t* first, uint32_t* inverse,
                         uint32_t* hp)
{
    hipLaunchKernelGGL((rsx::unique_write_kernel<Key, POS, PERM>), dim3(grid), dim3(rsx::kUniqThreads), 0, e->stream, keys, perm, n, off, nseg, bad,
                       e->seg_table, ntiles, chunk, uoff, kout, first, inverse, hp);
}

// What the grouping steps leave for the steps that write the runs: where the grouped keys (and the positions they came from) are, a buffer
// of n words for the heads' positions, the first-bad-segment word, and the tile grid.
template <typename Key>
struct UniqGroups {
    const Key* skeys;
    const uint32_t* sperm;
    uint32_t* hp;
    uint32_t* bad;
    uint32_t ntiles, chunk, tgrid;
    uint64_t cus;
};

// Steps 1 and 2 of rsx_segmented_unique, shared with rsx_segmented_reduce_by_key (capi_reduce.inc): validate the offsets, group equal keys
// (carry: with the positions as the sort's payload), count the heads per tile, scan, write the run offsets.
template <typename Key>
int unique_groups_enqueue(rsx_engine* e, const Key* kin, uint64_t n, const uint64_t* off, uint64_t nseg, bool consecutive, bool carry, uint64_t* uoff,
                          UniqGroups<Key>* out)
{
    const bool seg_sort = off && !consecutive;
    const uint64_t cus = cus_of(e);
    const TileTable t = tile_table(n, rsx::kUniqTileShift, cus);
    const uint32_t sgrid = offsets_grid(nseg, cus);

    // scratch: the segmented sort's (all of it only when that sort runs), with the table and group sums large enough for both uses
    SegShape shape{1, 0, 0};
    if (seg_sort) shape = seg_shape(n, nseg);
    int rc = ensure_segmented(e, shape, seg_sort ? nseg : 1);
    if (rc == RSX_OK) rc = grow_tile_table(e, t, "the segmented table", shape.max_tiles);
    if (rc == RSX_OK && carry && (e->uniq_iota_cap < n || !e->uniq_iota)) {
        rc = seg_grow(e, &e->uniq_iota, &e->uniq_iota_cap, e->capacity, "the positions");
        if (rc == RSX_OK) {
            const uint64_t grid = std::min<uint64_t>((e->uniq_iota_cap + rsx::kUniqSmallThreads - 1) / rsx::kUniqSmallThreads, cus * 8);
            hipLaunchKernelGGL(rsx::unique_iota_kernel, dim3(static_cast<uint32_t>(grid)), dim3(rsx::kUniqSmallThreads), 0, e->stream, e->uniq_iota,
                               e->uniq_iota_cap);
        }
    }
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, off, n);

    // 1. group equal keys: sorted keys (and the positions they came from) end up in the engine's own buffers
    const Key* skeys = kin;
    const uint32_t* sperm = nullptr;
    uint32_t* hp = static_cast<uint32_t*>(e->keys[0]);              // head positions: a key buffer the sort has finished with
    if (seg_sort) {
        // (an even number of passes: the chain's last pass reads keys[0] and writes keys[1]; the small segments go straight to keys[1])
        rc = segmented_enqueue<Key>(e, kin, carry ? e->uniq_iota : nullptr, n, off, nseg, static_cast<Key*>(e->keys[1]), carry ? e->perm[1] : nullptr, carry);
        if (rc != RSX_OK) return rc;
        skeys = static_cast<const Key*>(e->keys[1]);
        sperm = carry ? e->perm[1] : nullptr;
    } else if (!consecutive) {
        // every pass, whatever the options say; without positions the sort carries no payload, on a payload engine too
        const int passes = static_cast<int>(e->passes());
        const SortJob job{kin, carry ? e->uniq_iota : nullptr, n, 0, passes, 0, passes, nullptr, nullptr, carry};
        rc = sort_chain<Key>(e, job);
        if (rc != RSX_OK) return rc;
        skeys = static_cast<const Key*>(e->result_keys);
        sperm = carry ? e->result_perm : nullptr;
        hp = static_cast<uint32_t*>(e->keys[e->cur ^ 1]);
    }

    // 2. heads per tile, their flat exclusive scan, the run offsets
    hipLaunchKernelGGL((rsx::unique_count_kernel<Key>), dim3(t.tgrid), dim3(rsx::kUniqThreads), 0, e->stream, skeys, n, off, nseg, bad, e->seg_table, t.ntab,
                       t.npad, t.chunk, uoff);
    launch_table_scan(e, t.nrow, t.ngroups);
    hipLaunchKernelGGL(rsx::unique_offsets_kernel, dim3(sgrid), dim3(rsx::kUniqSmallThreads), 0, e->stream, off, nseg, n, bad, e->seg_table, uoff,
                       e->seg_status, consecutive ? 1 : 0);

    out->skeys = skeys;
    out->sperm = sperm;
    out->hp = hp;
    out->bad = bad;
    out->ntiles = t.ntiles;
    out->chunk = t.chunk;
    out->tgrid = t.tgrid;
    out->cus = cus;
    return RSX_OK;
}

template <typename Key>
int unique_enqueue(rsx_engine* e, const Key* kin, uint64_t n, const uint64_t* off, uint64_t nseg, uint32_t flags, Key* kout, uint64_t* uoff,
                   uint32_t* counts, uint32_t* first, uint32_t* inverse)
{
    const bool consecutive = (flags & RSX_UNIQUE_CONSECUTIVE) != 0;
    const bool positions = first || inverse;
    if (!off) nseg = 1;
    UniqGroups<Key> g;
    const int rc = unique_groups_enqueue<Key>(e, kin, n, off, nseg, consecutive, positions && !consecutive, uoff, &g);
    if (rc != RSX_OK) return rc;
    const Key* skeys = g.skeys;
    const uint32_t* sperm = g.sperm;
    uint32_t* bad = g.bad;
    uint32_t* hp = counts ? g.hp : nullptr;
    const uint32_t ntiles = g.ntiles, chunk = g.chunk, tgrid = g.tgrid;
    const uint64_t cus = g.cus;

    // 3. the runs: keys, first positions, inverse map; then the counts from the heads' positions
    if (positions && sperm) unique_write_launch<Key, true, true>(e, tgrid, skeys, sperm, n, off, nseg, bad, ntiles, chunk, uoff, kout, first, inverse, hp);
    else if (positions) unique_write_launch<Key, true, false>(e, tgrid, skeys, sperm, n, off, nseg, bad, ntiles, chunk, uoff, kout, first, inverse, hp);
    else unique_write_launch<Key, false, false>(e, tgrid, skeys, sperm, n, off, nseg, bad, ntiles, chunk, uoff, kout, first, inverse, hp);
    if (counts) {
        const uint64_t grid = std::min<uint64_t>((n + rsx::kUniqSmallThreads - 1) / rsx::kUniqSmallThreads, cus * 8);
        hipLaunchKernelGGL(rsx::unique_counts_kernel, dim3(static_cast<uint32_t>(grid)), dim3(rsx::kUniqSmallThreads), 0, e->stream, hp, e->seg_table, ntiles,
                           off, nseg, n, counts);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_unique(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, uint32_t flags,
                         void* d_keys_out, uint64_t* d_run_offsets_out, uint32_t* d_counts_out, uint32_t* d_first_out, uint32_t* d_inverse_out)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_unique: null engine");
    if ((flags & ~static_cast<uint32_t>(RSX_UNIQUE_CONSECUTIVE)) != 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_unique: unknown flag bits");
    if (n > e->capacity) return fail(RSX_RESIZE_FAILED, "rsx_segmented_unique: beyond capacity");
    if (n == 0 || (d_offsets && num_segments == 0)) return RSX_OK;
    if (!d_offsets) num_segments = 1;
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_unique: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_unique: at most 2^31 keys");
    const bool consecutive = (flags & RSX_UNIQUE_CONSECUTIVE) != 0;
    if (!d_keys || !aligned16(d_keys)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_unique: keys must be a 16-byte aligned device pointer");
    if (!d_keys_out || !d_run_offsets_out) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_unique: the key and run-offset outputs are required");
    if (!aligned(d_keys_out, e->key_bytes) || !aligned(d_run_offsets_out, 8) || !aligned(d_counts_out, 4) || !aligned(d_first_out, 4) || !aligned(d_inverse_out, 4))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_unique: the outputs must be aligned to their element size");
    if (!aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_unique: offsets must be an 8-byte aligned device pointer");
    if (!consecutive && (d_first_out || d_inverse_out) && !e->has_payload)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_unique: first positions and the inverse map of a sorted call travel through the sort as its payload: "
                                             "they need an engine created with has_payload = 1");
    const uint64_t kbytes = n * static_cast<uint64_t>(e->key_bytes), obytes = (num_segments + 1) * 8, ibytes = n * 4;
    if (check_buffers(e, "rsx_segmented_unique",
                      {{d_keys_out, kbytes}, {d_run_offsets_out, obytes}, {d_counts_out, ibytes}, {d_first_out, ibytes}, {d_inverse_out, ibytes}},
                      {{d_keys, kbytes}, {d_offsets, obytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (overlaps(d_keys, kbytes, d_offsets, obytes)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_unique: keys and offsets overlap");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    const int rc = by_key(e, [&](auto key) {
        using Key = decltype(key);
        return unique_enqueue<Key>(e, static_cast<const Key*>(d_keys), n, d_offsets, num_segments, flags, static_cast<Key*>(d_keys_out), d_run_offsets_out, d_counts_out,
                                   d_first_out, d_inverse_out);
    });
    result_is_external(e, n);       // (whatever rc says: a chain that failed half way has still used the engine's buffers)
    return rc;
}
