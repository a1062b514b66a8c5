// capi_unique.inc — C ABI of the segmented unique (rsx_segmented_unique, include/radixsort_hip.h): sort (the segmented chain, or the flat
// product chain when d_offsets is NULL; nothing in consecutive mode) into the engine's own buffers -> heads per tile of the global grid ->
// the flat table scan -> run offsets -> keys / first positions / inverse map -> counts.  Kernels: rsx_unique.hpp.
// Included by rsx_capi.hip inside its extern "C" block, after capi_select.inc.

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
    const uint64_t cus = e->num_cus > 0 ? static_cast<uint64_t>(e->num_cus) : 256u;

    // launch bounds from n and the segment count alone: the table has one entry per tile of the global grid and one more (rsx_unique.hpp)
    const uint32_t ntiles = static_cast<uint32_t>((n + rsx::kUniqTileKeys - 1) >> rsx::kUniqTileShift);
    const uint32_t ntab = ntiles + 1;
    const uint32_t npad = (ntab + rsx::kRadix - 1) / rsx::kRadix * rsx::kRadix;
    const uint32_t nrow = npad / rsx::kRadix;                        // the scan kernels' "tiles": 16 rows of nrow entries = the flat table
    const uint32_t ngroups = (nrow + rsx::kScanTiles - 1) / rsx::kScanTiles;
    const uint32_t chunk = static_cast<uint32_t>((npad + cus * 16 - 1) / (cus * 16));
    const uint32_t tgrid = (npad + chunk - 1) / chunk;
    const uint32_t sgrid = static_cast<uint32_t>(std::min<uint64_t>((nseg + 1 + rsx::kUniqSmallThreads - 1) / rsx::kUniqSmallThreads, cus * 4));

    // scratch: the segmented sort's (all of it only when that sort runs), with the table and group sums large enough for both uses
    SegShape shape{1, 0, 0};
    if (seg_sort) shape = seg_shape(n, nseg);
    int rc = ensure_segmented(e, shape, seg_sort ? nseg : 1);
    const uint64_t sort_groups = (shape.max_tiles + rsx::kScanTiles - 1) / rsx::kScanTiles;
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_table, &e->seg_table_cap, std::max<uint64_t>(rsx::kRadix * shape.max_tiles, npad), "the segmented table");
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_gsum, &e->seg_gsum_cap, rsx::kRadix * std::max<uint64_t>(sort_groups, ngroups), "the group sums");
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_gsum2, &e->seg_gsum2_cap, rsx::kRadix * std::max<uint64_t>(sort_groups, ngroups), "the scanned group sums");
    if (rc == RSX_OK && carry && (e->uniq_iota_cap < n || !e->uniq_iota)) {
        rc = seg_grow(e, &e->uniq_iota, &e->uniq_iota_cap, e->capacity, "the positions");
        if (rc == RSX_OK) {
            const uint64_t grid = std::min<uint64_t>((e->uniq_iota_cap + rsx::kUniqSmallThreads - 1) / rsx::kUniqSmallThreads, cus * 8);
            hipLaunchKernelGGL(rsx::unique_iota_kernel, dim3(static_cast<uint32_t>(grid)), dim3(rsx::kUniqSmallThreads), 0, e->stream, e->uniq_iota,
                               e->uniq_iota_cap);
        }
    }
    if (rc != RSX_OK) return rc;
    // (a launch, not hipMemsetAsync(bad, 0xFF, 4): with that memset a captured unique + reduce pair replayed as if its offsets were bad,
    // every run offset 0, though the same calls were right when run eagerly; DESIGN.md, the chain of the segmented unique)
    uint32_t* bad = e->seg_temp + 1;
    hipLaunchKernelGGL(rsx::unique_reset_kernel, dim3(1), dim3(rsx::kWave), 0, e->stream, bad);
    if (off) {
        hipLaunchKernelGGL(rsx::unique_validate_kernel, dim3(sgrid), dim3(rsx::kUniqSmallThreads), 0, e->stream, off, nseg, n, bad);
    }

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
    hipLaunchKernelGGL((rsx::unique_count_kernel<Key>), dim3(tgrid), dim3(rsx::kUniqThreads), 0, e->stream, skeys, n, off, nseg, bad, e->seg_table, ntab,
                       npad, chunk, uoff);
    hipLaunchKernelGGL((rsx::scan_blocks_kernel<false, false>), dim3(ngroups), dim3(rsx::kScanTiles), 0, e->stream, e->seg_table, e->seg_gsum, nrow,
                       ngroups, static_cast<uint32_t*>(nullptr));
    hipLaunchKernelGGL(rsx::paste_scan_kernel, dim3(ngroups), dim3(rsx::kScanTiles), 0, e->stream, e->seg_table, e->seg_gsum, e->seg_gsum2, e->seg_temp,
                       nrow, ngroups);
    hipLaunchKernelGGL(rsx::unique_offsets_kernel, dim3(sgrid), dim3(rsx::kUniqSmallThreads), 0, e->stream, off, nseg, n, bad, e->seg_table, uoff,
                       e->seg_status, consecutive ? 1 : 0);

    out->skeys = skeys;
    out->sperm = sperm;
    out->hp = hp;
    out->bad = bad;
    out->ntiles = ntiles;
    out->chunk = chunk;
    out->tgrid = tgrid;
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
    if ((reinterpret_cast<uintptr_t>(d_keys_out) % e->key_bytes) != 0 || (reinterpret_cast<uintptr_t>(d_run_offsets_out) & 7u) != 0 ||
        (reinterpret_cast<uintptr_t>(d_counts_out) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_first_out) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(d_inverse_out) & 3u) != 0)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_unique: the outputs must be aligned to their element size");
    if (d_offsets && (reinterpret_cast<uintptr_t>(d_offsets) & 7u) != 0) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_unique: offsets must be an 8-byte aligned device pointer");
    if (!consecutive && (d_first_out || d_inverse_out) && !e->has_payload)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_unique: first positions and the inverse map of a sorted call travel through the sort as its payload: "
                                             "they need an engine created with has_payload = 1");
    const uint64_t kbytes = n * static_cast<uint64_t>(e->key_bytes), obytes = (num_segments + 1) * 8, ibytes = n * 4;
    const uint64_t ebytes = e->capacity * static_cast<uint64_t>(e->key_bytes), epbytes = e->capacity * 4;
    const void* bufs[7] = {d_keys_out, d_run_offsets_out, d_counts_out, d_first_out, d_inverse_out, d_keys, d_offsets};       // outputs first
    const uint64_t bytes[7] = {kbytes, obytes, ibytes, ibytes, ibytes, kbytes, obytes};
    for (int b = 0; b < 7; ++b) {
        for (int i = 0; i < 2; ++i) {
            if (overlaps(bufs[b], bytes[b], e->keys[i], ebytes) || overlaps(bufs[b], bytes[b], e->perm[i], epbytes))
                return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_unique: an input or output overlaps the engine's own buffers");
        }
    }
    for (int a = 0; a < 5; ++a) {
        for (int b = a + 1; b < 7; ++b) {
            if (overlaps(bufs[a], bytes[a], bufs[b], bytes[b]))
                return fail(RSX_HOST_BUFFERS_FAILED, b < 5 ? "rsx_segmented_unique: two outputs overlap" : "rsx_segmented_unique: an output overlaps an input");
        }
    }
    if (overlaps(d_keys, kbytes, d_offsets, obytes)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_unique: keys and offsets overlap");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    const int rc = RSX_BY_KEY(e,
                              unique_enqueue<uint32_t>(e, static_cast<const uint32_t*>(d_keys), n, d_offsets, num_segments, flags,
                                                       static_cast<uint32_t*>(d_keys_out), d_run_offsets_out, d_counts_out, d_first_out, d_inverse_out),
                              unique_enqueue<uint64_t>(e, static_cast<const uint64_t*>(d_keys), n, d_offsets, num_segments, flags,
                                                       static_cast<uint64_t*>(d_keys_out), d_run_offsets_out, d_counts_out, d_first_out, d_inverse_out));
    // as after rsx_segmented_sort: the result lives in the caller's buffers only, and the engine's tables are not this call's
    e->n = n;
    e->result_external = true;
    e->counted_keys = nullptr;
    e->table_valid = false;
    e->globsum_valid = false;
    return rc;
}
