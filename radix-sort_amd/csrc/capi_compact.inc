// capi_compact.inc — C ABI of the stream compaction (rsx_segmented_compact, include/radixsort_hip.h): validate the offsets -> kept elements
// per tile of the global grid -> the flat table scan -> kept offsets -> survivors staged in LDS and stored.  Kernels: rsx_compact.hpp.
// Nothing of the engine's sort state is read or written: the call needs the first-bad-segment word, the status word and one table entry
// per tile (the segmented table and its group sums, grown on demand).
// Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc.

extern "C++" {
namespace {

template <typename Key, bool BOUND>
void compact_write_launch(rsx_engine* e, uint32_t grid, const Key* keys, uint64_t n, const uint64_t* off, uint64_t nseg, const uint8_t* mask, const Key* bounds,
                          uint32_t flags, Key a, Key m, const uint32_t* bad, uint32_t ntiles, uint32_t chunk, const uint64_t* koff, Key* kout, uint32_t* iout)
{
    if (flags & RSX_COMPACT_PARTITION) {
        hipLaunchKernelGGL((rsx::compact_write_kernel<Key, BOUND, true>), dim3(grid), dim3(rsx::kUniqThreads), 0, e->stream, keys, n, off, nseg, mask, bounds,
                           flags, a, m, bad, e->seg_table, ntiles, chunk, koff, kout, iout);
    } else {
        hipLaunchKernelGGL((rsx::compact_write_kernel<Key, BOUND, false>), dim3(grid), dim3(rsx::kUniqThreads), 0, e->stream, keys, n, off, nseg, mask, bounds,
                           flags, a, m, bad, e->seg_table, ntiles, chunk, koff, kout, iout);
    }
}

template <typename Key>
int compact_enqueue(rsx_engine* e, const Key* keys, uint64_t n, const uint64_t* off, uint64_t nseg, const uint8_t* mask, const Key* bounds, uint32_t flags,
                    Key* kout, uint32_t* iout, uint64_t* koff)
{
    if (!off) nseg = 1;
    const uint64_t cus = cus_of(e);
    const TileTable t = tile_table(n, rsx::kUniqTileShift, cus);
    int rc = ensure_status_words(e);
    if (rc == RSX_OK) rc = grow_tile_table(e, t, "the per-tile table of the compaction");
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, off, n);
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    // 1. kept elements per tile, their flat exclusive scan, the kept offsets (which also report a bad segment)
    if (bounds) {
        hipLaunchKernelGGL((rsx::compact_count_kernel<Key, true>), dim3(t.tgrid), dim3(rsx::kUniqThreads), 0, e->stream, keys, n, off, nseg, mask, bounds, flags, a,
                           m, bad, e->seg_table, t.ntab, t.npad, t.chunk, koff);
    } else {
        hipLaunchKernelGGL((rsx::compact_count_kernel<Key, false>), dim3(t.tgrid), dim3(rsx::kUniqThreads), 0, e->stream, keys, n, off, nseg, mask, bounds, flags, a,
                           m, bad, e->seg_table, t.ntab, t.npad, t.chunk, koff);
    }
    launch_table_scan(e, t.nrow, t.ngroups);
    hipLaunchKernelGGL(rsx::unique_offsets_kernel, dim3(offsets_grid(nseg, cus)), dim3(rsx::kUniqSmallThreads), 0, e->stream, off, nseg, n, bad, e->seg_table, koff,
                       e->seg_status, 1);
    // 2. the survivors, staged and stored
    if (kout || iout) {
        if (bounds) compact_write_launch<Key, true>(e, t.wgrid, keys, n, off, nseg, mask, bounds, flags, a, m, bad, t.ntiles, t.chunk, koff, kout, iout);
        else compact_write_launch<Key, false>(e, t.wgrid, keys, n, off, nseg, mask, bounds, flags, a, m, bad, t.ntiles, t.chunk, koff, kout, iout);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_compact(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, const uint8_t* d_mask,
                          const void* d_bounds, uint32_t flags, void* d_keys_out, uint32_t* d_index_out, uint64_t* d_kept_offsets_out)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_compact: null engine");
    if ((flags & ~static_cast<uint32_t>(RSX_COMPACT_PARTITION | RSX_COMPACT_INVERT | RSX_COMPACT_STRICT)) != 0)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_compact: unknown flag bits (RSX_COMPACT_PARTITION, _INVERT, _STRICT or none)");
    if ((d_mask != nullptr) == (d_bounds != nullptr))
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_compact: exactly one of d_mask and d_bounds must be given");
    if (d_mask && (flags & RSX_COMPACT_STRICT) != 0)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_compact: RSX_COMPACT_STRICT belongs to the bound form (a mask has no ties)");
    if (n == 0 || (d_offsets && num_segments == 0)) return RSX_OK;
    if (!d_offsets) num_segments = 1;
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_compact: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_compact: at most 2^31 elements");
    const uint64_t kb = static_cast<uint64_t>(e->key_bytes);
    if (!d_keys || !aligned16(d_keys)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_compact: keys must be a 16-byte aligned device pointer");
    if (!d_kept_offsets_out) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_compact: the kept-offsets output is required");
    if (!aligned(d_keys_out, kb) || !aligned(d_index_out, 4) || !aligned(d_kept_offsets_out, 8))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_compact: the outputs must be aligned to their element size");
    if (!aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_compact: offsets must be an 8-byte aligned device pointer");
    if (!aligned(d_bounds, kb)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_compact: bounds must be aligned to the key size");
    const uint64_t kbytes = n * kb, obytes = (num_segments + 1) * 8, ibytes = n * 4, bbytes = num_segments * kb;
    const uint64_t kin_bytes = d_mask && !d_keys_out ? 0 : kbytes;       // a mask's keys are read for the key output only
    if (check_buffers(e, "rsx_segmented_compact", {{d_keys_out, kbytes}, {d_index_out, ibytes}, {d_kept_offsets_out, obytes}},
                      {{d_keys, kin_bytes}, {d_offsets, obytes}, {d_mask, n}, {d_bounds, bbytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    return by_key(e, [&](auto key) {
        using Key = decltype(key);
        return compact_enqueue<Key>(e, static_cast<const Key*>(d_keys), n, d_offsets, num_segments, d_mask, static_cast<const Key*>(d_bounds), flags,
                                    static_cast<Key*>(d_keys_out), d_index_out, d_kept_offsets_out);
    });
}
