// capi_compact.inc — C ABI of the stream compaction (rsx_segmented_compact, include/radixsort_hip.h): validate the offsets -> kept elements
// per tile of the global grid -> the flat table scan -> kept offsets -> survivors staged in LDS and stored.  Kernels: rsx_compact.hpp.
// Nothing of the engine's sort state is read or written: the call needs the first-bad-segment word, the status word and one table entry
// per tile (the segmented table and its group sums, grown on demand).
// Included by rsx_capi.hip inside its extern "C" block, after capi_search.inc.

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
    const uint64_t cus = e->num_cus > 0 ? static_cast<uint64_t>(e->num_cus) : 256u;
    // launch bounds from n and the segment count alone: the table has one entry per tile of the global grid and one more (rsx_unique.hpp);
    // a workgroup walks `chunk` consecutive tiles (more than one above cus * 16 tiles)
    const uint32_t ntiles = static_cast<uint32_t>((n + rsx::kUniqTileKeys - 1) >> rsx::kUniqTileShift);
    const uint32_t ntab = ntiles + 1;
    const uint32_t npad = (ntab + rsx::kRadix - 1) / rsx::kRadix * rsx::kRadix;
    const uint32_t nrow = npad / rsx::kRadix;                        // the scan kernels' "tiles": 16 rows of nrow entries = the flat table
    const uint32_t ngroups = (nrow + rsx::kScanTiles - 1) / rsx::kScanTiles;
    const uint32_t chunk = static_cast<uint32_t>((npad + cus * 16 - 1) / (cus * 16));
    const uint32_t tgrid = (npad + chunk - 1) / chunk;
    const uint32_t wgrid = (ntiles + chunk - 1) / chunk;
    const uint32_t sgrid = static_cast<uint32_t>(std::min<uint64_t>((nseg + 1 + rsx::kUniqSmallThreads - 1) / rsx::kUniqSmallThreads, cus * 4));
    int rc = ensure_segmented(e, SegShape{1, 0, 0}, 1);           // the status words; none of the sort's scratch
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_table, &e->seg_table_cap, npad, "the per-tile table of the compaction");
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_gsum, &e->seg_gsum_cap, static_cast<uint64_t>(rsx::kRadix) * ngroups, "the group sums");
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_gsum2, &e->seg_gsum2_cap, static_cast<uint64_t>(rsx::kRadix) * ngroups, "the scanned group sums");
    if (rc != RSX_OK) return rc;
    // (a launch, not a non-zero hipMemsetAsync: capi_unique.inc)
    uint32_t* bad = e->seg_temp + 1;
    hipLaunchKernelGGL(rsx::unique_reset_kernel, dim3(1), dim3(rsx::kWave), 0, e->stream, bad);
    if (off) {
        hipLaunchKernelGGL(rsx::unique_validate_kernel, dim3(sgrid), dim3(rsx::kUniqSmallThreads), 0, e->stream, off, nseg, n, bad);
    }
    Key a = 0, m = 0;
    order_consts<Key>(e, &a, &m);
    // 1. kept elements per tile, their flat exclusive scan, the kept offsets (which also report a bad segment)
    if (bounds) {
        hipLaunchKernelGGL((rsx::compact_count_kernel<Key, true>), dim3(tgrid), dim3(rsx::kUniqThreads), 0, e->stream, keys, n, off, nseg, mask, bounds, flags, a,
                           m, bad, e->seg_table, ntab, npad, chunk, koff);
    } else {
        hipLaunchKernelGGL((rsx::compact_count_kernel<Key, false>), dim3(tgrid), dim3(rsx::kUniqThreads), 0, e->stream, keys, n, off, nseg, mask, bounds, flags, a,
                           m, bad, e->seg_table, ntab, npad, chunk, koff);
    }
    hipLaunchKernelGGL((rsx::scan_blocks_kernel<false, false>), dim3(ngroups), dim3(rsx::kScanTiles), 0, e->stream, e->seg_table, e->seg_gsum, nrow, ngroups,
                       static_cast<uint32_t*>(nullptr));
    hipLaunchKernelGGL(rsx::paste_scan_kernel, dim3(ngroups), dim3(rsx::kScanTiles), 0, e->stream, e->seg_table, e->seg_gsum, e->seg_gsum2, e->seg_temp, nrow,
                       ngroups);
    hipLaunchKernelGGL(rsx::unique_offsets_kernel, dim3(sgrid), dim3(rsx::kUniqSmallThreads), 0, e->stream, off, nseg, n, bad, e->seg_table, koff, e->seg_status, 1);
    // 2. the survivors, staged and stored
    if (kout || iout) {
        if (bounds) compact_write_launch<Key, true>(e, wgrid, keys, n, off, nseg, mask, bounds, flags, a, m, bad, ntiles, chunk, koff, kout, iout);
        else compact_write_launch<Key, false>(e, wgrid, keys, n, off, nseg, mask, bounds, flags, a, m, bad, ntiles, chunk, koff, kout, iout);
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
    if ((reinterpret_cast<uintptr_t>(d_keys_out) % kb) != 0 || (reinterpret_cast<uintptr_t>(d_index_out) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(d_kept_offsets_out) & 7u) != 0)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_compact: the outputs must be aligned to their element size");
    if ((reinterpret_cast<uintptr_t>(d_offsets) & 7u) != 0) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_compact: offsets must be an 8-byte aligned device pointer");
    if ((reinterpret_cast<uintptr_t>(d_bounds) % kb) != 0) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_compact: bounds must be aligned to the key size");
    const uint64_t kbytes = n * kb, obytes = (num_segments + 1) * 8, ibytes = n * 4, bbytes = num_segments * kb;
    const uint64_t ebytes = e->capacity * kb, epbytes = e->capacity * 4;
    const uint64_t kin_bytes = d_mask && !d_keys_out ? 0 : kbytes;       // a mask's keys are read for the key output only
    const void* bufs[7] = {d_keys_out, d_index_out, d_kept_offsets_out, d_keys, d_offsets, d_mask, d_bounds};       // outputs first
    const uint64_t bytes[7] = {kbytes, ibytes, obytes, kin_bytes, obytes, n, bbytes};
    for (int b = 0; b < 7; ++b) {
        for (int i = 0; i < 2; ++i) {
            if (overlaps(bufs[b], bytes[b], e->keys[i], ebytes) || overlaps(bufs[b], bytes[b], e->perm[i], epbytes))
                return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_compact: an input or output overlaps the engine's own buffers");
        }
    }
    for (int a = 0; a < 3; ++a) {
        for (int b = a + 1; b < 7; ++b) {
            if (overlaps(bufs[a], bytes[a], bufs[b], bytes[b]))
                return fail(RSX_HOST_BUFFERS_FAILED, b < 3 ? "rsx_segmented_compact: two outputs overlap"
                                                           : "rsx_segmented_compact: an output overlaps an input (no operation is in place)");
        }
    }
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    return RSX_BY_KEY(e, (compact_enqueue<uint32_t>(e, static_cast<const uint32_t*>(d_keys), n, d_offsets, num_segments, d_mask, static_cast<const uint32_t*>(d_bounds),
                                                    flags, static_cast<uint32_t*>(d_keys_out), d_index_out, d_kept_offsets_out)),
                      (compact_enqueue<uint64_t>(e, static_cast<const uint64_t*>(d_keys), n, d_offsets, num_segments, d_mask, static_cast<const uint64_t*>(d_bounds),
                                                 flags, static_cast<uint64_t*>(d_keys_out), d_index_out, d_kept_offsets_out)));
}
