// capi_scan.inc — C ABI of the scan by key (rsx_segmented_scan, include/radixsort_hip.h): validate the offsets -> tails per tile -> the
// carries of all tiles (one workgroup) -> the tiles scanned and stored.  Kernels: rsx_scan_by_key.hpp.  Nothing of the engine's sort state
// is read or written: the call needs the first-bad-segment word, the status word and 3 * tiles + 2 slots of per-tile scratch.
// Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc.

extern "C++" {
namespace {

template <typename Key, typename Val, bool KEYS>
void scan_launch(rsx_engine* e, const Key* keys, const void* values, uint64_t n, const uint64_t* off, uint64_t nseg, uint32_t flags, uint32_t op,
                 void* vout, uint32_t* bad, uint32_t ntiles, uint32_t chunk, uint32_t tgrid)
{
    // the per-tile partials: tail, carry (one 8-byte slot each, whatever the value's width; the carry has one entry more) and the flags
    Val* tail = reinterpret_cast<Val*>(e->red_part);
    Val* carry = reinterpret_cast<Val*>(e->red_part + ntiles);
    uint32_t* tflags = reinterpret_cast<uint32_t*>(e->red_part + 2 * static_cast<uint64_t>(ntiles) + 1);
    const Val* vin = static_cast<const Val*>(values);
    hipLaunchKernelGGL((rsx::scan_tile_reduce_kernel<Key, Val, KEYS>), dim3(tgrid), dim3(rsx::kUniqThreads), 0, e->stream, keys, vin, n, off, nseg, bad, ntiles,
                       chunk, op, tail, tflags);
    hipLaunchKernelGGL((rsx::scan_carry_kernel<Val>), dim3(1), dim3(rsx::kScanCarryThreads), 0, e->stream, n, off, nseg, bad, ntiles, op, tail, tflags, carry,
                       e->seg_status);
    hipLaunchKernelGGL((rsx::scan_tile_kernel<Key, Val, KEYS>), dim3(tgrid), dim3(rsx::kUniqThreads), 0, e->stream, keys, vin, n, off, nseg, bad, ntiles, chunk,
                       op, flags, carry, static_cast<Val*>(vout));
}

template <typename Key, bool KEYS>
int scan_enqueue(rsx_engine* e, const Key* keys, const void* values, uint64_t n, const uint64_t* off, uint64_t nseg, uint32_t flags, uint32_t op,
                 uint32_t kind, void* vout)
{
    if (!off) nseg = 1;
    const uint64_t cus = cus_of(e);
    const uint32_t ntiles = static_cast<uint32_t>((n + rsx::kUniqTileKeys - 1) >> rsx::kUniqTileShift);
    const TileChunks c = tile_chunks(ntiles, cus);
    int rc = ensure_status_words(e);
    if (rc == RSX_OK) rc = seg_grow(e, &e->red_part, &e->red_part_cap, 3 * static_cast<uint64_t>(ntiles) + 2, "the per-tile partials of the scan");
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, off, n);
    switch (kind) {
    case RSX_VALUE_INT32: scan_launch<Key, int32_t, KEYS>(e, keys, values, n, off, nseg, flags, op, vout, bad, ntiles, c.chunk, c.grid); break;
    case RSX_VALUE_INT64: scan_launch<Key, int64_t, KEYS>(e, keys, values, n, off, nseg, flags, op, vout, bad, ntiles, c.chunk, c.grid); break;
    case RSX_VALUE_FLOAT32: scan_launch<Key, float, KEYS>(e, keys, values, n, off, nseg, flags, op, vout, bad, ntiles, c.chunk, c.grid); break;
    default: scan_launch<Key, double, KEYS>(e, keys, values, n, off, nseg, flags, op, vout, bad, ntiles, c.chunk, c.grid); break;
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_scan(rsx_engine* e, const void* d_keys, const void* d_values, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, uint32_t flags,
                       uint32_t op, uint32_t value_kind, void* d_values_out)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_scan: null engine");
    if ((flags & ~static_cast<uint32_t>(RSX_SCAN_EXCLUSIVE)) != 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_scan: unknown flag bits (RSX_SCAN_EXCLUSIVE or none)");
    if (op > RSX_REDUCE_MAX) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_scan: unknown op (RSX_REDUCE_SUM, _MIN or _MAX)");
    if (value_kind > RSX_VALUE_FLOAT64) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_scan: unknown value kind (RSX_VALUE_INT32, _INT64, _FLOAT32 or _FLOAT64)");
    if (n == 0 || (d_offsets && num_segments == 0)) return RSX_OK;
    if (!d_offsets) num_segments = 1;
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_scan: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_scan: at most 2^31 elements");
    const uint64_t vb = (value_kind == RSX_VALUE_INT32 || value_kind == RSX_VALUE_FLOAT32) ? 4 : 8;
    if (d_keys && !aligned16(d_keys)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_scan: keys must be a 16-byte aligned device pointer (or NULL)");
    if (!d_values || !aligned(d_values, vb))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_scan: values must be a device pointer aligned to the value size");
    if (!d_values_out || !aligned(d_values_out, vb))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_scan: the output must be a device pointer aligned to the value size");
    if (!aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_scan: offsets must be an 8-byte aligned device pointer");
    const uint64_t kbytes = n * static_cast<uint64_t>(e->key_bytes), obytes = (num_segments + 1) * 8, vbytes = n * vb;
    // in place (d_values_out == d_values exactly) is the one overlap that is served: a tile is read whole before it is written
    const bool in_place = d_values_out == d_values;
    if (!in_place && overlaps(d_values_out, vbytes, d_values, vbytes))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_scan: the output overlaps the values without being the same pointer (in place means d_values_out == d_values)");
    if (check_buffers(e, "rsx_segmented_scan", {{d_values_out, vbytes}}, {{in_place ? nullptr : d_values, vbytes}, {d_keys, kbytes}, {d_offsets, obytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    if (!d_keys) return scan_enqueue<uint32_t, false>(e, nullptr, d_values, n, d_offsets, num_segments, flags, op, value_kind, d_values_out);
    return by_key(e, [&](auto key) {
        using Key = decltype(key);
        return scan_enqueue<Key, true>(e, static_cast<const Key*>(d_keys), d_values, n, d_offsets, num_segments, flags, op, value_kind, d_values_out);
    });
}
