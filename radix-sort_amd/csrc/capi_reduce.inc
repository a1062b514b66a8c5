// capi_reduce.inc — C ABI of the reduce by key (rsx_segmented_reduce_by_key, include/radixsort_hip.h): the grouping steps of
// rsx_segmented_unique (capi_unique.inc: sort with the positions as payload, or nothing in consecutive mode -> heads per tile -> the flat
// table scan -> run offsets), then the values reduced per tile and carried across tiles -> counts.  Kernels: rsx_reduce.hpp.
// Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc and capi_unique.inc (whose grouping steps it calls).

extern "C++" {
namespace {

template <typename Key, typename Val>
int reduce_launch(rsx_engine* e, const UniqGroups<Key>& g, const void* values, uint64_t n, const uint64_t* off, uint64_t nseg, uint32_t op, Key* kout,
                  void* vout, uint32_t* hp)
{
    // the per-tile partials: lead, tail (one 8-byte slot each, whatever the value's width) and the flags
    Val* lead = reinterpret_cast<Val*>(e->red_part);
    Val* tail = reinterpret_cast<Val*>(e->red_part + g.ntiles);
    uint32_t* flags = reinterpret_cast<uint32_t*>(e->red_part + 2 * static_cast<uint64_t>(g.ntiles));
    const Val* vin = static_cast<const Val*>(values);
    Val* out = static_cast<Val*>(vout);
    if (g.sperm) {
        hipLaunchKernelGGL((rsx::reduce_tile_kernel<Key, Val, true>), dim3(g.tgrid), dim3(rsx::kUniqThreads), 0, e->stream, g.skeys, g.sperm, vin, n, off, nseg,
                           g.bad, e->seg_table, g.ntiles, g.chunk, op, kout, out, hp, lead, tail, flags);
    } else {
        hipLaunchKernelGGL((rsx::reduce_tile_kernel<Key, Val, false>), dim3(g.tgrid), dim3(rsx::kUniqThreads), 0, e->stream, g.skeys, g.sperm, vin, n, off, nseg,
                           g.bad, e->seg_table, g.ntiles, g.chunk, op, kout, out, hp, lead, tail, flags);
    }
    constexpr uint32_t waves = rsx::kRedCarryThreads / rsx::kWave;
    const uint32_t cgrid = static_cast<uint32_t>(std::min<uint64_t>((g.ntiles + waves - 1) / waves, g.cus * 8));
    hipLaunchKernelGGL((rsx::reduce_carry_kernel<Val>), dim3(cgrid), dim3(rsx::kRedCarryThreads), 0, e->stream, n, off, nseg, g.bad, e->seg_table, g.ntiles, op,
                       out, lead, tail, flags);
    return RSX_OK;
}

template <typename Key>
int reduce_enqueue(rsx_engine* e, const Key* kin, const void* values, uint64_t n, const uint64_t* off, uint64_t nseg, uint32_t flags, uint32_t op,
                   uint32_t kind, Key* kout, uint64_t* uoff, void* vout, uint32_t* counts)
{
    const bool consecutive = (flags & RSX_UNIQUE_CONSECUTIVE) != 0;
    if (!off) nseg = 1;
    const uint64_t ntiles = (n + rsx::kUniqTileKeys - 1) >> rsx::kUniqTileShift;
    int rc = seg_grow(e, &e->red_part, &e->red_part_cap, 3 * ntiles, "the per-tile partials of the reduction");
    if (rc != RSX_OK) return rc;
    UniqGroups<Key> g;
    rc = unique_groups_enqueue<Key>(e, kin, n, off, nseg, consecutive, !consecutive, uoff, &g);
    if (rc != RSX_OK) return rc;
    uint32_t* hp = counts ? g.hp : nullptr;
    switch (kind) {
    case RSX_VALUE_INT32: rc = reduce_launch<Key, int32_t>(e, g, values, n, off, nseg, op, kout, vout, hp); break;
    case RSX_VALUE_INT64: rc = reduce_launch<Key, int64_t>(e, g, values, n, off, nseg, op, kout, vout, hp); break;
    case RSX_VALUE_FLOAT32: rc = reduce_launch<Key, float>(e, g, values, n, off, nseg, op, kout, vout, hp); break;
    default: rc = reduce_launch<Key, double>(e, g, values, n, off, nseg, op, kout, vout, hp); break;
    }
    if (counts) {
        const uint64_t grid = std::min<uint64_t>((n + rsx::kUniqSmallThreads - 1) / rsx::kUniqSmallThreads, g.cus * 8);
        hipLaunchKernelGGL(rsx::unique_counts_kernel, dim3(static_cast<uint32_t>(grid)), dim3(rsx::kUniqSmallThreads), 0, e->stream, hp, e->seg_table,
                           g.ntiles, off, nseg, n, counts);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return rc;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_reduce_by_key(rsx_engine* e, const void* d_keys, const void* d_values, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments,
                                uint32_t flags, uint32_t op, uint32_t value_kind, void* d_keys_out, uint64_t* d_run_offsets_out, void* d_values_out,
                                uint32_t* d_counts_out)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce_by_key: null engine");
    if ((flags & ~static_cast<uint32_t>(RSX_UNIQUE_CONSECUTIVE)) != 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce_by_key: unknown flag bits");
    if (op > RSX_REDUCE_MAX) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce_by_key: unknown op (RSX_REDUCE_SUM, _MIN or _MAX)");
    if (value_kind > RSX_VALUE_FLOAT64) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce_by_key: unknown value kind (RSX_VALUE_INT32, _INT64, _FLOAT32 or _FLOAT64)");
    if (n > e->capacity) return fail(RSX_RESIZE_FAILED, "rsx_segmented_reduce_by_key: beyond capacity");
    if (n == 0 || (d_offsets && num_segments == 0)) return RSX_OK;
    if (!d_offsets) num_segments = 1;
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce_by_key: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce_by_key: at most 2^31 keys");
    const bool consecutive = (flags & RSX_UNIQUE_CONSECUTIVE) != 0;
    const uint64_t vb = (value_kind == RSX_VALUE_INT32 || value_kind == RSX_VALUE_FLOAT32) ? 4 : 8;
    if (!d_keys || !aligned16(d_keys)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce_by_key: keys must be a 16-byte aligned device pointer");
    if (!d_values || !aligned(d_values, vb))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce_by_key: values must be a device pointer aligned to the value size");
    if (!d_keys_out || !d_run_offsets_out || !d_values_out)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce_by_key: the key, run-offset and value outputs are required");
    if (!aligned(d_keys_out, e->key_bytes) || !aligned(d_run_offsets_out, 8) || !aligned(d_values_out, vb) || !aligned(d_counts_out, 4))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce_by_key: the outputs must be aligned to their element size");
    if (!aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce_by_key: offsets must be an 8-byte aligned device pointer");
    if (!consecutive && !e->has_payload)
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce_by_key: the positions of the values of a sorted call travel through the sort as its payload: "
                                             "they need an engine created with has_payload = 1");
    const uint64_t kbytes = n * static_cast<uint64_t>(e->key_bytes), obytes = (num_segments + 1) * 8, vbytes = n * vb, cbytes = n * 4;
    if (check_buffers(e, "rsx_segmented_reduce_by_key", {{d_keys_out, kbytes}, {d_run_offsets_out, obytes}, {d_values_out, vbytes}, {d_counts_out, cbytes}},
                      {{d_keys, kbytes}, {d_values, vbytes}, {d_offsets, obytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (overlaps(d_keys, kbytes, d_values, vbytes) || overlaps(d_keys, kbytes, d_offsets, obytes) || overlaps(d_values, vbytes, d_offsets, obytes))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce_by_key: two inputs overlap");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    const int rc = by_key(e, [&](auto key) {
        using Key = decltype(key);
        return reduce_enqueue<Key>(e, static_cast<const Key*>(d_keys), d_values, n, d_offsets, num_segments, flags, op, value_kind, static_cast<Key*>(d_keys_out),
                                   d_run_offsets_out, d_values_out, d_counts_out);
    });
    result_is_external(e, n);       // (whatever rc says: as rsx_segmented_unique)
    return rc;
}
