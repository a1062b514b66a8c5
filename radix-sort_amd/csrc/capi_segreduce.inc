// capi_segreduce.inc — C ABI of the segmented reduction (rsx_segmented_reduce, include/radixsort_hip.h): validate the offsets -> one fold per
// 4096-element tile, the segments inside a tile stored at once -> the empty segments and the segments that cross tile edges.  Kernels:
// rsx_segreduce.hpp.  Nothing of the engine's sort state is read or written: the call needs the first-bad-segment word, the status words
// and 4 * tiles slots of per-tile scratch.  Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc.

extern "C++" {
namespace {

template <typename Val, bool ARG>
void segreduce_launch(rsx_engine* e, const void* values, uint64_t n, const uint64_t* off, uint64_t nseg, uint32_t op, void* vout, uint32_t* iout,
                      uint32_t* bad, uint32_t ntiles, uint64_t cus)
{
    // the per-tile partials: lead and tail (one 8-byte slot each, whatever the value's width), then three words per tile: the positions
    // that go with them (arg ops) and the segment that the tail belongs to
    Val* lead = reinterpret_cast<Val*>(e->red_part);
    Val* tail = reinterpret_cast<Val*>(e->red_part + ntiles);
    uint32_t* lead_pos = reinterpret_cast<uint32_t*>(e->red_part + 2 * static_cast<uint64_t>(ntiles));
    uint32_t* tail_pos = lead_pos + ntiles;
    uint32_t* open_seg = tail_pos + ntiles;
    if (ntiles != 0) {
        const TileChunks c = tile_chunks(ntiles, cus);
        hipLaunchKernelGGL((rsx::segreduce_tile_kernel<Val, ARG>), dim3(c.grid), dim3(rsx::kUniqThreads), 0, e->stream, static_cast<const Val*>(values), n, off, nseg,
                           bad, ntiles, c.chunk, op, static_cast<Val*>(vout), iout, lead, tail, lead_pos, tail_pos, open_seg);
    }
    // one thread per segment and one workgroup per tile, bounded by residency
    const uint64_t want = std::max<uint64_t>((nseg + rsx::kSegRedJoinThreads - 1) / rsx::kSegRedJoinThreads, ntiles);
    const uint32_t jgrid = static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(want, 1), cus * 16));
    hipLaunchKernelGGL((rsx::segreduce_join_kernel<Val, ARG>), dim3(jgrid), dim3(rsx::kSegRedJoinThreads), 0, e->stream, n, off, nseg, bad, ntiles, op,
                       static_cast<Val*>(vout), iout, lead, tail, lead_pos, tail_pos, open_seg, e->seg_status, kStatusCallReduce);
}

int segreduce_enqueue(rsx_engine* e, const void* values, uint64_t n, const uint64_t* off, uint64_t nseg, uint32_t op, uint32_t kind, void* vout, uint32_t* iout)
{
    const uint64_t cus = cus_of(e);
    const uint32_t ntiles = static_cast<uint32_t>((n + rsx::kUniqTileKeys - 1) >> rsx::kUniqTileShift);
    int rc = ensure_status_words(e);
    if (rc == RSX_OK) rc = seg_grow(e, &e->red_part, &e->red_part_cap, 4 * static_cast<uint64_t>(ntiles) + 2, "the per-tile partials of the segmented reduction");
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, off, n);
    const bool arg = op >= RSX_REDUCE_ARGMIN;
    const uint32_t kop = op == RSX_REDUCE_ARGMIN ? rsx::kRedMin : op == RSX_REDUCE_ARGMAX ? rsx::kRedMax : op;
    switch (kind) {
    case RSX_VALUE_INT32:
        if (arg) segreduce_launch<int32_t, true>(e, values, n, off, nseg, kop, vout, iout, bad, ntiles, cus);
        else segreduce_launch<int32_t, false>(e, values, n, off, nseg, kop, vout, iout, bad, ntiles, cus);
        break;
    case RSX_VALUE_INT64:
        if (arg) segreduce_launch<int64_t, true>(e, values, n, off, nseg, kop, vout, iout, bad, ntiles, cus);
        else segreduce_launch<int64_t, false>(e, values, n, off, nseg, kop, vout, iout, bad, ntiles, cus);
        break;
    case RSX_VALUE_FLOAT32:
        if (arg) segreduce_launch<float, true>(e, values, n, off, nseg, kop, vout, iout, bad, ntiles, cus);
        else segreduce_launch<float, false>(e, values, n, off, nseg, kop, vout, iout, bad, ntiles, cus);
        break;
    default:
        if (arg) segreduce_launch<double, true>(e, values, n, off, nseg, kop, vout, iout, bad, ntiles, cus);
        else segreduce_launch<double, false>(e, values, n, off, nseg, kop, vout, iout, bad, ntiles, cus);
        break;
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_reduce(rsx_engine* e, const void* d_values, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, uint32_t flags, uint32_t op,
                         uint32_t value_kind, void* d_values_out, uint32_t* d_index_out)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce: null engine");
    if (flags != 0) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce: unknown flag bits (flags must be 0)");
    if (op > RSX_REDUCE_ARGMAX) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce: unknown op (RSX_REDUCE_SUM, _MIN, _MAX, _ARGMIN or _ARGMAX)");
    if (value_kind > RSX_VALUE_FLOAT64) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce: unknown value kind (RSX_VALUE_INT32, _INT64, _FLOAT32 or _FLOAT64)");
    if (!d_offsets && num_segments != 1) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce: d_offsets == NULL is the one segment [0, n): num_segments must be 1");
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_reduce: at most 2^31 elements");
    if (num_segments == 0) return RSX_OK;
    const bool arg = op >= RSX_REDUCE_ARGMIN;
    const uint64_t vb = (value_kind == RSX_VALUE_INT32 || value_kind == RSX_VALUE_FLOAT32) ? 4 : 8;
    if ((n > 0 && !d_values) || !aligned(d_values, vb))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce: values must be a device pointer aligned to the value size");
    if ((!arg && !d_values_out) || !aligned(d_values_out, vb))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce: the output must be a device pointer aligned to the value size (it may be NULL for the arg ops only)");
    if (arg && (!d_index_out || !aligned(d_index_out, 4)))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce: RSX_REDUCE_ARGMIN / _ARGMAX need d_index_out, a 4-byte aligned device pointer");
    if (!arg && d_index_out) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce: d_index_out must be NULL for RSX_REDUCE_SUM, _MIN and _MAX");
    if (!aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_reduce: offsets must be an 8-byte aligned device pointer");
    const uint64_t vbytes = n * vb, obytes = d_offsets ? (num_segments + 1) * 8 : 0;
    if (check_buffers(e, "rsx_segmented_reduce", {{d_values_out, num_segments * vb}, {d_index_out, num_segments * 4}}, {{d_values, vbytes}, {d_offsets, obytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    return segreduce_enqueue(e, d_values, n, d_offsets, num_segments, op, value_kind, d_values_out, d_index_out);
}
