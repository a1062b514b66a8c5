// capi_expand.inc — C ABI of the segmented expand (rsx_segmented_expand, include/radixsort_hip.h): validate the offsets (and, in gather form,
// the starts) -> the owner of every tile boundary of the absolute 4096-position grid -> per tile the segment, rank and value of every
// position.  Kernels: rsx_expand.hpp.  Nothing of the engine's sort state is read or written: the call needs the first-bad-segment word,
// the status words and tiles + 1 words of scratch.  Included by rsx_capi.hip inside its extern "C" block, after capi_family.inc.

extern "C++" {
namespace {

template <typename Val, bool GATHER>
void expand_launch(rsx_engine* e, const void* values, const uint64_t* off, uint64_t nseg, const uint64_t* starts, const uint32_t* bad, uint32_t ntiles,
                   uint64_t cus, void* vout, uint32_t* sout, uint32_t* rout)
{
    const TileChunks c = tile_chunks(ntiles, cus);
    hipLaunchKernelGGL((rsx::expand_tile_kernel<Val, GATHER>), dim3(c.grid), dim3(rsx::kExpandThreads), 0, e->stream, static_cast<const Val*>(values), off, nseg,
                       starts, bad, e->expand_split, ntiles, c.chunk, static_cast<Val*>(vout), sout, rout);
}

int expand_enqueue(rsx_engine* e, const void* values, uint64_t num_values, uint32_t value_bytes, const uint64_t* off, uint64_t nseg, uint64_t n,
                   const uint64_t* starts, void* vout, uint32_t* sout, uint32_t* rout)
{
    const uint64_t cus = cus_of(e);
    const uint32_t ntiles = static_cast<uint32_t>((n + rsx_expand::kTileSlots - 1) >> rsx_expand::kTileShift);
    int rc = ensure_status_words(e);
    if (rc == RSX_OK) rc = seg_grow(e, &e->expand_split, &e->expand_split_cap, static_cast<uint64_t>(ntiles) + 1, "the tile splits of the segmented expand");
    if (rc != RSX_OK) return rc;
    uint32_t* bad = begin_offset_check(e, cus, nseg, off, n);
    if (starts)
        hipLaunchKernelGGL(rsx::expand_starts_kernel, dim3(offsets_grid(nseg, cus)), dim3(rsx::kExpandSmallThreads), 0, e->stream, off, starts, nseg, num_values, bad);
    const uint32_t sgrid = static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(ntiles) + rsx::kExpandSmallThreads) / rsx::kExpandSmallThreads, cus * 4));
    hipLaunchKernelGGL(rsx::expand_split_kernel, dim3(sgrid), dim3(rsx::kExpandSmallThreads), 0, e->stream, off, nseg, bad, ntiles, e->expand_split, e->seg_status,
                       kStatusCallExpand);
    const bool gather = starts != nullptr && values != nullptr;
    if (!values || value_bytes == 4) {
        if (gather) expand_launch<uint32_t, true>(e, values, off, nseg, starts, bad, ntiles, cus, vout, sout, rout);
        else expand_launch<uint32_t, false>(e, values, off, nseg, starts, bad, ntiles, cus, vout, sout, rout);
    } else {
        if (gather) expand_launch<uint64_t, true>(e, values, off, nseg, starts, bad, ntiles, cus, vout, sout, rout);
        else expand_launch<uint64_t, false>(e, values, off, nseg, starts, bad, ntiles, cus, vout, sout, rout);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

}  // namespace
}  // extern "C++"

int rsx_segmented_expand(rsx_engine* e, const void* d_values, uint64_t num_values, uint32_t value_bytes, const uint64_t* d_offsets, uint64_t num_segments,
                         uint64_t n, const uint64_t* d_starts, uint32_t flags, void* d_values_out, uint32_t* d_segment_out, uint32_t* d_rank_out)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_expand: null engine");
    if (flags & ~static_cast<uint32_t>(RSX_EXPAND_GATHER)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_expand: unknown flag bits (RSX_EXPAND_GATHER is the only one)");
    if (value_bytes != 4 && value_bytes != 8) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_expand: value_bytes must be 4 or 8");
    const bool gather = (flags & RSX_EXPAND_GATHER) != 0;
    if (gather != (d_starts != nullptr)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_expand: d_starts must be given if and only if RSX_EXPAND_GATHER is set");
    if ((d_values != nullptr) != (d_values_out != nullptr))
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_expand: d_values and d_values_out must both be NULL or both be given");
    if (!d_values_out && !d_segment_out && !d_rank_out) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_expand: at least one output must be given");
    if (!gather && d_values && num_values != num_segments)
        return fail(RSX_CALCULATION_FAILED, "rsx_segmented_expand: the fill form has one value per segment (num_values must equal num_segments)");
    if (num_segments >= 0xFFFFFFFFull) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_expand: at most 2^32 - 2 segments");
    if (n > (1ull << 31)) return fail(RSX_CALCULATION_FAILED, "rsx_segmented_expand: at most 2^31 elements");
    if (num_segments == 0 || n == 0) return RSX_OK;
    if (!d_offsets || !aligned(d_offsets, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_expand: offsets must be an 8-byte aligned device pointer");
    if (!aligned(d_starts, 8)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_expand: starts must be an 8-byte aligned device pointer");
    if (!aligned(d_values, value_bytes) || !aligned(d_values_out, value_bytes))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_expand: values and their output must be device pointers aligned to the value size");
    if (!aligned(d_segment_out, 4) || !aligned(d_rank_out, 4))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_segmented_expand: d_segment_out and d_rank_out must be 4-byte aligned device pointers");
    const uint64_t sbytes = num_segments * 8;
    if (check_buffers(e, "rsx_segmented_expand", {{d_values_out, d_values_out ? n * value_bytes : 0}, {d_segment_out, n * 4}, {d_rank_out, n * 4}},
                      {{d_values, num_values * value_bytes}, {d_offsets, sbytes + 8}, {d_starts, sbytes}}) != RSX_OK)
        return RSX_HOST_BUFFERS_FAILED;
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    // (the engine's n, result and tables stay as they were: this call is no sort and uses none of the capacity-sized buffers)
    return expand_enqueue(e, d_values, num_values, value_bytes, d_offsets, num_segments, n, d_starts, d_values_out, d_segment_out, d_rank_out);
}
