// capi_msd.inc — C ABI of the sharded sort's exchange step on the top B <= 8 key bits (rsx_msd_*, include/radixsort_hip.h):
// count -> [all_gather by the caller] -> scatter into wave-major staging -> device-side plan -> one push per wave.  Kernels: rsx_msd.hpp.
// Included by rsx_capi.hip inside its extern "C" block.

namespace {

constexpr int kMsdAlign = 4;          // waves start on multiples of 4 keys in a receive buffer (16 bytes for 32-bit keys: the local sort loads 16 bytes per lane)

int msd_check(const rsx_engine* e, int bits, int world, const char* who)
{
    if (bits < 1 || bits > 8) return fail(RSX_CALCULATION_FAILED, (std::string(who) + ": 1..8 partition bits").c_str());
    if (world < 1 || world > rsx::kMsdMaxWorld || (world & (world - 1)) != 0 || world > (1 << bits))
        return fail(RSX_CALCULATION_FAILED, (std::string(who) + ": world must be a power of two, at most 16 and at most 2^bits").c_str());
    (void)e;
    return RSX_OK;
}

// the buffers of the exchange step, on first use (never inside a stream capture: the sharded callers do not capture)
int ensure_msd(rsx_engine* e)
{
    if (!e->msd_plan) RSX_TRY(hipMalloc(reinterpret_cast<void**>(&e->msd_plan), sizeof(rsx::MsdPlan)), RSX_INITIALIZATION_FAILED);
    if (!e->msd_starts) RSX_TRY(hipMalloc(reinterpret_cast<void**>(&e->msd_starts), rsx::kRadix8 * 4), RSX_INITIALIZATION_FAILED);
    if (!e->msd_plan_host) RSX_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->msd_plan_host), sizeof(rsx::MsdPlan), hipHostMallocDefault), RSX_HOST_BUFFERS_FAILED);
    if (!e->msd_event) RSX_TRY(hipEventCreateWithFlags(&e->msd_event, hipEventDisableTiming), RSX_INITIALIZATION_FAILED);
    if (!e->msd_scatter_event) RSX_TRY(hipEventCreateWithFlags(&e->msd_scatter_event, hipEventDisableTiming), RSX_INITIALIZATION_FAILED);
    return RSX_OK;
}

}  // namespace

int rsx_msd_count(rsx_engine* e, const void* d_keys, uint64_t n, int bits, int world, uint64_t* d_counts)
{
    if (!e || !d_counts) return fail(RSX_CALCULATION_FAILED, "rsx_msd_count: null argument");
    if (e->codec()) return refuse_codec("rsx_msd_count");
    int rc = msd_check(e, bits, world, "rsx_msd_count");
    if (rc != RSX_OK) return rc;
    if (n > e->capacity) return fail(RSX_RESIZE_FAILED, "rsx_msd_count: beyond capacity");
    if (n > 0 && (!d_keys || !aligned16(d_keys))) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_msd_count: keys must be a 16-byte aligned device pointer");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    e->counted_keys = nullptr;
    if (n == 0) {
        RSX_TRY(hipMemsetAsync(d_counts, 0, rsx::kRadix8 * 8, e->stream), RSX_CALCULATION_FAILED);
        e->msd_keys = nullptr;
        e->msd_n = 0;
        e->msd_bits = bits;
        e->msd_world = world;
        if ((rc = ensure_msd(e)) != RSX_OK) return rc;
        RSX_TRY(hipMemsetAsync(e->msd_starts, 0, rsx::kRadix8 * 4, e->stream), RSX_CALCULATION_FAILED);
        return RSX_OK;
    }
#if RSX_TILE_THREADS == 256
    rc = RSX_BY_KEY(e, ensure_radix8<uint32_t>(e), ensure_radix8<uint64_t>(e));
    if (rc == RSX_OK) rc = ensure_msd(e);
    if (rc != RSX_OK) return rc;
    const Grid g = grid_for(e, n);
    const Scan8Shape s = scan8_shape(g.ntiles);
    const int shift = e->key_bytes * 8 - 8;             // always the top BYTE: 256 fine buckets; `bits` decides how they group into (wave, rank)
    {
        Bracket b(e, PH_HISTO);
        if (e->key_bytes == 4) {
            hipLaunchKernelGGL((rsx::histogram8_kernel<uint32_t, kTileThreads, kKeysPerThread>), dim3(g.blocks), dim3(kTileThreads), 0, e->stream,
                               static_cast<const uint32_t*>(d_keys), e->counts8, n, g.ntiles, g.tiles_per_xcd, g.remap, shift, flip_mask<uint32_t>(e));
        } else {
            hipLaunchKernelGGL((rsx::histogram8_kernel<uint64_t, kTileThreads, kKeysPerThread>), dim3(g.blocks), dim3(kTileThreads), 0, e->stream,
                               static_cast<const uint64_t*>(d_keys), e->counts8, n, g.ntiles, g.tiles_per_xcd, g.remap, shift, flip_mask<uint64_t>(e));
        }
    }
    {
        Bracket b(e, PH_SCAN);
        hipLaunchKernelGGL(rsx::scan8_blocks_kernel, dim3(s.ngroups), dim3(rsx::kRadix8), 0, e->stream, e->counts8, e->table8, e->gsum8, g.ntiles);
        hipLaunchKernelGGL(rsx::scan8_chunks_kernel<false>, dim3(s.nchunks), dim3(rsx::kRadix8), 0, e->stream, e->gsum8, e->csum8, s.ngroups, s.chunk_groups, e->cbase8, e->temp);
        hipLaunchKernelGGL(rsx::msd_top_kernel, dim3(1), dim3(rsx::kRadix8), 0, e->stream, e->csum8, e->cbase8, s.nchunks, static_cast<uint32_t>(bits),
                           static_cast<uint32_t>(world), reinterpret_cast<unsigned long long*>(d_counts), e->msd_starts, e->temp);
    }
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    e->table_valid = false;
    e->globsum_valid = false;
    e->msd_keys = d_keys;
    e->msd_n = n;
    e->msd_bits = bits;
    e->msd_world = world;
    return RSX_OK;
#else
    return fail(RSX_CALCULATION_FAILED, "rsx_msd_count: this build has no 8-bit kernels");
#endif
}

int rsx_msd_scatter(rsx_engine* e, const void* d_keys, const uint32_t* d_payload, uint64_t n, void* d_staging, uint32_t* d_staging_payload)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_msd_scatter: null engine");
    if (e->codec()) return refuse_codec("rsx_msd_scatter");
    if (n == 0) {
        e->msd_keys = nullptr;
        e->msd_scattered = false;           // nothing was enqueued: a push has nothing to wait for (all its segments are empty)
        return RSX_OK;
    }
    if (d_keys != e->msd_keys || n != e->msd_n) return fail(RSX_CALCULATION_FAILED, "rsx_msd_scatter: must follow rsx_msd_count on the same keys");
    e->msd_keys = nullptr;              // table8 / cbase8 are consumed by this call
    if (!d_staging || !aligned16(d_staging)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_msd_scatter: staging must be a 16-byte aligned device pointer");
    const bool with_payload = e->has_payload && d_payload && d_staging_payload;
    if (e->has_payload && !with_payload) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_msd_scatter: payload engine needs payload buffers");
    if (with_payload && !aligned16(d_payload)) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_msd_scatter: the payload input must be 16-byte aligned (it is read 16 bytes per lane)");
    if (overlaps(d_staging, n * static_cast<uint64_t>(e->key_bytes), d_keys, n * static_cast<uint64_t>(e->key_bytes)))
        return fail(RSX_HOST_BUFFERS_FAILED, "rsx_msd_scatter: input and staging overlap");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
#if RSX_TILE_THREADS == 256
    const Grid g = grid_for(e, n);
    const Scan8Shape s = scan8_shape(g.ntiles);
    const int shift = e->key_bytes * 8 - 8;
    const uint32_t* pin = with_payload ? d_payload : nullptr;
    uint32_t* pout = with_payload ? d_staging_payload : nullptr;
    int rc;
    {
        Bracket b(e, PH_REORDER);
        rc = RSX_BY_KEY(e, launch_reorder8<uint32_t>(e, d_keys, d_staging, pin, pout, n, g, s.chunk_groups, shift),
                        launch_reorder8<uint64_t>(e, d_keys, d_staging, pin, pout, n, g, s.chunk_groups, shift));
    }
    if (rc != RSX_OK) return rc;
    RSX_TRY(hipEventRecord(e->msd_scatter_event, e->stream), RSX_CALCULATION_FAILED);       // pushes on another stream wait for this
    e->msd_scattered = true;
    return RSX_OK;
#else
    return fail(RSX_CALCULATION_FAILED, "rsx_msd_scatter: this build has no 8-bit kernels");
#endif
}

int rsx_msd_plan(rsx_engine* e, const uint64_t* d_table, uint32_t stride, uint32_t cap_at, int rank, int grouping, void* hip_stream)
{
    if (grouping != 0 && grouping != 1) return fail(RSX_CALCULATION_FAILED, "rsx_msd_plan: grouping is 0 (every wave aligned) or 1 (doubling groups)");
    if (!e || !d_table) return fail(RSX_CALCULATION_FAILED, "rsx_msd_plan: null argument");
    if (e->codec()) return refuse_codec("rsx_msd_plan");
    if (e->msd_bits == 0) return fail(RSX_CALCULATION_FAILED, "rsx_msd_plan: must follow rsx_msd_count");
    const uint32_t nbuckets = 1u << e->msd_bits;
    if (rank < 0 || rank >= e->msd_world || stride < nbuckets || cap_at < nbuckets || cap_at + 3 > stride)
        return fail(RSX_CALCULATION_FAILED, "rsx_msd_plan: rank outside the world, or a row too short for its 2^bits counts + two capacities + status word");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    const int rc = ensure_msd(e);
    if (rc != RSX_OK) return rc;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    hipLaunchKernelGGL(rsx::msd_layout_kernel, dim3(1), dim3(rsx::kRadix8), 0, s, reinterpret_cast<const unsigned long long*>(d_table), stride, cap_at, nbuckets,
                       static_cast<uint32_t>(e->msd_world), static_cast<uint32_t>(rank), static_cast<uint32_t>(kMsdAlign), static_cast<uint32_t>(8 - e->msd_bits), static_cast<uint32_t>(grouping),
                       e->msd_starts, e->msd_plan);
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    // what the host needs (its own waves, the loads, the verdict) follows the segments in the struct
    constexpr size_t host_at = offsetof(rsx::MsdPlan, wave_start);
    RSX_TRY(hipMemcpyAsync(reinterpret_cast<char*>(e->msd_plan_host) + host_at, reinterpret_cast<const char*>(e->msd_plan) + host_at, sizeof(rsx::MsdPlan) - host_at,
                           hipMemcpyDeviceToHost, s), RSX_CALCULATION_FAILED);
    RSX_TRY(hipEventRecord(e->msd_event, s), RSX_CALCULATION_FAILED);
    e->msd_planned = true;
    return RSX_OK;
}

int rsx_msd_plan_wait(rsx_engine* e, uint64_t* wave_start, uint64_t* wave_count, uint64_t* loads, uint64_t* verdict)
{
    if (!e) return fail(RSX_CALCULATION_FAILED, "rsx_msd_plan_wait: null engine");
    if (e->codec()) return refuse_codec("rsx_msd_plan_wait");
    if (!e->msd_planned) return fail(RSX_CALCULATION_FAILED, "rsx_msd_plan_wait: must follow rsx_msd_plan");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    RSX_TRY(hipEventSynchronize(e->msd_event), RSX_CALCULATION_FAILED);
    const rsx::MsdPlan* p = e->msd_plan_host;
    const uint32_t waves = (1u << e->msd_bits) / static_cast<uint32_t>(e->msd_world);
    for (uint32_t w = 0; w < waves; ++w) {
        if (wave_start) wave_start[w] = p->wave_start[w];
        if (wave_count) wave_count[w] = p->wave_count[w];
    }
    for (int r = 0; r < e->msd_world && loads; ++r) loads[r] = p->load[r];
    if (verdict) *verdict = p->verdict;
    return RSX_OK;
}

int rsx_msd_push(rsx_engine* e, int wave, const void* d_staging, const uint32_t* d_staging_payload, const uint64_t* d_peer_keys, const uint64_t* d_peer_payload, int parts,
                 void* hip_stream)
{
    if (!e || !d_peer_keys) return fail(RSX_CALCULATION_FAILED, "rsx_msd_push: null argument");
    if (e->codec()) return refuse_codec("rsx_msd_push");
    if (!e->msd_planned) return fail(RSX_CALCULATION_FAILED, "rsx_msd_push: must follow rsx_msd_plan");
    const int waves = (1 << e->msd_bits) / e->msd_world;
    if (wave < 0 || wave >= waves) return fail(RSX_CALCULATION_FAILED, "rsx_msd_push: wave out of range");
    // an empty shard has an empty staging buffer (often no address at all): its segments are all empty, the kernel never reads it
    const bool has_keys = e->msd_n > 0;
    if (has_keys && !d_staging) return fail(RSX_CALCULATION_FAILED, "rsx_msd_push: null staging buffer");
    if (e->has_payload && (!d_peer_payload || (has_keys && !d_staging_payload))) return fail(RSX_HOST_BUFFERS_FAILED, "rsx_msd_push: payload engine needs payload buffers");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    if (parts <= 0) parts = std::max(16, 128 / e->msd_world);       // at least 128 workgroups per wave: enough loads in flight for a link- (or, on one GPU, HBM-) bound copy
    if (parts > 256) parts = 256;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream;
    RSX_TRY(hipStreamWaitEvent(s, e->msd_event, 0), RSX_CALCULATION_FAILED);                  // the plan may have been made on another stream
    if (s != e->stream && e->msd_scattered) RSX_TRY(hipStreamWaitEvent(s, e->msd_scatter_event, 0), RSX_CALCULATION_FAILED);      // ... and the staging buffer filled on the engine's
    hipLaunchKernelGGL(rsx::msd_push_kernel, dim3(static_cast<uint32_t>(parts), static_cast<uint32_t>(e->msd_world)), dim3(256), 0, s, e->msd_plan,
                       static_cast<uint32_t>(wave), static_cast<uint32_t>(e->msd_world), static_cast<uint32_t>(e->key_bytes / 4), static_cast<const uint32_t*>(d_staging),
                       e->has_payload ? d_staging_payload : static_cast<const uint32_t*>(nullptr), reinterpret_cast<const unsigned long long*>(d_peer_keys),
                       reinterpret_cast<const unsigned long long*>(d_peer_payload));
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

// ---- plumbing for hosts that do not link HIP themselves (radix-sort_amd/host: g++ over this C ABI) ---------------------------------
int rsx_copy_to_device(rsx_engine* e, void* d_dst, const void* host_src, uint64_t bytes)
{
    if (!e || (bytes && (!d_dst || !host_src))) return fail(RSX_DATA_UPLOAD_FAILED, "rsx_copy_to_device: null argument");
    if (bind_device(e, RSX_DATA_UPLOAD_FAILED) != RSX_OK) return RSX_DATA_UPLOAD_FAILED;
    if (bytes) RSX_TRY(hipMemcpyAsync(d_dst, host_src, static_cast<size_t>(bytes), hipMemcpyHostToDevice, e->stream), RSX_DATA_UPLOAD_FAILED);
    return RSX_OK;
}

int rsx_copy_from_device(rsx_engine* e, void* host_dst, const void* d_src, uint64_t bytes)
{
    if (!e || (bytes && (!host_dst || !d_src))) return fail(RSX_DATA_DOWNLOAD_FAILED, "rsx_copy_from_device: null argument");
    if (bind_device(e, RSX_DATA_DOWNLOAD_FAILED) != RSX_OK) return RSX_DATA_DOWNLOAD_FAILED;
    if (bytes) RSX_TRY(hipMemcpyAsync(host_dst, d_src, static_cast<size_t>(bytes), hipMemcpyDeviceToHost, e->stream), RSX_DATA_DOWNLOAD_FAILED);
    return RSX_OK;
}

int rsx_copy_on_device(rsx_engine* e, void* d_dst, const void* d_src, uint64_t bytes)
{
    if (!e || (bytes && (!d_dst || !d_src))) return fail(RSX_CALCULATION_FAILED, "rsx_copy_on_device: null argument");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    if (bytes) RSX_TRY(hipMemcpyAsync(d_dst, d_src, static_cast<size_t>(bytes), hipMemcpyDeviceToDevice, e->stream), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

int rsx_wait_for(rsx_engine* e, rsx_engine* other)
{
    if (!e || !other) return fail(RSX_CALCULATION_FAILED, "rsx_wait_for: null engine");
    if (e == other || e->stream == other->stream) return RSX_OK;
    // The event belongs to the WAITER (several threads may wait for one engine at the same time: rank threads of a sharded sort) but lives
    // on the device of the stream it is recorded on (an event can only be recorded on a stream of its own device): one per other device.
    if (bind_device(other, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    hipEvent_t& ev = e->order_events[other->device];
    if (!ev) RSX_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming), RSX_CALCULATION_FAILED);
    RSX_TRY(hipEventRecord(ev, other->stream), RSX_CALCULATION_FAILED);
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    RSX_TRY(hipStreamWaitEvent(e->stream, ev, 0), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

int rsx_record_mark(rsx_engine* e, int slot)
{
    if (!e || slot < 0 || slot >= RSX_MAX_MARKS) return fail(RSX_CALCULATION_FAILED, "rsx_record_mark: null engine or slot outside 0..RSX_MAX_MARKS-1");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    hipEvent_t& ev = e->marks[slot];
    if (!ev) RSX_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming), RSX_CALCULATION_FAILED);
    RSX_TRY(hipEventRecord(ev, e->stream), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

int rsx_wait_mark(rsx_engine* e, rsx_engine* other, int slot)
{
    if (!e || !other || slot < 0 || slot >= RSX_MAX_MARKS) return fail(RSX_CALCULATION_FAILED, "rsx_wait_mark: null engine or slot outside 0..RSX_MAX_MARKS-1");
    if (!other->marks[slot]) return fail(RSX_CALCULATION_FAILED, "rsx_wait_mark: that mark was never recorded");
    if (bind_device(e, RSX_CALCULATION_FAILED) != RSX_OK) return RSX_CALCULATION_FAILED;
    RSX_TRY(hipStreamWaitEvent(e->stream, other->marks[slot], 0), RSX_CALCULATION_FAILED);
    return RSX_OK;
}
