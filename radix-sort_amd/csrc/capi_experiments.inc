// capi_experiments.inc — host side of the measured-and-rejected alternatives, compiled into rsx_capi.hip only with -DRSX_EXPERIMENTS
// (tools/build_variant.sh experiments -DRSX_EXPERIMENTS -> tools/_variants/libradixsort_hip_experiments.so).  The product library
// contains none of this: no alternative 8-bit scatter kernels, no inline table scan, no VMM-chunked buffers, no test hooks.
//   RSX_XOPT_* options: include/radixsort_hip_experiments.h.   Results are identical to the product's in every mode (tested on this build).
#pragma once

// ---- 8-bit scatter: kernels 2 / 3 and the staying grid -------------------------------------------------------------------------
constexpr size_t kTickets8Bytes = 8 * rsx::kNumXcd * sizeof(uint32_t);           // at most 8 byte passes (64-bit keys)

template <typename Key>
int ensure_radix8_experiments(rsx_engine* e, int extra)
{
    using L = rsx::Reorder8Layout<Key, kTileThreads, kKeysPerThread>;
    using LP = rsx::Reorder8Layout<Key, kTileThreads, kKeysPerThread, true>;
    if (!e->tickets8) RSX_TRY(hipMalloc(reinterpret_cast<void**>(&e->tickets8), kTickets8Bytes), RSX_INITIALIZATION_FAILED);
    RSX_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&rsx::reorder8_stay_kernel<Key, kTileThreads, kKeysPerThread, false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(L::BYTES) + extra), RSX_INITIALIZATION_FAILED);
    RSX_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&rsx::reorder8_stay_kernel<Key, kTileThreads, kKeysPerThread, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(LP::BYTES) + extra), RSX_INITIALIZATION_FAILED);
    constexpr int lds_v2k = static_cast<int>(rsx::Reorder8V2Layout<Key, kTileThreads, kKeysPerThread, false>::BYTES);
    constexpr int lds_v2p = static_cast<int>(rsx::Reorder8V2Layout<Key, kTileThreads, kKeysPerThread, true>::BYTES);
    RSX_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&rsx::reorder8v2_kernel<Key, kTileThreads, kKeysPerThread, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_v2k),
            RSX_INITIALIZATION_FAILED);
    RSX_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&rsx::reorder8v2_kernel<Key, kTileThreads, kKeysPerThread, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_v2p),
            RSX_INITIALIZATION_FAILED);
    if constexpr (sizeof(Key) == 4) {
        constexpr int lds_packed = static_cast<int>(rsx::Reorder8Layout<uint64_t, kTileThreads, kKeysPerThread>::BYTES);
        RSX_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&rsx::reorder8_stay_kernel<uint64_t, kTileThreads, kKeysPerThread, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_packed + extra),
                RSX_INITIALIZATION_FAILED);
    }
    constexpr int lds_v3k = static_cast<int>(rsx::Reorder8V3Layout<Key, kTileThreads, kKeysPerThread, false>::BYTES);
    constexpr int lds_v3p = static_cast<int>(rsx::Reorder8V3Layout<Key, kTileThreads, kKeysPerThread, true>::BYTES);
    RSX_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&rsx::reorder8v3_kernel<Key, kTileThreads, kKeysPerThread, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_v3k),
            RSX_INITIALIZATION_FAILED);
    RSX_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&rsx::reorder8v3_kernel<Key, kTileThreads, kKeysPerThread, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_v3p),
            RSX_INITIALIZATION_FAILED);
    if (e->lds_atomics_ordered < 0) {
        // kernel 3 ranks keys by the value a returning LDS atomic hands back and relies on lanes that meet on an address being served in
        // ascending lane order — measured behaviour, NOT an architectural promise: checked once per engine on the device it runs on (64 rounds
        // of 16 instructions, patterns from all-equal to all-distinct); if it ever fails the engine keeps the two-round kernel.  Keys always
        // come out sorted; what rests on the property is the ORDER OF EQUAL KEYS' PAYLOADS (stability) — experimental, not guaranteed.
        RSX_TRY(hipMemsetAsync(e->temp + 8, 0, 4, e->stream), RSX_INITIALIZATION_FAILED);
        hipLaunchKernelGGL(rsx::lds_atomic_order_probe_kernel, dim3(1), dim3(256), 0, e->stream, e->temp + 8);
        RSX_TRY(hipGetLastError(), RSX_INITIALIZATION_FAILED);
        uint32_t bad = 1;
        RSX_TRY(hipMemcpyAsync(&bad, e->temp + 8, 4, hipMemcpyDeviceToHost, e->stream), RSX_INITIALIZATION_FAILED);
        RSX_TRY(hipStreamSynchronize(e->stream), RSX_INITIALIZATION_FAILED);
        e->lds_atomics_ordered = bad == 0 ? 1 : 0;
        if (bad) std::fprintf(stderr, "[radixsort_hip] LDS atomics do not return ranks in lane order on this device (%u mismatches): the 8-bit scatter keeps the two-round kernel\n", bad);
    }
    return RSX_OK;
}

// Returns true when an experimental kernel took the launch (*rc = its status); false: the product's launch_reorder8 runs.
template <typename Key>
bool launch_reorder8_experiment(rsx_engine* e, const void* in, void* out, const uint32_t* pin, uint32_t* pout, uint64_t count, const Grid& g,
                                uint32_t chunk_groups, int shift, int byte_pass, bool first_of_chain, int* rc)
{
    const Key flip = flip_mask<Key>(e);
    const bool payload = pin && pout;
    *rc = RSX_OK;
    constexpr size_t lds_v2k = rsx::Reorder8V2Layout<Key, kTileThreads, kKeysPerThread, false>::BYTES;
    constexpr size_t lds_v2p = rsx::Reorder8V2Layout<Key, kTileThreads, kKeysPerThread, true>::BYTES;
    constexpr size_t lds_v3k = rsx::Reorder8V3Layout<Key, kTileThreads, kKeysPerThread, false>::BYTES;
    constexpr size_t lds_v3p = rsx::Reorder8V3Layout<Key, kTileThreads, kKeysPerThread, true>::BYTES;
    if (e->reorder8_version == 3 && e->lds_atomics_ordered == 1) {
        if (payload) {
            hipLaunchKernelGGL((rsx::reorder8v3_kernel<Key, kTileThreads, kKeysPerThread, true>), dim3(g.blocks), dim3(kTileThreads), lds_v3p, e->stream,
                               static_cast<const Key*>(in), static_cast<Key*>(out), pin, pout, e->table8, e->gsum8, e->cbase8, chunk_groups,
                               count, g.ntiles, g.tiles_per_xcd, g.remap, shift, flip);
        } else {
            hipLaunchKernelGGL((rsx::reorder8v3_kernel<Key, kTileThreads, kKeysPerThread, false>), dim3(g.blocks), dim3(kTileThreads), lds_v3k, e->stream,
                               static_cast<const Key*>(in), static_cast<Key*>(out), nullptr, nullptr, e->table8, e->gsum8, e->cbase8, chunk_groups,
                               count, g.ntiles, g.tiles_per_xcd, g.remap, shift, flip);
        }
    } else if (e->reorder8_version == 2) {
        if (payload) {
            hipLaunchKernelGGL((rsx::reorder8v2_kernel<Key, kTileThreads, kKeysPerThread, true>), dim3(g.blocks), dim3(kTileThreads), lds_v2p, e->stream,
                               static_cast<const Key*>(in), static_cast<Key*>(out), pin, pout, e->table8, e->gsum8, e->cbase8, chunk_groups,
                               count, g.ntiles, g.tiles_per_xcd, g.remap, shift, flip);
        } else {
            hipLaunchKernelGGL((rsx::reorder8v2_kernel<Key, kTileThreads, kKeysPerThread, false>), dim3(g.blocks), dim3(kTileThreads), lds_v2k, e->stream,
                               static_cast<const Key*>(in), static_cast<Key*>(out), nullptr, nullptr, e->table8, e->gsum8, e->cbase8, chunk_groups,
                               count, g.ntiles, g.tiles_per_xcd, g.remap, shift, flip);
        }
    } else {
        // kernel 1 as a grid that stays: `stay` workgroups per CU draw tile tickets (zeroed once per chain) and prefetch their next tile
        const int stay = e->r8_stay > 0 ? e->r8_stay : 0;
        const uint32_t stay_blocks = static_cast<uint32_t>(stay) * static_cast<uint32_t>(std::max(e->num_cus, static_cast<int>(rsx::kNumXcd))) / rsx::kNumXcd * rsx::kNumXcd;
        if (stay == 0 || stay_blocks >= g.blocks) return false;
        if (first_of_chain && hipMemsetAsync(e->tickets8, 0, kTickets8Bytes, e->stream) != hipSuccess) {
            *rc = fail(RSX_CALCULATION_FAILED, "hipMemsetAsync(tile tickets)");
            return true;
        }
        uint32_t* tickets = e->tickets8 + static_cast<size_t>(byte_pass) * rsx::kNumXcd;
        const bool packed = sizeof(Key) == 4 && payload && e->r8_packed;
        const dim3 grid(stay_blocks);
        if (packed) {
            const size_t lds = rsx::Reorder8Layout<uint64_t, kTileThreads, kKeysPerThread>::BYTES + r8_extra_lds_for(e, true, false);
            hipLaunchKernelGGL((rsx::reorder8_stay_kernel<uint64_t, kTileThreads, kKeysPerThread, false, true>), grid, dim3(kTileThreads), lds, e->stream,
                               static_cast<const uint64_t*>(in), static_cast<uint64_t*>(out), pin, pout, e->table8, e->gsum8, e->cbase8, chunk_groups,
                               count, g.ntiles, g.tiles_per_xcd, g.remap, shift, static_cast<uint64_t>(flip), tickets);
        } else if (payload) {
            const size_t lds = rsx::Reorder8Layout<Key, kTileThreads, kKeysPerThread, true>::BYTES + r8_extra_lds_for(e, sizeof(Key) == 8, true);
            hipLaunchKernelGGL((rsx::reorder8_stay_kernel<Key, kTileThreads, kKeysPerThread, true>), grid, dim3(kTileThreads), lds, e->stream,
                               static_cast<const Key*>(in), static_cast<Key*>(out), pin, pout, e->table8, e->gsum8, e->cbase8, chunk_groups,
                               count, g.ntiles, g.tiles_per_xcd, g.remap, shift, flip, tickets);
        } else {
            const size_t lds = rsx::Reorder8Layout<Key, kTileThreads, kKeysPerThread>::BYTES + r8_extra_lds_for(e, sizeof(Key) == 8, false);
            hipLaunchKernelGGL((rsx::reorder8_stay_kernel<Key, kTileThreads, kKeysPerThread, false>), grid, dim3(kTileThreads), lds, e->stream,
                               static_cast<const Key*>(in), static_cast<Key*>(out), nullptr, nullptr, e->table8, e->gsum8, e->cbase8, chunk_groups,
                               count, g.ntiles, g.tiles_per_xcd, g.remap, shift, flip, tickets);
        }
    }
    if (hipGetLastError() != hipSuccess) *rc = fail(RSX_CALCULATION_FAILED, "experimental 8-bit scatter launch");
    return true;
}

// ---- the table scan inside the reorder launch ----------------------------------------------------------------------------------
// Co-residency of the inline scan: the workgroups that wait for each other are those of reorder_kernel<..., INLINE_SCAN> (2-5 per CU by
// their LDS and registers), not those of scan_fused_kernel — the limit comes from the occupancy of the instantiated inline kernels with
// their own dynamic LDS, halved as for the fused scan (ADVICE r03).  Also raises the kernels' dynamic-LDS limit.  Called when the option is set.
template <typename Key, bool PAYLOAD, bool LOOKAHEAD>
int inline_scan_prepare_one(rsx_engine* e)
{
    using L = rsx::ReorderLayout<Key, kTileThreads, kKeysPerThread>;
    const void* fn = reinterpret_cast<const void*>(&rsx::reorder_kernel<Key, kTileThreads, kKeysPerThread, PAYLOAD, LOOKAHEAD, false, true>);
    RSX_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(L::BYTES)), RSX_INITIALIZATION_FAILED);
    int per_cu = 0;
    RSX_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kTileThreads, L::BYTES), RSX_INITIALIZATION_FAILED);
    const uint32_t resident = static_cast<uint32_t>(std::max(per_cu, 0)) * static_cast<uint32_t>(std::max(e->num_cus, 0));
    e->inline_scan_limit = std::min<uint32_t>(e->inline_scan_limit, std::min<uint32_t>(resident / 2, rsx::kFusedScanMaxGroups));
    return RSX_OK;
}

template <typename Key>
int inline_scan_prepare(rsx_engine* e)
{
    e->inline_scan_limit = rsx::kFusedScanMaxGroups;
    int rc = e->has_payload ? inline_scan_prepare_one<Key, true, false>(e) : inline_scan_prepare_one<Key, false, false>(e);
    if (rc == RSX_OK) rc = e->has_payload ? inline_scan_prepare_one<Key, true, true>(e) : inline_scan_prepare_one<Key, false, true>(e);
    if (rc != RSX_OK) e->inline_scan_limit = 0;
    return rc;
}

// Reorder launch with the table scan inside it (rsx::InlineScanArgs): LOOKAHEAD counts the next pass into `next_counts`.
template <typename Key, bool PAYLOAD, bool LOOKAHEAD>
int launch_reorder_inline(rsx_engine* e, const void* in, void* out, const uint32_t* pin, uint32_t* pout, uint64_t count, int shift, int next_shift,
                          uint32_t* next_counts, const rsx::InlineScanArgs& iscan)
{
    using L = rsx::ReorderLayout<Key, kTileThreads, kKeysPerThread>;
    static_assert(L::BYTES >= sizeof(rsx::FusedScanLds), "the scan's scratch lies over the reorder's dynamic LDS");
    const Grid g = grid_for(e, count);
    e->last_in = in;
    e->last_shift = shift;
    Bracket b(e, PH_REORDER);
    hipLaunchKernelGGL((rsx::reorder_kernel<Key, kTileThreads, kKeysPerThread, PAYLOAD, LOOKAHEAD, false, true>), dim3(g.blocks), dim3(kTileThreads), L::BYTES, e->stream,
                       static_cast<const Key*>(in), static_cast<Key*>(out), pin, pout, e->table, count, g.ntiles, g.tiles_per_xcd, g.remap, shift, flip_mask<Key>(e),
                       static_cast<uint32_t>(RSX_RADIX - 1), next_counts, next_shift, static_cast<const uint32_t*>(nullptr), Key{0}, Key{0}, split_set<Key>(e, 0),
                       rsx::SelfScanArgs{nullptr, nullptr, nullptr}, iscan);
    RSX_TRY(hipGetLastError(), RSX_CALCULATION_FAILED);
    return RSX_OK;
}

// Mid-size tables (beyond the self-scan, at most inline_scan_max_groups scan groups): one histogram launch, then ONE launch per pass —
// the first workgroups of every reorder launch scan the pass's table before they turn to their own tiles (rsx::InlineScanArgs), so the
// chain is passes + 1 dependent launches instead of 2 passes + 1.  Two count buffers alternate between "scanned (and zeroed) by this
// launch" and "filled by this launch's look-ahead".
template <typename Key>
int sort_inline_enqueue(rsx_engine* e, const SortJob& job)
{
    const uint64_t count = job.n;
    const uint32_t ntiles = static_cast<uint32_t>(e->ntiles(count));
    const uint32_t ngroups = (ntiles + rsx::kScanTiles - 1) / rsx::kScanTiles;
    PingPong pp(e, job);
    Bracket whole(e, PH_TOTAL);
    const size_t rows = static_cast<size_t>(ntiles) * RSX_RADIX * 4;
    RSX_TRY(hipMemsetAsync(e->counts_next, 0, rows, e->stream), RSX_CALCULATION_FAILED);      // (a sort that failed midway may have left counts)
    RSX_TRY(hipMemsetAsync(e->counts_next2, 0, rows, e->stream), RSX_CALCULATION_FAILED);
    int rc = launch_histogram<Key>(e, pp.in, count, job.first * RSX_RADIX_BITS, RSX_RADIX - 1);
    if (rc != RSX_OK) return rc;
    uint32_t* bufs[2] = {e->counts_next, e->counts_next2};
    int filled = 1;                      // bufs[filled] holds the counts the NEXT launch scans (none before the first pass); its look-ahead fills the other
    for (int pass = job.first; pass < job.last; ++pass) {
        const bool first = pass == job.first, last = pass + 1 == job.last;
        pp.target(e, job, last);
        const int shift = pass * RSX_RADIX_BITS;
        if (++e->scan_epoch == 0) e->scan_epoch = 1;
        const rsx::InlineScanArgs iscan{e->gsums, e->globsum2, e->temp, bufs[filled], e->scan_ready, e->scan_timeout, e->scan_epoch, ngroups, first ? 0 : 1};
        uint32_t* next = bufs[filled ^ 1];
        if (job.payload) {
            rc = last ? launch_reorder_inline<Key, true, false>(e, pp.in, pp.out, pp.pin, pp.pout, count, shift, 0, next, iscan)
                      : launch_reorder_inline<Key, true, true>(e, pp.in, pp.out, pp.pin, pp.pout, count, shift, shift + RSX_RADIX_BITS, next, iscan);
        } else {
            rc = last ? launch_reorder_inline<Key, false, false>(e, pp.in, pp.out, nullptr, nullptr, count, shift, 0, next, iscan)
                      : launch_reorder_inline<Key, false, true>(e, pp.in, pp.out, nullptr, nullptr, count, shift, shift + RSX_RADIX_BITS, next, iscan);
        }
        if (rc != RSX_OK) return rc;
        filled ^= 1;
        pp.advance();
    }
    e->counted_keys = nullptr;
    e->globsum_live = e->globsum2;
    e->table_valid = true;
    e->globsum_valid = true;
    finish_chain(e, job, pp.in);
    return RSX_OK;
}

// the inline chain takes a sort when the option is on, the chain is the plain look-ahead one and the table is mid-size
bool inline_scan_takes(const rsx_engine* e, const SortJob& job)
{
    const uint32_t groups = static_cast<uint32_t>((e->ntiles(job.n) + rsx::kScanTiles - 1) / rsx::kScanTiles);
    // (profile mode 1 keeps the separate scan launches: timeScan / timePaste would otherwise be empty; a captured graph would replay a stale epoch)
    return e->inline_scan && e->lookahead && e->fused_scan && !e->use_graph && e->profile != 1 && job.n > 0 && job.first < job.last &&
           e->ntiles(job.n) > static_cast<uint64_t>(rsx::kSmallScanMaxTiles) && groups <= std::min(e->inline_scan_max_groups, e->inline_scan_limit);
}

// ---- large buffers as VMM chunks mapped in a chosen order (env RSX_ALLOC_MODE = 1 | 2, RSX_ALLOC_CHUNK_MB) ------------------------
hipError_t big_alloc(rsx_engine* e, void** out, size_t bytes)
{
    *out = nullptr;
    rsx_engine::BigBuf b;
    if (e->alloc_mode == 0 || bytes < (64u << 20)) {
        const hipError_t err = hipMalloc(&b.base, bytes);
        if (err != hipSuccess) return err;
        b.size = bytes;
        e->big.push_back(b);
        *out = b.base;
        return hipSuccess;
    }
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = e->device;
    size_t gran = 0;
    hipError_t err = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended);
    if (err != hipSuccess) return err;
    // chunks of at least 2 MiB and at most 1024 of them per buffer: the first version took the recommended granularity as it came
    // (small on this stack) and spent minutes creating and mapping chunks (profiles/r03_fault_vmm_alloc_silence.txt)
    size_t chunk = e->alloc_chunk ? e->alloc_chunk : (static_cast<size_t>(32) << 20);
    chunk = std::max(chunk, static_cast<size_t>(2) << 20);
    chunk = std::max(chunk, (bytes + 1023) / 1024);
    chunk = (chunk + gran - 1) / gran * gran;
    const size_t nchunks = (bytes + chunk - 1) / chunk;
    if (std::getenv("RSX_DEBUG_ALLOC")) std::fprintf(stderr, "[radixsort_hip] big_alloc: %zu bytes as %zu chunks of %zu (granularity %zu), mode %d\n", bytes, nchunks, chunk, gran, e->alloc_mode);
    b.size = nchunks * chunk;
    if ((err = hipMemAddressReserve(&b.base, b.size, chunk, nullptr, 0)) != hipSuccess) return err;
    auto undo = [&](hipError_t why) {
        for (auto h : b.chunks) (void)hipMemRelease(h);
        (void)hipMemAddressFree(b.base, b.size);
        return why;
    };
    for (size_t i = 0; i < nchunks; ++i) {
        hipMemGenericAllocationHandle_t h;
        if ((err = hipMemCreate(&h, chunk, &prop, 0)) != hipSuccess) return undo(err);
        b.chunks.push_back(h);
    }
    std::vector<size_t> order(nchunks);
    for (size_t i = 0; i < nchunks; ++i) order[i] = i;
    if (e->alloc_mode == 2) {
        // a fixed pseudo-random permutation (xorshift; the same for every buffer of the same length: reproducible runs)
        unsigned long long x = 0x9E3779B97F4A7C15ull ^ (nchunks * 0x100000001B3ull);
        for (size_t i = nchunks - 1; i > 0; --i) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            std::swap(order[i], order[static_cast<size_t>(x % (i + 1))]);
        }
    }
    for (size_t i = 0; i < nchunks; ++i) {
        if ((err = hipMemMap(static_cast<char*>(b.base) + i * chunk, chunk, 0, b.chunks[order[i]], 0)) != hipSuccess) {
            if (i) (void)hipMemUnmap(b.base, i * chunk);
            return undo(err);
        }
    }
    hipMemAccessDesc acc = {};
    acc.location.type = hipMemLocationTypeDevice;
    acc.location.id = e->device;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    if ((err = hipMemSetAccess(b.base, b.size, &acc, 1)) != hipSuccess) {
        (void)hipMemUnmap(b.base, b.size);
        return undo(err);
    }
    e->big.push_back(b);
    *out = b.base;
    return hipSuccess;
}

bool big_free(rsx_engine* e, void* p)
{
    if (!p) return true;
    for (size_t i = 0; i < e->big.size(); ++i) {
        if (e->big[i].base != p) continue;
        rsx_engine::BigBuf b = e->big[i];
        e->big.erase(e->big.begin() + static_cast<long>(i));
        if (b.chunks.empty()) return hipFree(p) == hipSuccess;
        bool ok = hipMemUnmap(b.base, b.size) == hipSuccess;
        for (auto h : b.chunks) ok = (hipMemRelease(h) == hipSuccess) && ok;
        return (hipMemAddressFree(b.base, b.size) == hipSuccess) && ok;
    }
    return hipFree(p) == hipSuccess;
}

