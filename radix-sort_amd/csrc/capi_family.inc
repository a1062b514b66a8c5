// capi_family.inc — the host front end that the fourteen segmented calls share (capi_segmented.inc ... capi_join.inc): the buffer rules, the
// 32/64-bit dispatch, the engine state after a call, the scratch that grows on demand, the tile arithmetic, the check of the offsets and
// the table scan.  No kernel of its own: every launch in here is one that each call used to spell out itself.  The address arithmetic
// is in rsx_args.hpp.  Included by rsx_capi.hip first inside its extern "C" block (templates and helpers: C++ linkage).

extern "C++" {
namespace {

using rsx_args::Buf;

// The rules of rsx_args::clash for one call: `outs` and `ins` are the caller's buffers, absent ones (null or zero bytes) included.
int check_buffers(const rsx_engine* e, const char* call, std::initializer_list<Buf> outs, std::initializer_list<Buf> ins)
{
    const uint64_t ebytes = e->capacity * static_cast<uint64_t>(e->key_bytes), epbytes = e->capacity * 4;
    const Buf engine[4] = {{e->keys[0], ebytes}, {e->perm[0], epbytes}, {e->keys[1], ebytes}, {e->perm[1], epbytes}};
    const char* what = nullptr;
    switch (rsx_args::clash(engine, outs, ins)) {
    case rsx_args::Clash::None: return RSX_OK;
    case rsx_args::Clash::Engine: what = ": an input or output overlaps the engine's own buffers"; break;
    case rsx_args::Clash::Outputs: what = ": two outputs overlap"; break;
    case rsx_args::Clash::OutputInput: what = ": an output overlaps an input (no call of the family has an in-place form but rsx_segmented_scan's)"; break;
    }
    return fail(RSX_HOST_BUFFERS_FAILED, (std::string(call) + what).c_str());
}

// f(Key{}) for the engine's key width: an entry point writes its argument list once, with Key = decltype of f's parameter.
template <typename F>
int by_key(const rsx_engine* e, F&& f)
{
    return e->key_bytes == 4 ? f(uint32_t{}) : f(uint64_t{});
}

// As after rsx_sort_from_to: the result lives in the caller's buffers only, and the engine's tables are not this call's.
void result_is_external(rsx_engine* e, uint64_t n)
{
    e->n = n;
    e->result_external = true;
    e->counted_keys = nullptr;
    e->table_valid = false;
    e->globsum_valid = false;
}

uint64_t cus_of(const rsx_engine* e)
{
    return e->num_cus > 0 ? static_cast<uint64_t>(e->num_cus) : 256u;
}

// ---- scratch ----------------------------------------------------------------------------------------------------------------

// Launch bounds that depend on n and the segment count only (the host never reads the offsets).
struct SegShape {
    uint64_t nblocks;       // classify workgroups
    uint64_t max_large;     // large segments (> 4096 keys) there can be
    uint64_t max_tiles;     // tiles of the chain: the 4096-key grid plus at most one partial tile per large segment
};

SegShape seg_shape(uint64_t n, uint64_t nseg)
{
    SegShape s;
    s.nblocks = (nseg + rsx::kSegPerBlock - 1) / rsx::kSegPerBlock;
    s.max_large = std::min<uint64_t>(nseg, n / (rsx::kSegTileKeys + 1));
    s.max_tiles = s.max_large ? (n + rsx::kSegTileKeys - 1) / rsx::kSegTileKeys + s.max_large : 0;
    return s;
}

// One scratch buffer of the family: grown to `want` elements on demand, never inside a stream capture.
// (The text names rsx_segmented_sort whichever call grows the buffer: a known wart, left as it is.)
template <typename T>
int seg_grow(rsx_engine* e, T** p, uint64_t* cap, uint64_t want, const char* what)
{
    if (want <= *cap && *p) return RSX_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (e->stream && hipStreamIsCapturing(e->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return fail(RSX_CALCULATION_FAILED, (std::string("rsx_segmented_sort: ") + what + " must grow, which cannot happen inside a stream capture (run one call of this size first)").c_str());
    if (*p) {
        RSX_TRY(hipStreamSynchronize(e->stream), RSX_CALCULATION_FAILED);      // a pending call may still use the old buffer
        RSX_TRY(hipFree(*p), RSX_CLEANUP_FAILED);
        *p = nullptr;
        *cap = 0;
    }
    const uint64_t n = std::max<uint64_t>(want, 1);
    RSX_TRY(hipMalloc(reinterpret_cast<void**>(p), static_cast<size_t>(n) * sizeof(T)), RSX_INITIALIZATION_FAILED);
    *cap = n;
    return RSX_OK;
}

int ensure_segmented(rsx_engine* e, const SegShape& s, uint64_t nseg)
{
    int rc = RSX_OK;
    if (!e->seg_status_host) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (e->stream && hipStreamIsCapturing(e->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return fail(RSX_CALCULATION_FAILED, "rsx_segmented_sort: the first call of an engine cannot run inside a stream capture (it allocates)");
        RSX_TRY(hipMalloc(reinterpret_cast<void**>(&e->seg_hdr), sizeof(rsx::SegHeader)), RSX_INITIALIZATION_FAILED);
        RSX_TRY(hipMalloc(reinterpret_cast<void**>(&e->seg_temp), 64), RSX_INITIALIZATION_FAILED);
        RSX_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->seg_status_host), 64, hipHostMallocMapped), RSX_HOST_BUFFERS_FAILED);
        e->seg_status_host[0] = 0;
        e->seg_status_host[1] = 0;       // (which call reported: capi_merge.inc)
        RSX_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&e->seg_status), e->seg_status_host, 0), RSX_HOST_BUFFERS_FAILED);
    }
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_bsum, &e->seg_bsum_cap, s.nblocks * rsx::SF_STRIDE, "the classify block sums");
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_list, &e->seg_list_cap, nseg, "the small-segment list");
    if (rc == RSX_OK && s.max_large) {
        const uint64_t groups = (s.max_tiles + rsx::kScanTiles - 1) / rsx::kScanTiles;
        rc = seg_grow(e, &e->seg_large, &e->seg_large_cap, s.max_large, "the large-segment table");
        if (rc == RSX_OK) rc = seg_grow(e, &e->seg_tstart, &e->seg_tstart_cap, s.max_large + 1, "the tile starts");
        if (rc == RSX_OK) rc = seg_grow(e, &e->seg_table, &e->seg_table_cap, rsx::kRadix * s.max_tiles, "the segmented table");
        if (rc == RSX_OK) rc = seg_grow(e, &e->seg_gsum, &e->seg_gsum_cap, rsx::kRadix * groups, "the group sums");
        if (rc == RSX_OK) rc = seg_grow(e, &e->seg_gsum2, &e->seg_gsum2_cap, rsx::kRadix * groups, "the scanned group sums");
    }
    return rc;
}

// The calls that are no sort: the status words and the first-bad-segment word, none of the sort's scratch.
int ensure_status_words(rsx_engine* e)
{
    return ensure_segmented(e, SegShape{1, 0, 0}, 1);
}

// ---- tile arithmetic --------------------------------------------------------------------------------------------------------
// Launch bounds from the element and segment counts alone.  A workgroup walks `chunk` consecutive tiles (more than one above cus * 16).

struct TileChunks {
    uint32_t chunk, grid;
};

TileChunks tile_chunks(uint32_t ntiles, uint64_t cus)
{
    TileChunks c;
    c.chunk = static_cast<uint32_t>((ntiles + cus * 16 - 1) / (cus * 16));
    c.grid = (ntiles + c.chunk - 1) / c.chunk;
    return c;
}

// The flat per-tile table of the calls that count, scan and write: one entry per tile of the global grid and one more (rsx_unique.hpp).
struct TileTable {
    uint32_t ntiles, ntab;      // tiles of (1 << tile_shift) elements; entries
    uint32_t npad, nrow;        // entries padded to the scan kernels' 16 rows; entries per row (the scan's "tiles")
    uint32_t ngroups;           // scan workgroups
    uint32_t chunk;             // tiles (and entries) per workgroup
    uint32_t tgrid, wgrid;      // workgroups over the padded entries (count kernels) and over the tiles (write kernels)
};

TileTable tile_table(uint64_t total, int tile_shift, uint64_t cus)
{
    TileTable t;
    t.ntiles = static_cast<uint32_t>((total + (1ull << tile_shift) - 1) >> tile_shift);
    t.ntab = t.ntiles + 1;
    t.npad = (t.ntab + rsx::kRadix - 1) / rsx::kRadix * rsx::kRadix;
    t.nrow = t.npad / rsx::kRadix;
    t.ngroups = (t.nrow + rsx::kScanTiles - 1) / rsx::kScanTiles;
    const TileChunks c = tile_chunks(t.npad, cus);
    t.chunk = c.chunk;
    t.tgrid = c.grid;
    t.wgrid = (t.ntiles + t.chunk - 1) / t.chunk;
    return t;
}

// Workgroups of the kernels that walk the nseg + 1 offsets.
uint32_t offsets_grid(uint64_t nseg, uint64_t cus)
{
    return static_cast<uint32_t>(std::min<uint64_t>((nseg + 1 + rsx::kUniqSmallThreads - 1) / rsx::kUniqSmallThreads, cus * 4));
}

// The table and its group sums, large enough for `t` and for a segmented sort chain of `sort_tiles` tiles on the same buffers.
int grow_tile_table(rsx_engine* e, const TileTable& t, const char* what, uint64_t sort_tiles = 0)
{
    const uint64_t groups = std::max<uint64_t>((sort_tiles + rsx::kScanTiles - 1) / rsx::kScanTiles, t.ngroups);
    int rc = seg_grow(e, &e->seg_table, &e->seg_table_cap, std::max<uint64_t>(rsx::kRadix * sort_tiles, t.npad), what);
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_gsum, &e->seg_gsum_cap, rsx::kRadix * groups, "the group sums");
    if (rc == RSX_OK) rc = seg_grow(e, &e->seg_gsum2, &e->seg_gsum2_cap, rsx::kRadix * groups, "the scanned group sums");
    return rc;
}

// ---- shared launches --------------------------------------------------------------------------------------------------------

// Resets the first-bad-segment word and validates one or two offsets arrays into it; returns the word.
// (A launch, not hipMemsetAsync(bad, 0xFF, 4): with that memset a captured unique + reduce pair replayed as if its offsets were bad,
// every run offset 0, though the same calls were right when run eagerly; DESIGN.md, the chain of the segmented unique.)
uint32_t* begin_offset_check(rsx_engine* e, uint64_t cus, uint64_t nseg, const uint64_t* off_a, uint64_t n_a, const uint64_t* off_b = nullptr, uint64_t n_b = 0)
{
    uint32_t* bad = e->seg_temp + 1;
    hipLaunchKernelGGL(rsx::unique_reset_kernel, dim3(1), dim3(rsx::kWave), 0, e->stream, bad);
    if (off_a) {
        const uint32_t sgrid = offsets_grid(nseg, cus);
        hipLaunchKernelGGL(rsx::unique_validate_kernel, dim3(sgrid), dim3(rsx::kUniqSmallThreads), 0, e->stream, off_a, nseg, n_a, bad);
        if (off_b) hipLaunchKernelGGL(rsx::unique_validate_kernel, dim3(sgrid), dim3(rsx::kUniqSmallThreads), 0, e->stream, off_b, nseg, n_b, bad);
    }
    return bad;
}

// The exclusive scan of the segmented table in place: `rows` entries in each of its 16 rows, `groups` workgroups.
void launch_table_scan(rsx_engine* e, uint32_t rows, uint32_t groups)
{
    hipLaunchKernelGGL((rsx::scan_blocks_kernel<false, false>), dim3(groups), dim3(rsx::kScanTiles), 0, e->stream, e->seg_table, e->seg_gsum, rows, groups,
                       static_cast<uint32_t*>(nullptr));
    hipLaunchKernelGGL(rsx::paste_scan_kernel, dim3(groups), dim3(rsx::kScanTiles), 0, e->stream, e->seg_table, e->seg_gsum, e->seg_gsum2, e->seg_temp, rows,
                       groups);
}

// The shape of an LDS sort workgroup, as a type: f reads THREADS and KPT at compile time.
template <int T, int K>
struct SortShape {
    static constexpr int THREADS = T, KPT = K;
};

// f(class, grid, SortShape) for each of the three small-segment classes that can have a member: one workgroup per segment, grids bounded
// by what could exist and by residency.
template <typename F>
void for_each_small_class(uint64_t nseg, uint64_t n, uint64_t cus, F&& f)
{
    const uint64_t min_len[rsx::kSegClasses] = {2, rsx::kSegClass0Max + 1, rsx::kSegClass1Max + 1};
    const uint64_t per_cu[rsx::kSegClasses] = {32, 16, 4};
    for (int c = 0; c < rsx::kSegClasses; ++c) {
        const uint64_t grid = std::min<uint64_t>({nseg, n / min_len[c], cus * per_cu[c]});
        if (grid == 0) continue;
        if (c == 0) f(c, grid, SortShape<64, 4>{});
        else if (c == 1) f(c, grid, SortShape<64, 16>{});
        else f(c, grid, SortShape<256, 16>{});
    }
}

}  // namespace
}  // extern "C++"
