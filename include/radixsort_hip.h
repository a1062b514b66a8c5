/* radixsort_hip.h — C ABI of the MI355X (gfx950) LSD radix-sort engine.
 *
 * This is the drop-in boundary for the reference's GPU hot path: the private
 * steps of RadixSortGPU<T> (/root/reference/src/RadixSortGPU.h:95-109) and the
 * device-buffer set of ComputeDeviceData<T> (src/ComputeDeviceData.cpp:42-77),
 * re-expressed as plain C so that C++ (radix-sort_amd/host), ctypes, cgo or JNI
 * hosts bind the same symbols.  No C++ types, no exceptions and no ownership
 * transfer cross this boundary.  Every function returns an rsx_status whose
 * values map 1:1 onto the reference's `enum class OperationStatus`
 * (src/OperationStatus.h:4-17).
 *
 * One engine = one device + one HIP stream + one set of device buffers
 * (inputKeys/outputKeys ping-pong, optional uint32 payload ping-pong, digit
 * table, block sums).  Engines share nothing; an engine is not thread-safe
 * (same as the reference, which swaps buffer names in place,
 * src/RadixSortGPU.cpp:263-266).
 *
 * There is no CPU fallback behind these symbols: without a HIP device every
 * entry point that needs one fails with RSX_INITIALIZATION_FAILED.
 */
#ifndef RADIXSORT_HIP_H
#define RADIXSORT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* == OperationStatus (src/OperationStatus.h:4-17), same order, same values == */
typedef enum rsx_status {
    RSX_OK = 0,
    RSX_HOST_BUFFERS_FAILED = 1,
    RSX_INITIALIZATION_FAILED = 2,
    RSX_DATA_UPLOAD_FAILED = 3,
    RSX_CALCULATION_FAILED = 4,
    RSX_DATA_DOWNLOAD_FAILED = 5,
    RSX_CLEANUP_FAILED = 6,
    RSX_RESIZE_FAILED = 7,
    RSX_KERNEL_CREATION_FAILED = 8,   /* unreachable: kernels are AOT-compiled for gfx950 */
    RSX_PROGRAM_CREATION_FAILED = 9,  /* unreachable, kept for value parity */
    RSX_NO_SOURCE_FOUND = 10,         /* unreachable, kept for value parity */
    RSX_LOADING_SOURCE_FAILED = 11    /* unreachable, kept for value parity */
} rsx_status;

typedef struct rsx_engine rsx_engine;   /* opaque */

/* Digit geometry of the sort: 4-bit digits, 16 buckets, bits/4 passes
 * (src/Parameters.h:25,45,47). */
#define RSX_RADIX_BITS 4
#define RSX_RADIX 16

/* Key kinds of rsx_create.  Keys are ordered by the unsigned value of their ENCODING, B = key width in bits:
 *   RSX_KEY_UNSIGNED  enc(x) = x
 *   RSX_KEY_SIGNED    enc(x) = x ^ signbit                                (two's complement)
 *   RSX_KEY_FLOAT     enc(x) = x ^ ((x >>arith (B-1)) | signbit)          (IEEE-754 binary32 for key_bytes 4, binary64 for 8)
 * The float order is IEEE 754 totalOrder: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN.  The sorted keys are the input
 * bit patterns, unchanged (no NaN canonicalisation).  This equals numpy's stable sort on any input without -0.0 and without NaNs
 * whose sign bit is set; numpy and torch differ there: they treat -0.0 and +0.0 as equal (input order) and put every NaN last.
 * With RSX_OPT_DESCENDING the passes sort ~enc(x).  Float keys and descending order are coded on the fly (the first pass of a
 * sort encodes as it loads, the last one decodes as it stores; memory between the passes of a sort holds encoded keys, which is
 * what RSX_OPT_FIRST_PASS / LAST_PASS ranges, rsx_sort_from_to and the step API see: their passes are digits of the ENCODED key).
 * Engines of these kinds refuse rsx_partition*, rsx_key_range, rsx_sample_keys, rsx_msd_* and RSX_OPT_REF_DIAGNOSTICS. */
#define RSX_KEY_UNSIGNED 0
#define RSX_KEY_SIGNED 1
#define RSX_KEY_FLOAT 2

/* Options for rsx_set_option. */
typedef enum rsx_option {
    RSX_OPT_PROFILE = 0,      /* HIP events around launches -> RuntimesGPU: 0 off, 1 every launch, 2 reorder only */
    RSX_OPT_XCD_REMAP = 1,    /* 1 (default): consecutive tiles run on one XCD (L2 merges run seams) */
    RSX_OPT_FIRST_PASS = 2,   /* first pass of rsx_sort (default 0) */
    RSX_OPT_LAST_PASS = 3,    /* one past the last pass of rsx_sort (default bits/4) */
    RSX_OPT_REF_DIAGNOSTICS = 5, /* 1: rsx_download fills hist_out / globsum_out in the REFERENCE's geometry
                                 (16384-word [digit][group][item] table after paste, 512 scanned block sums,
                                 src/RadixSortGPU.cpp:412-428), recomputed from the last pass's input; needs a key
                                 count that is a multiple of 1024.  0 (default): the engine's own [digit][tile] table. */
    RSX_OPT_GRAPH = 6,        /* 1: rsx_sort / rsx_sort_from of at most 2^22 keys are captured once into a hipGraph and
                                 replayed; ignored while profiling and on the null stream.  Default 0: measured on
                                 MI355X the replay is no faster than eager launches (the ~3 us dependent-kernel
                                 boundary, not host launch cost, sets the 0.1 ms floor of a 33-kernel sort). */
    RSX_OPT_SMALL_SCAN = 7,   /* 1 (default): inside rsx_sort, tables of at most 1024 tiles (2^22 keys) are scanned and
                                 pasted by ONE workgroup in one launch instead of three; the step API is unaffected */
    RSX_OPT_TILE_SORT = 8,    /* 1 (default): inside rsx_sort, inputs of at most one tile (4096 keys) are sorted by ONE workgroup in
                                 ONE launch, every pass inside LDS; buffers, table and group sums end up as the pass chain
                                 leaves them.  Not taken while RSX_OPT_PROFILE is 1 (per-launch timings of the steps). */
    RSX_OPT_FUSED_SCAN = 9,   /* 1 (default): inside rsx_sort, tables of up to 512 scan groups (2^29 keys) are scanned and pasted in
                                 ONE launch whose workgroups hand their group sums to each other through tagged 8-byte
                                 granules; 0: scan #1, then scan #2 + paste (two launches).  Same table either way. */
    RSX_OPT_FUSED_SCAN_MAX_GROUPS = 15, /* largest table, in scan groups of 256 tiles (2^20 keys each), that takes the fused scan.  Its workgroups
                                 wait for each other inside the launch, so the whole grid must be resident at once: rsx_create asks
                                 hipOccupancyMaxActiveBlocksPerMultiprocessor x the CU count how many workgroups the device holds and takes
                                 HALF of it as the default (at most 512), which leaves room for a second engine scanning on another
                                 stream of the same device; engines that scan at the same time share that budget — a caller running k > 2
                                 of them concurrently on one device sets resident / k here.  Values are clamped to what is resident; -1 =
                                 default; 0 = never.  Larger tables take scan #1, then scan #2 + paste (two launches), same table. */
    RSX_OPT_RADIX_BITS = 10,  /* digit width of the rsx_sort chain: 4 (default, the reference's _NUM_BITS_PER_RADIX, src/Parameters.h:25) or 8.
                                 With 8 a pass sorts by a whole byte (two stable 4-bit rounds inside LDS, one scatter of up to
                                 256 runs per tile): half the passes over HBM.  Same result.  Pass ranges (RSX_OPT_FIRST_PASS /
                                 LAST_PASS, rsx_sort_from_to) stay in units of 4-bit passes: a range of whole bytes runs 8-bit passes, an odd
                                 range that starts on a byte boundary runs them for its whole bytes and one 4-bit pass for the last
                                 nibble, any other range runs the 4-bit chain; the step API and the diagnostic tables are those of
                                 4-bit passes. */
    RSX_OPT_SELF_SCAN = 11,   /* 1 (default): inside rsx_sort, tables of 2..1024 tiles (up to 2^22 keys) get no scan launch: every reorder
                                 workgroup derives the 16 first slots of its tile from the raw [tile][16] counts itself while
                                 its keys are on their way (passes + 1 dependent launches instead of 2 passes + 2) */
    RSX_OPT_SMALL_TILE_MAX_KEYS = 12, /* (default 2^19) self-scan sorts of at most this many keys (<= 2^20) run on tiles of 1024 keys (4 per thread) instead of
                                 4096: a shorter per-tile dependency chain for latency-bound small sorts.  The engine's own table
                                 read-back is not produced in that geometry (the reference-geometry diagnostics are). */
    RSX_OPT_SELF_SCAN_MAX_TILES = 14, /* (default 1024) largest table, in tiles (<= 1024), that takes the SELF_SCAN path */
    RSX_OPT_XCD_PHASE = 13,   /* (default -1) with XCD_REMAP: XCD x enters its tile range x * value tiles in and wraps round, so that the eight
                                 XCDs do not walk ranges that start n/8 apart in lockstep (same HBM channels); -1 = an eighth of a
                                 range, 0 = lockstep.  Placement only: results are identical. */
    RSX_OPT_LOOKAHEAD = 4,    /* 1 (default): inside rsx_sort the reorder of pass p also counts pass p+1's digits per
                                 output tile, so only the first pass runs the histogram kernel; 0: every pass runs
                                 histogram -> scan -> paste -> reorder separately.  Results are identical. */
    RSX_OPT_DESCENDING = 21   /* 1: sort in descending order from the next sort on (0, default: ascending), for every key kind.  Still
                                 STABLE: equal keys keep their input order (torch.sort(descending=True, stable=True)), which is not the
                                 reverse of the ascending result.  The passes sort ~enc(x) ascending (see the key kinds above). */
} rsx_option;

/* Per-phase launch timings in milliseconds, the RuntimesGPU fields
 * (src/RadixSortGPU.h:18-24) with Statistics semantics (src/Statistics.h). */
typedef struct rsx_phase_stat {
    double min_ms, max_ms, avg_ms, sum_ms;
    uint64_t n;
} rsx_phase_stat;

typedef struct rsx_runtimes {
    rsx_phase_stat histogram;  /* timeHisto   */
    rsx_phase_stat scan;       /* timeScan    (two launches per pass, as in the reference) */
    rsx_phase_stat paste;      /* timePaste   */
    rsx_phase_stat reorder;    /* timeReorder */
    rsx_phase_stat total;      /* whole rsx_sort calls (first launch -> last launch done) */
} rsx_runtimes;

typedef struct rsx_geometry {
    uint32_t tile_threads;     /* workgroup size of histogram/reorder (two scatter variants over 64-bit keys rank the same tile with 2x the threads and half the keys per thread) */
    uint32_t keys_per_thread;
    uint32_t tile_keys;        /* keys per tile = table column */
    uint32_t scan_block;       /* tiles per scan group: a group = this many consecutive tiles of ONE digit */
    uint64_t num_keys;         /* active length (rsx_resize / rsx_upload) */
    uint64_t capacity;
    uint64_t num_tiles;        /* ceil(num_keys / tile_keys) */
    uint64_t table_len;        /* RSX_RADIX * num_tiles, layout [digit][tile] */
    uint64_t num_scan_blocks;  /* 16 * ceil(num_tiles / scan_block) = live entries of globsum, layout [digit][group] */
    uint32_t num_passes;       /* key bits / 4 */
    uint32_t key_bytes;
    uint32_t fused_scan_resident;   /* workgroups of the fused table scan the device holds at once (occupancy query x CU count) */
    uint32_t fused_scan_max_groups; /* largest table, in scan groups, that takes the fused scan (RSX_OPT_FUSED_SCAN_MAX_GROUPS) */
} rsx_geometry;

/* ---- device --------------------------------------------------------------- */
/* Replaces ComputeState::init's device discovery (Common/ComputeState.cpp:14-104). */
int rsx_device_count(int* count);
int rsx_device_name(int device, char* buf, size_t buflen);
const char* rsx_last_error(void);   /* thread-local text of the last failure */
const char* rsx_version(void);

/* ---- lifetime ---------------------------------------------------------------
 * rsx_create replaces RadixSortGPU<T>::initialize (src/RadixSortGPU.cpp:452-543)
 * + ComputeDeviceData's constructor: allocates inputKeys/outputKeys
 * (capacity*key_bytes each), inputPermutations/outputPermutations
 * (capacity*4 each, only with has_payload), the digit table and block sums.
 * key_bytes is 4 or 8; key_kind is RSX_KEY_UNSIGNED, RSX_KEY_SIGNED (the OFFSET treatment of signed keys,
 * src/RadixSortGPU.cpp:436-440, RadixSort.cl:51,114) or RSX_KEY_FLOAT; any other value is refused with
 * RSX_INITIALIZATION_FAILED.  The engine creates its
 * own stream; rsx_set_stream substitutes a caller-owned hipStream_t.
 * rsx_destroy replaces release() (src/RadixSortGPU.cpp:445-449). */
int rsx_create(rsx_engine** out, int device, int key_bytes, int key_kind, int has_payload, uint64_t capacity);
int rsx_destroy(rsx_engine* e);
int rsx_set_stream(rsx_engine* e, void* hip_stream);
int rsx_get_stream(const rsx_engine* e, void** hip_stream);   /* the hipStream_t every call of this engine is enqueued on */
int rsx_set_option(rsx_engine* e, int option, int64_t value);
int rsx_get_geometry(const rsx_engine* e, rsx_geometry* out);

/* Sets the active number of keys (any value <= capacity; the reference's
 * 1024-rounding lives in the host class, RadixSortGPU::Resize,
 * src/RadixSortGPU.cpp:288-297). */
int rsx_resize(rsx_engine* e, uint64_t num_keys);

/* ---- transfers ------------------------------------------------------------
 * rsx_upload   = CopyDataToDevice + finish (src/RadixSortGPU.cpp:300-308,366-387):
 *                host keys -> inputKeys, host perm -> inputPermutations (payload
 *                engines only; perm may be NULL otherwise).  Sets num_keys = n.
 * rsx_fill_pad = padGPUData (:270-285): fills inputKeys from byte_offset to the
 *                end of the active length with the key that sorts next-to-last: dec(all-ones - 1)
 *                in the engine's encoding, i.e. numeric_limits<T>::max()-1 for integer keys in
 *                ascending order.
 * rsx_download = CopyDataFromDevice + finish (:349-357,390-429): sorted keys,
 *                payload (NULL to skip), the first hist_cap entries of the digit
 *                table and the first globsum_cap block sums of the last pass. */
int rsx_upload(rsx_engine* e, const void* host_keys, const uint32_t* host_perm, uint64_t n);
int rsx_fill_pad(rsx_engine* e, uint64_t byte_offset);
int rsx_download(rsx_engine* e, void* host_keys_out, uint32_t* host_perm_out,
                 uint32_t* hist_out, uint64_t hist_cap, uint32_t* globsum_out, uint64_t globsum_cap);

/* Pinned host memory for the transfers (the reference leaves a "consider CL_MEM_USE_HOST_PTR" note at
 * src/ComputeDeviceData.cpp:26; pageable memcpy is what its avgTotalGPU column pays for).  rsx_pin_host
 * page-locks a caller-owned range so that rsx_upload / rsx_download DMA straight from / to it;
 * rsx_unpin_host undoes it.  Both are optional; unpinned buffers keep working. */
int rsx_pin_host(rsx_engine* e, void* host_ptr, uint64_t bytes);
int rsx_unpin_host(rsx_engine* e, void* host_ptr);

/* End-to-end beyond one upload -> sort -> download at a time (the reference's avgTotalGPU column pays for all
 * three in sequence, src/CRadixSortTask.cpp:357-378; its visualizer sorts straight out of mapped host memory,
 * examples/visualize/visualize.cpp:801-854).
 * rsx_pipeline_submit: asynchronous.  Copies n keys (and permutation) from host memory into a device inbox on an
 *   upload stream, sorts them behind that copy on the engine's stream, and copies the result to host_keys_out on a
 *   download stream.  Two jobs are in flight at once (two inboxes, two outboxes, allocated on first use): the
 *   upload of job i+1 and the download of job i-1 run beside the sort of job i.  Host buffers must stay untouched
 *   until rsx_pipeline_wait and should be pinned (rsx_pin_host), otherwise the copies serialise on the host.
 * rsx_pipeline_wait: waits for every submitted job.
 * rsx_host_device_pointer: the device-side address of pinned (rsx_pin_host) host memory, for the zero-copy form:
 *   rsx_sort_from_to(e, <that address>, ...) reads the keys over PCIe in its first pass (and histogram) and
 *   writes its last pass straight into mapped host memory. */
int rsx_pipeline_submit(rsx_engine* e, const void* host_keys, const uint32_t* host_perm, uint64_t n, void* host_keys_out, uint32_t* host_perm_out);
int rsx_pipeline_wait(rsx_engine* e);
int rsx_host_device_pointer(rsx_engine* e, void* host_ptr, void** device_ptr);

/* ---- the hot path, step by step ---------------------------------------------
 * Asynchronous on the engine's stream; no host synchronisation inside.
 * rsx_histogram = RadixSortGPU::Histogram        (src/RadixSortGPU.cpp:16-61)
 * rsx_scan      = ScanHistogram, scans #1 and #2 (:64-152)
 * rsx_paste     = ScanHistogram, paste part      (:155-195)
 * rsx_reorder   = Reorder incl. the buffer swap  (:199-267)
 * rsx_sort      = calculate's pass loop          (:311-346) */
int rsx_histogram(rsx_engine* e, int pass);
int rsx_scan(rsx_engine* e);
int rsx_paste(rsx_engine* e);
int rsx_reorder(rsx_engine* e, int pass);
int rsx_sort(rsx_engine* e);
int rsx_sync(rsx_engine* e);   /* CommandQueue.finish() */
/* The fused table scan bounds its polls; a workgroup whose poll ran out (its grid was not resident at once — a device
 * shared with long-running kernels of other processes, see RSX_OPT_FUSED_SCAN_MAX_GROUPS) stores to a word of mapped host
 * memory and finishes, leaving that sort's result undefined.  The word is reported ONCE — by rsx_sync, rsx_download,
 * rsx_pipeline_wait (after their synchronisation), and by rsx_check_status / rsx_copy_result without synchronising, i.e. for
 * sorts that have already finished — with RSX_CALCULATION_FAILED / RSX_DATA_DOWNLOAD_FAILED, and is then cleared: the
 * engine stays usable.  Asynchronous callers (rsx_sort_from_to into their own buffers) end a batch with rsx_sync, or
 * call rsx_check_status after synchronising the stream themselves. */
int rsx_check_status(rsx_engine* e);

/* ---- device-resident callers (PyTorch / RCCL plumbing) ----------------------
 * rsx_sort_from: sorts n keys that already live in HBM at d_keys (16-byte
 *   aligned, not modified) with optional payload d_payload; the result stays in
 *   the engine (rsx_result_device / rsx_copy_result / rsx_download).
 * rsx_partition: ONE stable radix pass on the bit field [shift, shift+bits) of
 *   external keys into caller-provided output buffers; bucket_offsets receives
 *   (1<<bits)+1 exclusive offsets.  This is the bucket-grouping step of the
 *   multi-GPU exchange.  Synchronises the stream before returning.
 *   All partition entry points read keys and payload 16 bytes per lane: d_keys and d_payload must be 16-byte
 *   aligned (RSX_HOST_BUFFERS_FAILED otherwise); outputs need the alignment of their element type only,
 *   except where stated. */
/* Aliasing: d_keys may be the start of one of the engine's own two key buffers (the pointer
 * rsx_result_device returns; with a payload engine d_payload must then be the matching payload
 * buffer) — the sort then runs through the internal ping-pong, as rsx_sort does.  Any other overlap of
 * the input with the engine's buffers, of rsx_sort_from_to's output with them, or of input and output
 * with each other is refused with RSX_HOST_BUFFERS_FAILED.  After rsx_sort_from_to the result lives in
 * the caller's buffer only: rsx_download / rsx_copy_result of keys fail and rsx_result_device yields NULL
 * until the next sort or upload. */
int rsx_sort_from(rsx_engine* e, const void* d_keys, const uint32_t* d_payload, uint64_t n);
int rsx_partition(rsx_engine* e, const void* d_keys, const uint32_t* d_payload, uint64_t n,
                  int shift, int bits, void* d_keys_out, uint32_t* d_payload_out, uint64_t* bucket_offsets);
/* Range-adaptive partition for the multi-GPU exchange (keys whose top bits are all equal — small
 * ranges, sorted inputs — would otherwise land on one rank):
 * rsx_key_range: min and max of n device-resident keys in unsigned sort order (key ^ sign bit),
 *   returned as uint64; n == 0 gives lo = UINT64_MAX, hi = 0.  Synchronises.
 * rsx_partition_range: like rsx_partition with x = (key ^ sign) - lo and
 *   bucket = min(mul ? mulhi(x, mul) : x >> shift, 15), mul = floor(16 * 2^keybits / (hi - lo + 1)):
 *   16 equal-width buckets over [lo, hi] (mul == 0 for ranges of at most 16 values);
 *   bucket_offsets receives 17 entries. */
/* The same bit-field partition in two halves, so that the host can look at the bucket sizes (and
 * exchange them between ranks) BEFORE anything is moved: rsx_partition_count runs the histogram
 * and returns the (1<<bits) bucket sizes (synchronises); rsx_partition_scatter must follow on the
 * same keys / n / bit field and does scan + paste + reorder into the caller's buffers (asynchronous). */
int rsx_partition_count(rsx_engine* e, const void* d_keys, uint64_t n, int shift, int bits, uint64_t* bucket_counts);
int rsx_partition_scatter(rsx_engine* e, const void* d_keys, const uint32_t* d_payload, uint64_t n, int shift, int bits,
                          void* d_keys_out, uint32_t* d_payload_out);
/* Splitter partition (multi-GPU exchange on arbitrary distributions, heavy ties included):
 * rsx_sample_keys: `count` (<= 4096) keys, one per stratum of n/count consecutive keys, in unsigned
 *   sort order (key ^ sign bit) as uint64.  Synchronises.
 * rsx_partition_count_split: nsplit (1..7) strictly increasing splitters in that same order;
 *   bucket(x) = 2 * #{splitters < x} + [x equals a splitter]: even buckets are the open intervals, odd
 *   buckets hold exactly the keys equal to a splitter (which the caller may cut anywhere, in (rank,
 *   index) order).  Returns the 2*nsplit+1 bucket sizes.  Synchronises.
 * rsx_partition_scatter_split: must follow on the same keys; scan + paste + reorder by those buckets. */
int rsx_sample_keys(rsx_engine* e, const void* d_keys, uint64_t n, uint32_t count, uint64_t* samples);
int rsx_partition_count_split(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* splitters, int nsplit, uint64_t* bucket_counts);
int rsx_partition_scatter_split(rsx_engine* e, const void* d_keys, const uint32_t* d_payload, uint64_t n, void* d_keys_out, uint32_t* d_payload_out);
/* rsx_sort_from_to: rsx_sort_from over passes [first_pass, last_pass) (4-bit pass units, whatever the digit width of the chain) whose last pass
 * writes to the caller's d_keys_out / d_payload_out (any alignment), e.g. at an offset inside the final array — the local sort of one
 * wave of the sharded sort, whose keys share their top bits. */
int rsx_sort_from_to(rsx_engine* e, const void* d_keys, const uint32_t* d_payload, uint64_t n, int first_pass, int last_pass, void* d_keys_out,
                     uint32_t* d_payload_out);
/* rsx_segmented_sort: many independent segments of one array sorted in one call.  d_offsets is DEVICE memory with num_segments + 1
 *   uint64 entries (a torch int64 tensor of non-negative offsets as it is); segment s is [off[s], off[s+1]).  Every segment is sorted
 *   stably and written to the same index range of d_keys_out / d_payload_out; positions outside [off[0], off[S]) are not written.
 *   Empty segments and segments of one key are legal; boundaries may fall at any index.
 *   Key kind, RSX_OPT_DESCENDING and the payload follow the engine, as in rsx_sort_from_to (a payload engine needs both payload
 *   pointers, other engines ignore them).  The call always sorts every key bit with 4-bit digits: RSX_OPT_RADIX_BITS,
 *   RSX_OPT_FIRST_PASS / LAST_PASS and RSX_OPT_REF_DIAGNOSTICS do not apply to it.
 *   Buffers: n <= capacity; d_keys and d_payload 16-byte aligned, d_offsets 8-byte aligned, the outputs need only their element
 *   alignment.  Any overlap of inputs, outputs and the engine's own buffers is refused with RSX_HOST_BUFFERS_FAILED; afterwards
 *   rsx_download / rsx_copy_result of keys fail until the next sort, as after rsx_sort_from_to.
 *   Asynchronous on the engine's stream: no host synchronisation and no read-back of the offsets; every launch is sized from n
 *   and num_segments.  Segments of at most 4096 keys are sorted by one workgroup each inside LDS (classes of <= 256, <= 1024 and
 *   <= 4096 keys); larger ones share one LSD chain over their tiles.  Scratch space grows on first use of a larger n or
 *   num_segments — never inside a stream capture (such a call fails instead); hipGraph capture of this call is not supported.
 *   The offsets are validated on the device: a segment with off[s+1] < off[s] or off[s+1] > n is neither read nor written, and
 *   the next rsx_sync / rsx_check_status reports RSX_CALCULATION_FAILED once, rsx_last_error naming the first such segment; the
 *   other segments of such a call are sorted unless bad offsets make them overlap (their result is then undefined, but no access
 *   leaves d_keys[0, n), the outputs or d_offsets[0, S]).  The engine stays usable.
 *   n == 0 or num_segments == 0 returns RSX_OK and launches nothing; at most 2^32 - 2 segments and n <= 2^31 keys
 *   (RSX_CALCULATION_FAILED otherwise; n <= capacity gives RSX_RESIZE_FAILED first). */
int rsx_segmented_sort(rsx_engine* e, const void* d_keys, const uint32_t* d_payload, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments,
                       void* d_keys_out, uint32_t* d_payload_out);
/* rsx_segmented_topk: the k first keys of every segment's stable sort, by radix select.  Segment s = [off[s], off[s+1]) of length L
 *   gives m = min(k, L) keys to d_keys_out[s*k .. s*k+m) and their positions relative to off[s], as uint32, to d_index_out[s*k .. s*k+m):
 *   the first m entries of the stable sort of the segment in the engine's direction.  An ascending engine yields the k smallest keys,
 *   a descending one (RSX_OPT_DESCENDING) the k largest; equal keys are taken lowest index first, and the result is bitwise the same
 *   from run to run.  Float keys follow IEEE 754 totalOrder (+NaN above +inf, as torch.topk puts NaN); the only differences from
 *   torch.topk / torch.sort are -0.0 (below +0.0 here) and negative-sign NaNs (below -inf here).
 *   Slots [s*k+m, s*k+k), the slots of invalid segments and everything past num_segments*k are not written.
 *   1 <= k <= 4096 (one LDS tile): a larger k is refused with RSX_CALCULATION_FAILED (sort the segments instead and keep a prefix).
 *   k == 0, n == 0 or num_segments == 0 returns RSX_OK and launches nothing.
 *   Key kind and direction follow the engine; the payload flag does not apply (the index output takes its place).
 *   Buffers: n <= capacity (RSX_RESIZE_FAILED) and n <= 2^31; d_keys 16-byte aligned, d_offsets 8-byte aligned, the outputs need only
 *   their element alignment.  Any overlap of inputs, outputs and the engine's own buffers is refused with RSX_HOST_BUFFERS_FAILED;
 *   afterwards rsx_download / rsx_copy_result behave as after rsx_segmented_sort.
 *   As rsx_segmented_sort: d_offsets is DEVICE memory (num_segments + 1 uint64), the call is asynchronous on the engine's stream and
 *   never reads the offsets back, every launch is sized from n, num_segments and k.  Segments of at most 4096 keys are sorted in LDS
 *   by one workgroup each; larger ones take 8-bit select rounds over their tiles (4 for 32-bit keys, 8 for 64-bit), a compaction of
 *   k candidates per segment and an LDS sort of those.  A segment with off[s+1] < off[s] or off[s+1] > n is neither read nor written,
 *   and the next rsx_sync / rsx_check_status reports it once (RSX_CALCULATION_FAILED, rsx_last_error names it).  Scratch grows on
 *   first use of a larger n or num_segments, never inside a stream capture. */
int rsx_segmented_topk(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, uint32_t k, void* d_keys_out,
                       uint32_t* d_index_out);
/* rsx_segmented_select: the entries at given ranks of every segment's stable sort (k-th value, median, quantiles), by radix select.
 *   For segment s = [off[s], off[s+1]) of length L and every q < R (R = ranks_per_segment), with r = d_ranks[s*R + q]:
 *   r < L:  d_keys_out[s*R + q] is the key at position r of the stable sort of the segment in the engine's direction, bit pattern
 *           unchanged, and d_index_out[s*R + q] that element's position relative to off[s], as uint32: entry r of what
 *           rsx_segmented_sort with an iota payload gives for the segment.  Among equal keys this is the (r - #strictly better + 1)-th
 *           one in index order, for ascending and descending (RSX_OPT_DESCENDING) engines alike; the result is bitwise the same
 *           from run to run.
 *   r >= L: (0xFFFFFFFF is the conventional "none"; an empty segment has no valid rank) the slot is not written, so ragged segments
 *           can share one R.  The slots of invalid segments and everything past num_segments*R are not written either.
 *   The ranks of a segment may repeat and need not be ordered; they are not limited to 4096 as the top-k's k is.
 *   Float keys follow IEEE 754 totalOrder (+NaN above +inf, as torch.kthvalue / torch.median put NaN); the only differences from
 *   torch are -0.0 (below +0.0 here) and negative-sign NaNs (below -inf here).
 *   1 <= R <= 8 (8 histograms per wave fill the LDS budget of a select round): a larger R is refused with RSX_CALCULATION_FAILED
 *   (call again for further ranks, or sort the segments instead).  R == 0, n == 0 or num_segments == 0 returns RSX_OK and launches nothing.
 *   Key kind and direction follow the engine; the payload flag does not apply (the index output takes its place).
 *   Buffers: n <= capacity (RSX_RESIZE_FAILED) and n <= 2^31; d_keys 16-byte aligned, d_offsets 8-byte aligned, d_ranks 4-byte
 *   aligned, the outputs need only their element alignment.  Any overlap of inputs, outputs and the engine's own buffers is refused
 *   with RSX_HOST_BUFFERS_FAILED; afterwards rsx_download / rsx_copy_result behave as after rsx_segmented_sort.
 *   As rsx_segmented_topk: d_offsets (num_segments + 1 uint64) and d_ranks (num_segments * R uint32) are DEVICE memory, the call is
 *   asynchronous on the engine's stream and never reads them back, every launch is sized from n, num_segments and R.  Segments of at
 *   most 4096 keys are sorted in LDS by one workgroup each; larger ones take 8-bit select rounds over their tiles (4 for 32-bit keys,
 *   8 for 64-bit) in which ONE pass over the keys serves all R ranks, then a count of the ties of every rank's key per tile and a pass
 *   that locates the wanted tie: rounds + 2 readings of the keys whatever R is, and nothing the size of the input is written.
 *   A segment with off[s+1] < off[s] or off[s+1] > n is neither read nor written, and the next rsx_sync / rsx_check_status reports it
 *   once (RSX_CALCULATION_FAILED, rsx_last_error names it).  Scratch grows on first use of a larger n, num_segments or R, never inside
 *   a stream capture. */
int rsx_segmented_select(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, const uint32_t* d_ranks,
                         uint32_t ranks_per_segment, void* d_keys_out, uint32_t* d_index_out);
/* rsx_segmented_weighted_select: a select by MASS.  Where rsx_segmented_select finds the entry at a given rank of every segment's stable
 *   sort, this call finds the entry at which the running weight of that sorted order reaches a target: the top-p (nucleus) cut-off (the
 *   keys are their own weights, on a descending engine), weighted medians and quantiles, frequency-weighted order statistics.
 *   Mass: every weight is quantised once to a 32-bit fixed-point mass and every sum of masses is a 64-bit integer add, so no result
 *   depends on an order of additions.
 *     RSX_WEIGHT_UINT32   the mass is the stored word, any uint32; weight_exp must be 0.
 *     RSX_WEIGHT_FLOAT32 / RSX_WEIGHT_FLOAT64   mass(w) = 0 unless w > 0 (NaN, negatives and both zeros weigh nothing), else
 *                         min(floor(w * 2^(31 - weight_exp)), 2^31): no rounding enters (a binary float scaled by a power of two is exact),
 *                         a weight of 2^weight_exp or more weighs exactly 2^31, so one-hot probability rows are exact with weight_exp = 0.
 *                         |weight_exp| <= 2048.
 *     d_weights == NULL   the keys are the weights: the engine must have RSX_KEY_FLOAT keys and weight_kind must be the float kind of
 *                         the key width (anything else is refused with RSX_HOST_BUFFERS_FAILED).
 *   A mass is at most 2^32 - 1 and n <= 2^31, so every segment total stays below 2^63.
 *   Meaning: segment s = [off[s], off[s+1]) of length L; x_(0), x_(1), ... its stable sort in the engine's direction and order map (the
 *   order of rsx_segmented_sort and rsx_segmented_select, floats in totalOrder); C_r the sum of mass over x_(0..r); total = C_(L-1).  For
 *   every q < R (R = targets_per_segment) with target T, the answer is the smallest r with C_r >= T: that element always has positive
 *   mass, and among equal keys the running mass advances in index order.
 *     absolute form:  T = ((const uint64_t*)d_targets)[s*R + q].  T == 0 or T > total writes nothing to the slot.
 *     fraction form (RSX_WSELECT_FRACTION in flags): f = ((const double*)d_targets)[s*R + q]; T = clamp(ceil((double)total * f), 1, total),
 *                     one IEEE multiply of the round-to-nearest conversion of total, then ceil.  NaN or total == 0 writes nothing;
 *                     f <= 0 gives the first element with mass, f >= 1 the last one.
 *   Written per slot s*R + q: the key, bits unchanged (d_keys_out), its position relative to off[s] (d_index_out), r (d_rank_out, or NULL;
 *   r + 1 elements are kept) and C_r (d_mass_out, or NULL).  d_total_out[s] = total (or NULL) is written for every valid segment, empty
 *   ones included (0).  No other flag than RSX_WSELECT_FRACTION is accepted.
 *   1 <= R <= 4 (4 histograms of 64-bit masses and 32-bit counts per wave fill 48 KiB of LDS): a larger R is refused with
 *   RSX_CALCULATION_FAILED (call again for further targets).  R == 0, n == 0 or num_segments == 0 returns RSX_OK and launches nothing.
 *   Key kind and direction follow the engine; it works with any has_payload.
 *   Buffers: n <= capacity (RSX_RESIZE_FAILED), n <= 2^31, num_segments < 2^32 - 1; d_keys 16-byte aligned; d_weights, d_offsets,
 *   d_targets and the outputs need their element alignment (16-byte aligned weights are read in 16-byte loads).  Any overlap of inputs,
 *   outputs and the engine's own buffers is refused with RSX_HOST_BUFFERS_FAILED; afterwards rsx_download / rsx_copy_result behave as
 *   after rsx_segmented_sort.
 *   As rsx_segmented_select: offsets, weights and targets are DEVICE memory, the call is asynchronous on the engine's stream, reads
 *   nothing back and can be captured; every launch is sized from n, num_segments and R.  Segments of at most 4096 keys are sorted in
 *   LDS by one workgroup each and scanned there; larger ones take 8-bit select rounds over their tiles (4 for 32-bit keys, 8 for
 *   64-bit) in which ONE pass over keys and weights serves all R targets, then one pass for the tie masses per tile and a read of the one
 *   tile that holds each answer: (rounds + 1) readings of keys and weights, nothing the size of the input written.  No atomic decides
 *   an order or a destination: equal input gives equal bits on any engine, stream or capacity, eagerly or replayed from a graph.
 *   A segment with off[s+1] < off[s] or off[s+1] > n is neither read nor written, and the next rsx_sync / rsx_check_status reports it
 *   once under this call's name (RSX_CALCULATION_FAILED).  Scratch grows on first use of a larger n, num_segments or R, never inside a
 *   stream capture. */
#define RSX_WEIGHT_UINT32  0      /* the mass itself, any uint32 */
#define RSX_WEIGHT_FLOAT32 1
#define RSX_WEIGHT_FLOAT64 2
#define RSX_WSELECT_FRACTION 128  /* flags bit 7 (bits 0-6 are taken): d_targets holds doubles, fractions of each segment's total mass */
int rsx_segmented_weighted_select(rsx_engine* e, const void* d_keys, const void* d_weights /* or NULL: the keys are the weights */,
                                  uint64_t n, const uint64_t* d_offsets, uint64_t num_segments,
                                  const void* d_targets /* [S*R] uint64 masses, or doubles with RSX_WSELECT_FRACTION */, uint32_t targets_per_segment /* R, 1..4 */,
                                  uint32_t flags, uint32_t weight_kind, int32_t weight_exp,
                                  void* d_keys_out, uint32_t* d_index_out, uint32_t* d_rank_out /* or NULL */,
                                  uint64_t* d_mass_out /* or NULL */, uint64_t* d_total_out /* or NULL, [S] */);
/* rsx_segmented_unique: the distinct keys of every segment, with their counts, first positions and the inverse map (torch.unique with
 *   return_inverse / return_counts per segment; with RSX_UNIQUE_CONSECUTIVE torch.unique_consecutive / a run-length encoding).
 *   Segments are those of rsx_segmented_sort: d_offsets is DEVICE memory, num_segments + 1 uint64, segment s = [off[s], off[s+1]).
 *   d_offsets == NULL means ONE segment [0, n) (num_segments is then ignored): the sort is then the flat rsx_sort_from chain.
 *   Per segment, let d_0 < d_1 < ... < d_{m-1} be its distinct keys in the engine's direction and order map (ascending, or descending with
 *   RSX_OPT_DESCENDING; every key kind).  Two keys are equal iff their BIT PATTERNS are equal, which is equality under the order map: for
 *   float keys -0.0 and +0.0 are two values and NaNs with equal bits are one (torch.unique merges -0.0 with +0.0 and keeps every NaN
 *   apart).  With RSX_UNIQUE_CONSECUTIVE (flags bit 0) nothing is sorted: the "distinct keys" are the maximal runs of ADJACENT equal keys of
 *   the segment in input order.  Equal keys on the two sides of a segment boundary are two runs; empty segments have none.  Written:
 *     d_run_offsets_out  (required; num_segments + 1 uint64, 2 entries when d_offsets is NULL)  uoff[0] = 0, uoff[s+1] = uoff[s] + m_s; uoff[S] is
 *                        the total number of runs.  The per-run outputs are packed densely across the segments in this order.
 *     d_keys_out         (required; room for n keys)  d_keys_out[uoff[s] + u] = d_u of segment s, bit pattern unchanged.
 *     d_counts_out       (NULL to skip; n uint32)  occurrences of that key in the segment (the length of the run).
 *     d_first_out        (NULL to skip; n uint32)  position relative to off[s] of the key's FIRST occurrence (the lowest index; consecutive
 *                        mode: where the run starts).
 *     d_inverse_out      (NULL to skip; n uint32)  for every i in [off[0], off[S]): d_inverse_out[i] = u such that d_keys_out[uoff[s] + u] has
 *                        the bits of d_keys[i], s the segment of i.  Positions outside [off[0], off[S]) are not written.
 *   Entries past uoff[S] of the per-run outputs are not written.  The result is bitwise the same from run to run.
 *   Positions cost a payload: in sorted mode d_first_out / d_inverse_out need an engine created with has_payload = 1 (its permutation
 *   ping-pong carries the positions through the sort; the call generates them itself, the caller passes no payload) and are refused with
 *   RSX_HOST_BUFFERS_FAILED otherwise.  Calls without them work on every engine and carry no payload through the sort even on a payload
 *   engine.  Consecutive mode sorts nothing and serves every output on every engine.
 *   n == 0, or num_segments == 0 with non-NULL offsets, returns RSX_OK, launches nothing and writes NOTHING — d_run_offsets_out included
 *   (the caller knows that every entry would be 0).  Unknown flag bits are refused with RSX_CALCULATION_FAILED.
 *   Buffers: n <= capacity (RSX_RESIZE_FAILED) and n <= 2^31, at most 2^32 - 2 segments; d_keys 16-byte aligned, the offsets and run offsets
 *   8-byte aligned, the other outputs need only their element alignment.  Any overlap among inputs, outputs and the engine's own buffers is
 *   refused with RSX_HOST_BUFFERS_FAILED; afterwards rsx_download / rsx_copy_result behave as after rsx_segmented_sort.
 *   As rsx_segmented_sort: the call is asynchronous on the engine's stream and reads nothing back, every launch is sized from n and
 *   num_segments.  The sorted keys (and positions) stay in the engine's own buffers; one pass over them on the global grid of 4096-key tiles
 *   counts the first keys of runs per tile, the table scan of the sort family turns the counts into run ids, a second pass stores the
 *   runs and scatters the inverse map, and a pass over the runs takes the counts from the positions of neighbouring run starts.  Scratch
 *   grows on first use of a larger n or num_segments, never inside a stream capture.
 *   Bad offsets (off[s+1] < off[s] or off[s+1] > n): the packing of every later segment depends on every earlier one, so the contract is
 *   looser than rsx_segmented_select's.  The next rsx_sync / rsx_check_status reports RSX_CALCULATION_FAILED once, rsx_last_error naming
 *   the first such segment, exactly as for rsx_segmented_sort; no access leaves d_keys[0, n), d_offsets[0, S] or the stated sizes of the
 *   outputs; d_run_offsets_out is non-decreasing with uoff[S] <= n (this implementation writes zeros); the engine stays usable.  The
 *   contents of that call's other outputs are unspecified. */
#define RSX_UNIQUE_CONSECUTIVE 1   /* flags bit 0: do not sort; collapse runs of ADJACENT equal keys (run-length encode) */
int rsx_segmented_unique(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, uint32_t flags,
                         void* d_keys_out, uint64_t* d_run_offsets_out, uint32_t* d_counts_out, uint32_t* d_first_out, uint32_t* d_inverse_out);
/* rsx_segmented_reduce_by_key: per segment, the distinct keys and the SUM, MIN or MAX of the values that came with each of them (a sparse
 *   coalesce, torch.unique + index_add_ / scatter_reduce_ in one call, without the inverse map and without atomics).
 *   Grouping and layout are rsx_segmented_unique's, bit for bit: the runs are the distinct keys of segment s = [off[s], off[s+1]) in the
 *   engine's direction and order map, equality is equality of bit patterns, the runs are packed densely across the segments
 *   (d_keys_out[uoff[s] + u], d_run_offsets_out = uoff, num_segments + 1 uint64), d_counts_out is optional (NULL to skip), d_offsets == NULL
 *   means ONE segment [0, n) on the flat chain.  flags accepts RSX_UNIQUE_CONSECUTIVE and nothing else: with it nothing is sorted and the
 *   runs of ADJACENT equal keys in input order are reduced (a run-length reduce).
 *   d_values is indexed like d_keys: n entries of 4 (RSX_VALUE_INT32, _FLOAT32) or 8 bytes (RSX_VALUE_INT64, _FLOAT64), aligned to their
 *   size; only positions in [off[0], off[S]) are read.  d_values_out (required; room for n values) gets
 *   d_values_out[uoff[s] + u] = op over the values of that run's elements:
 *     RSX_REDUCE_SUM   integers wrap (two's complement).  Floats are added in a FIXED ASSOCIATION that is determined by the input alone —
 *                      keys, values, offsets and n — through the stable order of the run's elements and their places on the grid of
 *                      4096-element tiles.  It does not depend on the grid size, the engine's capacity, the stream or on what ran before:
 *                      two calls on equal input give equal bits.  That is a contract.  No atomic touches a value.
 *     RSX_REDUCE_MIN / _MAX   floats compare as numbers; the result is NaN if any value of the run is NaN (torch's amin / amax); which of
 *                      -0.0 and +0.0 wins a tie is unspecified.
 *   Sorted mode carries the positions of the values through the sort as its payload: it needs an engine created with has_payload = 1 (the
 *   call generates the positions itself) and is refused with RSX_HOST_BUFFERS_FAILED otherwise.  Consecutive mode works on every engine.
 *   Everything else as rsx_segmented_unique: asynchronous on the engine's stream, nothing read back, every launch sized from n and
 *   num_segments; n == 0 (or num_segments == 0 with offsets) writes nothing; n <= capacity and n <= 2^31; d_keys 16-byte aligned; any
 *   overlap among inputs, outputs and the engine's own buffers is refused; bad offsets are reported once by the next rsx_sync /
 *   rsx_check_status, the outputs of that call then being unspecified but inside their stated sizes; an unknown op, value kind or flag bit
 *   is refused with RSX_CALCULATION_FAILED.  Per tile one pass reduces the runs that begin and end inside it and leaves two partials (the
 *   part before its first run start, the part after its last); a second launch joins the partials of the runs that cross tiles. */
#define RSX_REDUCE_SUM 0
#define RSX_REDUCE_MIN 1
#define RSX_REDUCE_MAX 2
#define RSX_VALUE_INT32 0
#define RSX_VALUE_INT64 1
#define RSX_VALUE_FLOAT32 2
#define RSX_VALUE_FLOAT64 3
int rsx_segmented_reduce_by_key(rsx_engine* e, const void* d_keys, const void* d_values, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments,
                                uint32_t flags, uint32_t op, uint32_t value_kind, void* d_keys_out, uint64_t* d_run_offsets_out, void* d_values_out,
                                uint32_t* d_counts_out);
/* rsx_segmented_scan: the running SUM, MIN or MAX of the values inside every segment and, with keys, inside every run of adjacent equal
 *   keys (a scan by key; torch.cumsum / cummax-without-indices of ragged rows in one call).  Nothing is sorted.
 *   RESTARTS.  A position i in [off[0], off[S]) is a restart if it starts a non-empty segment, or — d_keys given — if key[i] and key[i-1]
 *   differ by bit pattern: the head rule of RSX_UNIQUE_CONSECUTIVE, so equal keys on the two sides of a segment boundary are two runs.
 *   d_offsets == NULL is the one segment [0, n); d_keys == NULL is a pure segmented scan; both NULL is the plain scan.  Keys are read with
 *   the engine's key width; key kind and direction do not matter.
 *   RESULTS.  With r(i) the last restart <= i: d_values_out[i] = v[r(i)] o ... o v[i]; with RSX_SCAN_EXCLUSIVE (flags bit 1; bit 0 stays
 *   RSX_UNIQUE_CONSECUTIVE's and is refused here, as every other bit is) it is v[r(i)] o ... o v[i-1], and the identity at a restart: 0 for
 *   SUM, the type's largest value (+inf) for MIN, its smallest (-inf) for MAX.  Positions outside [off[0], off[S]) are not written, and
 *   values there are not read.  Values and ops are rsx_segmented_reduce_by_key's: n entries of RSX_VALUE_INT32, _INT64, _FLOAT32 or
 *   _FLOAT64; integer sums wrap; for float MIN / MAX a NaN makes every later output of the same run NaN.
 *   FLOAT SUMS ARE BITWISE REPRODUCIBLE.  d_values_out[i] is a function of values, keys, offsets and n alone, through the element's place
 *   on the grid of 4096-element tiles and the places of the restarts (the association is written at the top of rsx_scan_by_key.hpp).  It
 *   does not depend on the grid size, on which workgroup takes a tile, on the engine's capacity, the stream, eager or captured execution,
 *   or on in-place operation; the exclusive result holds the inclusive result's bits one place further on.  That is a contract.  No
 *   atomic touches a value and no workgroup waits for another: three launches in stream order (tails per tile, the carries of all tiles,
 *   the tiles scanned), 2 reads and 1 write of the values, 2 reads of the keys.
 *   IN PLACE.  d_values_out == d_values exactly is served.  Every other overlap is refused with RSX_HOST_BUFFERS_FAILED: the output with
 *   the keys or the offsets, a partial overlap with the values, anything with the engine's own buffers.
 *   THE ENGINE'S SORT STATE IS UNTOUCHED.  The call uses none of the capacity-sized buffers (only per-tile scratch grows, outside stream
 *   captures), so n may exceed the capacity, and the result of an earlier sort, rsx_copy_result included, stays what it was.  n <= 2^31:
 *   tile indices and launch sizes are 32-bit words on the grid this family shares, and 2^31 is the bound its other calls are held to.
 *   Otherwise as the family: asynchronous on the engine's stream, nothing read back, every launch sized from n and num_segments; n == 0
 *   (or num_segments == 0 with offsets) launches and writes nothing; d_keys 16-byte aligned, values and output aligned to their element
 *   size, offsets to 8 bytes; an unknown flag bit, op or value kind is refused with RSX_CALCULATION_FAILED.  Offsets are validated on the
 *   device: with off[s+1] < off[s] or off[s+1] > n the call writes NOTHING and the next rsx_sync / rsx_check_status reports
 *   RSX_CALCULATION_FAILED once, naming the first such segment; the engine stays usable. */
#define RSX_SCAN_EXCLUSIVE 2   /* flags bit 1: out[i] folds the elements before i only; a restart holds the identity */
int rsx_segmented_scan(rsx_engine* e, const void* d_keys, const void* d_values, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments,
                       uint32_t flags, uint32_t op, uint32_t value_kind, void* d_values_out);
/* rsx_segmented_search: lower / upper bound of every query in the sorted segment of the same number (thrust's vectorised binary search;
 *   torch.searchsorted / bucketize, with ragged rows and in either direction).  Nothing is sorted and nothing is rewritten.
 *   SEGMENTS.  Haystack segment s is d_sorted[off[s] .. off[s+1]), L_s keys, sorted in the ENGINE's order: its key kind (floats: IEEE 754
 *   totalOrder) and direction (RSX_OPT_DESCENDING), i.e. what rsx_segmented_sort or rsx_sort_from of an engine of the same kind and
 *   direction leaves.  Query segment s is d_queries[qoff[s] .. qoff[s+1]) and is searched in haystack segment s.  Keys and queries have the
 *   engine's key type.
 *   RESULTS.  For query position j of segment s: d_index_out[j] = #{ i in segment s : key_i strictly before q_j in the engine's order };
 *   with RSX_SEARCH_RIGHT (flags bit 2) #{ i : key_i not after q_j }.  Both are relative to off[s]; on an ascending engine they are
 *   lower_bound and upper_bound.  Before and equal are those of the order map: equal means equal by bits, -0.0 is before +0.0, NaNs of
 *   the same bits are equal and a NaN is an ordinary largest or smallest key.  Positions outside [qoff[0], qoff[S]) are not written.
 *   OFFSET FORMS.  d_offsets == NULL: one haystack segment [0, n); d_query_offsets must be NULL too and the queries are [0, num_queries).
 *   d_offsets given, d_query_offsets == NULL: the even form, every segment has Q = num_queries / num_segments queries and query j belongs
 *   to segment j / Q (rows; a remainder is refused).  Both given: ragged queries, qoff has num_segments + 1 entries in device memory.
 *   A HAYSTACK THAT IS NOT SORTED gives unspecified results; each still lies in [0, L_s] and nothing outside the buffers is read.
 *   HOW.  Tiles of 1024 queries, one workgroup each (several tiles above 16 x CUs tiles).  A tile inside one segment of at most 4096 keys
 *   with at least one query per 16 keys stages the segment in LDS; one inside a longer segment (256 live queries or more) stages 1024
 *   evenly spaced keys, runs ten levels there and the rest in the window between two samples; every other tile bisects global memory
 *   (rsx_search.hpp).  Bytes: Q (key + 4), plus per tile L keys (staged), or 1024 sectors and the probed ones.
 *   THE ENGINE'S SORT STATE IS UNTOUCHED, as with rsx_segmented_scan: n may exceed the capacity and an earlier sort's result stays valid.
 *   Asynchronous on the engine's stream, nothing read back, every launch sized from n, num_segments and num_queries: capturable.  Offsets
 *   are validated on the device: with off[s+1] < off[s] or off[S] > n, or the same of qoff against num_queries, NOTHING is written and
 *   the next rsx_sync / rsx_check_status reports RSX_CALCULATION_FAILED once, naming the first such segment; the engine stays usable.
 *   REFUSED AT ONCE: RSX_CALCULATION_FAILED for a null engine, unknown flag bits, n or num_queries above 2^31, 2^32 - 1 segments or more,
 *   a num_queries that is no multiple of num_segments in the even form, d_query_offsets without d_offsets; RSX_HOST_BUFFERS_FAILED for a
 *   null d_sorted (n > 0), d_queries or d_index_out, a d_sorted that is not 16-byte aligned, queries, output or offsets not aligned to
 *   their element, the output overlapping an input, anything overlapping the engine's buffers.  num_queries == 0 (or num_segments == 0
 *   with offsets) launches nothing; n == 0 with queries is valid, every result is 0. */
#define RSX_SEARCH_RIGHT 4   /* flags bit 2 (disjoint from RSX_UNIQUE_CONSECUTIVE, bit 0, and RSX_SCAN_EXCLUSIVE, bit 1): upper bound */
int rsx_segmented_search(rsx_engine* e, const void* d_sorted, uint64_t n, const uint64_t* d_offsets, uint64_t num_segments, const void* d_queries,
                         uint64_t num_queries, const uint64_t* d_query_offsets, uint32_t flags, uint32_t* d_index_out);
/* rsx_segmented_compact: stream compaction of every segment by a byte mask or by one key bound per segment (thrust::copy_if, CUB's
 *   DeviceSelect::Flagged and DevicePartition; torch.masked_select, x[mask] and nonzero, with ragged rows and their new offsets).  Nothing is
 *   sorted.  (The name is compact: rsx_partition* is the digit partition of the sharded sort.)
 *   PREDICATE.  Exactly one of d_mask and d_bounds is given.  Mask form: element i is kept iff d_mask[i] != 0 (n bytes, any non-zero value,
 *   no alignment: torch.bool and uint8 as they are); the keys are opaque bits of the engine's key width.  Bound form: d_bounds holds one key
 *   of the engine's key type per segment; key k of segment s is kept iff it does not come after d_bounds[s] in the ENGINE's order (key
 *   kind, IEEE 754 totalOrder for floats, direction), with RSX_COMPACT_STRICT iff it comes strictly before: an ascending engine keeps
 *   k <= b, a descending float engine k >= b.  -0.0 comes before +0.0 and a NaN is an ordinary key.  RSX_COMPACT_INVERT keeps what the
 *   predicate rejects, in either form.
 *   COMPACT MODE (default).  With K(i) the number of kept elements in [off[0], i): a kept element i of segment s goes to d_keys_out[K(i)],
 *   bits unchanged, and its position relative to off[s] to d_index_out[K(i)].  d_kept_offsets_out[s] = K(off[s]) (num_segments + 1
 *   uint64): koff[0] = 0, koff[s+1] - koff[s] elements of segment s were kept, koff[S] is the total.  The packing is dense across the
 *   segments, as rsx_segmented_unique's; entries past koff[S] are not written.
 *   PARTITION MODE (RSX_COMPACT_PARTITION).  Nothing is dropped and the outputs cover the input's index range, as rsx_segmented_sort's:
 *   within [off[s], off[s+1]) the kept elements come first and the rejected ones behind them, both in input order (stable on both
 *   sides); d_index_out[off[s] + j] is the position, relative to off[s], that the element now at off[s] + j came from; koff is the
 *   same, the split point of segment s is off[s] + koff[s+1] - koff[s].  Positions outside [off[0], off[S]) are not written.
 *   BOTH MODES.  d_keys_out and d_index_out may each be NULL; with both NULL the call only counts.  d_kept_offsets_out is required.
 *   In mask form the keys are read only for d_keys_out: with d_keys_out == NULL d_keys is checked (non-null, 16-byte aligned) and not read.
 *   d_offsets == NULL is ONE segment [0, n).  The output is a function of the inputs alone: no atomic decides a destination.
 *   HOW.  The global grid of 4096-element tiles, reduce-then-scan: the kept elements per tile, the table scan of the sort family, the kept
 *   offsets, then a pass that recomputes the predicate, ranks the survivors of a tile, stages them in LDS at their rank and stores the
 *   staged copy to consecutive addresses (rsx_compact.hpp).  Bytes: the predicate's input twice (n mask bytes, or n keys), n keys once
 *   more in mask form, and what is kept.
 *   THE ENGINE'S SORT STATE IS UNTOUCHED, as with rsx_segmented_scan: n may exceed the capacity and an earlier sort's result stays valid;
 *   only per-tile scratch grows, outside stream captures.  Asynchronous on the engine's stream, nothing read back, every launch sized from
 *   n and num_segments: capturable.  n == 0 (or num_segments == 0 with offsets) launches and writes nothing.  Offsets are validated on
 *   the device: with off[s+1] < off[s] or off[s+1] > n every kernel leaves at once, d_kept_offsets_out is all zeros, d_keys_out and
 *   d_index_out are not written, and the next rsx_sync / rsx_check_status reports RSX_CALCULATION_FAILED once, naming the first such
 *   segment; the engine stays usable.
 *   REFUSED AT ONCE: RSX_CALCULATION_FAILED for a null engine, unknown flag bits, both or neither of d_mask and d_bounds,
 *   RSX_COMPACT_STRICT with a mask, n above 2^31, 2^32 - 1 segments or more; RSX_HOST_BUFFERS_FAILED for a d_keys that is null or not
 *   16-byte aligned, a null d_kept_offsets_out, outputs or bounds not aligned to their element, offsets or koff not 8-byte aligned, any
 *   overlap between an output and an input or another output (no operation is in place), anything overlapping the engine's buffers. */
#define RSX_COMPACT_PARTITION 8    /* flags bit 3: nothing is dropped; in every segment the kept elements come first, the others behind them, both in input order */
#define RSX_COMPACT_INVERT 16      /* flags bit 4: keep what the predicate rejects */
#define RSX_COMPACT_STRICT 32      /* flags bit 5, bound form only: keep keys strictly before the bound */
int rsx_segmented_compact(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets /* or NULL */, uint64_t num_segments,
                          const uint8_t* d_mask /* or NULL */, const void* d_bounds /* or NULL */, uint32_t flags,
                          void* d_keys_out /* or NULL */, uint32_t* d_index_out /* or NULL */, uint64_t* d_kept_offsets_out);
/* rsx_segmented_merge: the stable merge of sorted segment s of A with sorted segment s of B, for every s, in one pass over the keys
 *   (std::merge, thrust::merge / merge_by_key, cub::DeviceMerge, with ragged rows).  Nothing is sorted: every key is read once and
 *   written once.
 *   SEGMENTS.  Segment s of A is d_a[aoff[s] .. aoff[s+1]), La keys; segment s of B is d_b[boff[s] .. boff[s+1]), Lb keys; both are sorted
 *   in the ENGINE's order: its key kind (floats: IEEE 754 totalOrder) and direction (RSX_OPT_DESCENDING), i.e. what rsx_segmented_sort or
 *   rsx_sort_from of an engine of the same kind and direction leaves.  Both offsets arrays NULL: one segment [0, na) and [0, nb); one
 *   NULL and one given is refused.  Keys have the engine's key type; the payloads are one 32-bit word per key.
 *   RESULT.  ooff[s] = (aoff[s] - aoff[0]) + (boff[s] - boff[0]): the packing is dense from 0, as rsx_segmented_unique's and
 *   rsx_segmented_compact's, and ooff[S] is the total.  d_out_offsets, when non-NULL, gets these S + 1 uint64.  Output segment
 *   [ooff[s], ooff[s+1]) holds the STABLE SORT in the engine's order OF THE CONCATENATION A_s ++ B_s; for sorted inputs that is the stable
 *   merge: keys that are equal by bits keep the order within their side, and every A element comes before the B elements equal to it.  Key
 *   bits are unchanged; -0.0 sorts before +0.0 and a NaN is an ordinary key.  d_index_out[ooff[s] + r] = j is the position in that
 *   concatenation: j < La means A_s[j], otherwise B_s[j - La]: exactly what a stable argsort of the concatenation holds at r.
 *   d_payload_out gets the payload word that came with each key; the two payload inputs and d_payload_out are all given or all NULL.
 *   d_keys_out, d_index_out and d_out_offsets may each be NULL; with no output asked for at all the call is refused.  Nothing at or past
 *   ooff[S] is written.
 *   INPUTS THAT ARE NOT SORTED give an unspecified order; every access stays inside the buffers and exactly [0, ooff[S]) is written.
 *   HOW.  Tiles of 4096 OUTPUT positions.  One thread per tile boundary finds its segment and merge-path split (a bisection over the
 *   segments, one over the diagonal; A before equal B) and the output offsets are written; then a workgroup per tile (several tiles above
 *   16 x CUs tiles) stages the tile's sources - one contiguous range of A and one of B, 4096 keys together - in LDS, every thread merges 16
 *   consecutive outputs there, and the tile leaves as consecutive addresses (rsx_merge.hpp).  No atomics: the output is a function of the
 *   inputs alone.  Bytes: (na + nb) (2 key [+ 8 with payload] [+ 4 with index]) plus 8 per tile.
 *   THE ENGINE'S SORT STATE IS UNTOUCHED, whatever the engine's has_payload: na + nb may exceed the capacity and an earlier sort's result
 *   stays valid; only the per-tile splits grow, outside stream captures.  Asynchronous on the engine's stream, nothing read back, every
 *   launch sized from na, nb and num_segments: capturable.  Offsets are validated on the device, aoff against na and boff against nb:
 *   with off[s+1] < off[s] or off[s+1] > n in either, every kernel leaves at once, d_out_offsets is all zeros, nothing else is written,
 *   and the next rsx_sync / rsx_check_status reports RSX_CALCULATION_FAILED once, naming this call and the first such segment; the
 *   engine stays usable.
 *   REFUSED AT ONCE: RSX_CALCULATION_FAILED for a null engine, flags != 0 (no bit is defined; the argument exists because an ABI cannot
 *   grow one later), one offsets array without the other, na, nb or na + nb above 2^31, 2^32 - 1 segments or more, no output requested,
 *   payload pointers not all given or all NULL; RSX_HOST_BUFFERS_FAILED for a null d_a with na > 0 or a null d_b with nb > 0, a d_a or d_b
 *   that is not 16-byte aligned, payloads or outputs not aligned to their element, offsets not 8-byte aligned, any overlap of an output
 *   with an input or another output (there is no in-place form), anything overlapping the engine's buffers.  na + nb == 0 (or
 *   num_segments == 0 with offsets) launches and writes nothing; one empty side is valid: the result is a copy of the other side. */
int rsx_segmented_merge(rsx_engine* e, const void* d_a, const uint32_t* d_a_payload /* or NULL */, uint64_t na, const uint64_t* d_a_offsets /* or NULL */,
                        const void* d_b, const uint32_t* d_b_payload /* or NULL */, uint64_t nb, const uint64_t* d_b_offsets /* or NULL */,
                        uint64_t num_segments, uint32_t flags /* must be 0 */, void* d_keys_out /* or NULL */, uint32_t* d_payload_out /* or NULL */,
                        uint32_t* d_index_out /* or NULL */, uint64_t* d_out_offsets /* or NULL */);
/* rsx_segmented_set_op: intersection, difference, union or symmetric difference of sorted segment s of A with sorted segment s of B, for
 *   every s, in two passes over the keys (std::set_intersection / set_difference / set_union / set_symmetric_difference with duplicates,
 *   thrust::set_*_by_key, with ragged rows).  A set operation is the merge of rsx_segmented_merge whose outputs pass a predicate.
 *   SEGMENTS, ORDER AND EQUALITY as rsx_segmented_merge: segment s of A is d_a[aoff[s] .. aoff[s+1]), of B d_b[boff[s] .. boff[s+1]), both
 *   sorted in the ENGINE's order (key kind, IEEE 754 totalOrder for floats, direction); both offsets arrays NULL is the one segment
 *   [0, na) and [0, nb).  Keys are equal iff their bits are (-0.0 and +0.0 differ, NaNs with equal bits are one key).
 *   WHICH ELEMENTS ARE KEPT.  A key x occurs m times in A_s and n times in B_s; number its occurrences on each side r = 0, 1, ... in input
 *   order.  RSX_SET_INTERSECTION keeps the A occurrences r < n (min(m, n), all from A); RSX_SET_DIFFERENCE the A occurrences r >= n (the
 *   last max(m - n, 0) of A); RSX_SET_UNION every A occurrence and the B occurrences r >= m (max(m, n)); RSX_SET_SYMMETRIC_DIFFERENCE the
 *   A occurrences r >= n and the B occurrences r >= m (|m - n|): what std::set_* keeps.
 *   RESULT.  The kept elements of segment s appear in the order of the stable merge of A_s ++ B_s (A before equal B, each side in its own
 *   order), packed densely across segments: d_out_offsets[s] = koff[s] = the number kept before segment s, koff[0] = 0, koff[S] the
 *   total (S + 1 uint64; REQUIRED).  d_keys_out gets the keys (bits unchanged); d_payload_out the 32-bit word that came with each key (the
 *   two payload inputs and d_payload_out are all given or all NULL); d_index_out the position in A_s ++ B_s, the merge's convention
 *   (below La: A_s[j], otherwise B_s[j - La]); d_match_out (RSX_SET_INTERSECTION only) for the kept A occurrence r of x the position
 *   relative to boff[s] of B's occurrence r of x: index and match together are an inner join where no key repeats
 *   (min(m, n) pairs of a key's m x n otherwise: rsx_segmented_join is the relational join).  Each of these four may be NULL; with all
 *   NULL the call only counts.  Nothing at or past koff[S] is written in any output.  BUFFER SIZES: na elements for intersection and
 *   difference, na + nb for union and symmetric difference; the overlap checks use these sizes.
 *   INPUTS THAT ARE NOT SORTED give an unspecified result; every access stays inside the buffers, koff is non-decreasing, koff[S] is at
 *   most the buffer size above and exactly [0, koff[S]) is written (both passes evaluate the predicate with one function on the same
 *   data, and destinations are capped at the buffer size).
 *   HOW.  The merge's grid: tiles of 4096 merged positions, a workgroup per tile (several above 16 x CUs tiles), the merge's split per
 *   tile boundary.  A count pass stages the tile's A range and B range in LDS, merges, and asks per merged element with ONE probe of the
 *   other side whether it has a partner there (rsx_setop.hpp); the per-tile counts are scanned; a write pass repeats the merge and the
 *   predicate, ranks the kept elements and stores them as consecutive addresses.  No atomic decides a destination.  Bytes: 2 (na + nb)
 *   key reads [+ 4 (na + nb) with payload] + kept x (key [+ 4 payload] [+ 4 index] [+ 4 match]), plus 12 per tile.
 *   THE ENGINE'S SORT STATE IS UNTOUCHED, whatever the engine's has_payload: na + nb may exceed the capacity and an earlier sort's result
 *   stays valid; only the per-tile splits and the per-tile table grow, outside stream captures.  Asynchronous on the engine's stream,
 *   nothing read back, every launch sized from na, nb and num_segments: capturable.  Offsets are validated on the device as the merge's:
 *   with a bad segment in either array d_out_offsets is all zeros, nothing else is written, and the next rsx_sync / rsx_check_status
 *   reports RSX_CALCULATION_FAILED once, naming this call and the first such segment; the engine stays usable.
 *   REFUSED AT ONCE: RSX_CALCULATION_FAILED for a null engine, op > 3, flags != 0, a d_match_out with an op other than
 *   RSX_SET_INTERSECTION, one offsets array without the other, na, nb or na + nb above 2^31, 2^32 - 1 segments or more, payload pointers
 *   not all given or all NULL; RSX_HOST_BUFFERS_FAILED for a null d_out_offsets, a null d_a with na > 0 or a null d_b with nb > 0, a d_a
 *   or d_b that is not 16-byte aligned, payloads or outputs not aligned to their element, offsets not 8-byte aligned, any overlap of an
 *   output with an input or another output, anything overlapping the engine's buffers.  na + nb == 0 (or num_segments == 0 with offsets)
 *   launches and writes nothing.  With nb == 0 union, difference and symmetric difference give A back and intersection nothing but zero
 *   offsets. */
#define RSX_SET_INTERSECTION 0
#define RSX_SET_DIFFERENCE 1             /* A minus B */
#define RSX_SET_UNION 2
#define RSX_SET_SYMMETRIC_DIFFERENCE 3
int rsx_segmented_set_op(rsx_engine* e, const void* d_a, const uint32_t* d_a_payload /* or NULL */, uint64_t na, const uint64_t* d_a_offsets /* or NULL */,
                         const void* d_b, const uint32_t* d_b_payload /* or NULL */, uint64_t nb, const uint64_t* d_b_offsets /* or NULL */,
                         uint64_t num_segments, uint32_t op, uint32_t flags /* must be 0 */,
                         void* d_keys_out /* or NULL */, uint32_t* d_payload_out /* or NULL */, uint32_t* d_index_out /* or NULL */,
                         uint32_t* d_match_out /* or NULL; intersection only */, uint64_t* d_out_offsets);
/* rsx_segmented_histogram: the keys of every segment counted per bin (cub::DeviceHistogram; torch.bincount, torch.histc and
 *   torch.histogram, with ragged rows).  Segment s is d_keys[off[s] .. off[s+1]); d_offsets == NULL is the one segment [0, n).
 *   RESULT.  d_counts_out holds S x B uint32 counters, row-major: d_counts_out[s * B + b] = the keys of segment s that fall into bin b.  Every
 *   one of the S * B entries is written by every accepted call that launches, zeros included: the call zeroes them itself.  Keys that
 *   fall into no bin are dropped.  Nothing else is written.  Bins are numbered in the ENGINE's order, in both forms.
 *   EDGES FORM (d_edges != NULL): B + 1 keys of the engine's key kind in device memory, sorted in the engine's order (IEEE 754 totalOrder
 *   for floats, descending on a descending engine), shared by all segments; 1 <= B <= 4096.  With j the RSX_SEARCH_RIGHT position of key k
 *   in the edges (what rsx_segmented_search returns): bin j - 1 if 1 <= j <= B; bin B - 1 if j == B + 1 and k has the bits of edges[B]
 *   (the last bin is closed on both sides); dropped otherwise.  On an ascending engine that is numpy.histogram(x, bins=edges).  Keys are
 *   equal iff their bits are: -0.0 and +0.0 are different edges and a NaN is an ordinary key.  Edges that are not sorted give unspecified
 *   counts; every key is still counted at most once and no access leaves the buffers.  lo_bits, hi_bits and width_shift must be 0.
 *   EVEN FORM, INTEGER KEY KINDS (d_edges == NULL): lo = the key whose bits are the low key_bytes of lo_bits.  Key k goes to bin
 *   (k - lo) >> width_shift if k does not come before lo in ascending value order and that bin is < B (the arithmetic runs on the
 *   order-mapped unsigned words: right for signed keys).  width_shift = 0, lo = 0 is torch.bincount(x, minlength=B)[:B].
 *   width_shift < 8 * key_bytes; hi_bits must be 0.  On a descending engine bin b becomes B - 1 - b.
 *   EVEN FORM, FLOAT KEY KINDS: lo and hi from lo_bits and hi_bits, both finite, lo < hi; width_shift must be 0.  With scale =
 *   Key(B) / (hi - lo) computed once on the host in the key's own precision (refused unless finite and positive), key x goes to bin
 *   min(B - 1, floor((x - lo) * scale)) if lo <= x && x <= hi by IEEE comparison: -0.0 counts as 0.0; NaN and out-of-range keys are
 *   dropped, as torch.histc drops them.  The subtraction and the multiplication are each rounded once.  Results with a subnormal x - lo
 *   are unspecified.  On a descending engine bin b becomes B - 1 - b.
 *   HOW.  One kernel zeroes the counters; one kernel walks tiles of 4096 keys.  Up to 4096 bins a workgroup counts in LDS (a copy per wave
 *   up to 1024 bins), keeps counting from tile to tile while the segment stays the same, and adds its non-zero counters to the result
 *   when the segment changes and at its end.  More bins, and the pieces of segments shorter than 256 keys, add to the result directly.
 *   Counts are integers: the result does not depend on the order of the additions.  Bytes: n keys read, 8 per counter.
 *   THE ENGINE'S SORT STATE IS UNTOUCHED, whatever the engine's has_payload: n may exceed the capacity and an earlier sort's result stays
 *   valid; no scratch grows.  Asynchronous on the engine's stream, nothing read back, capturable once the engine's status words exist (any
 *   earlier call of the segmented family).  Offsets are validated on the device: with a bad segment (off[s+1] < off[s] or off[s+1] > n)
 *   all S * B counters are zero and the next rsx_sync / rsx_check_status reports RSX_CALCULATION_FAILED once, naming this call and the
 *   first such segment; the engine stays usable.
 *   REFUSED AT ONCE: RSX_CALCULATION_FAILED for a null engine, flags != 0, num_bins == 0, more than 4096 bins in the edges form, the
 *   parameter combinations ruled out above, 2^32 - 1 segments or more, n > 2^31, num_segments * num_bins > 2^31;
 *   RSX_HOST_BUFFERS_FAILED for a null d_keys with n > 0 or one that is not 16-byte aligned, edges not aligned to the key size, a null
 *   d_counts_out or one not 4-byte aligned, offsets not 8-byte aligned, the counters overlapping an input, anything overlapping the
 *   engine's buffers.  n == 0 with a valid shape STILL ZEROES the counters (rsx_segmented_compact launches nothing then; here an all-zero
 *   histogram is the right answer).  d_offsets != NULL with num_segments == 0 returns RSX_OK and writes nothing. */
int rsx_segmented_histogram(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets /* or NULL */, uint64_t num_segments,
                            const void* d_edges /* or NULL */, uint64_t lo_bits, uint64_t hi_bits, uint32_t width_shift, uint64_t num_bins,
                            uint32_t flags /* must be 0 */, uint32_t* d_counts_out);
/* rsx_segmented_weighted_histogram: the MASSES of the keys of every segment summed per bin, bitwise reproducibly (torch.bincount(x,
 *   weights=w), torch.histogram(x, bins, weight=w), numpy.histogram(weights=), the gate mass per expert of a router, with ragged rows).
 *   RESULT.  d_sums_out holds S x B 64-bit sums, row-major: d_sums_out[s * B + b] = the sum of the masses of the keys of segment s that fall
 *   into bin b.  THE BIN OF A KEY is exactly rsx_segmented_histogram's, in all three forms (edges, even integer, even float), with the
 *   same parameters (d_edges, lo_bits, hi_bits, width_shift, num_bins), the engine's direction, totalOrder, the closed last bin and the
 *   dropped keys: read them above.  d_weights holds n weights of weight_kind, element i beside key i; it is required (keys as their own
 *   weights are not offered here).
 *   MASS, flags == 0.  Exactly rsx_segmented_weighted_select's: RSX_WEIGHT_UINT32: the stored word, any uint32, weight_exp must be 0;
 *   RSX_WEIGHT_FLOAT32 / _FLOAT64: mass(w) = 0 unless w > 0 (NaN, negatives and both zeros weigh nothing), else min(floor(w *
 *   2^(31 - weight_exp)), 2^31), |weight_exp| <= 2048.  The sums are uint64.  The row sum of a histogram whose bins cover every key equals
 *   that call's d_total_out[s] bit for bit.
 *   MASS, RSX_WHIST_SIGNED in flags (float kinds only).  The mass is that of |w| — the sign bit cleared, then the rule above — and it is
 *   added NEGATED for a negative weight: NaN of either sign and both zeros weigh nothing, -inf weighs -2^31.  The sums are then
 *   two's-complement int64.
 *   REPRODUCIBLE.  A weight is quantised once to an integer mass and every sum is a 64-bit integer add modulo 2^64: the adds commute, so
 *   the result does not depend on their order, the grid, the stream, or eager or captured execution.  n <= 2^31 and a mass of at most
 *   2^32 - 1 keep every sum below 2^63 in magnitude.
 *   HOW.  One kernel zeroes the sums; one kernel walks tiles of 4096 keys with the thread's 16 weights loaded beside its keys (16-byte
 *   loads where d_weights is 16-byte aligned).  Up to 2048 bins a workgroup sums in LDS (64-bit counters, a copy per wave up to 512
 *   bins), keeps summing from tile to tile while the segment stays the same, and adds its non-zero sums to the result when the segment
 *   changes and at its end.  More bins (the edges form takes up to 4096, its edges staged in LDS), and the pieces of segments shorter than
 *   256 keys, add to the result directly.  A key whose mass is 0 adds nothing.  Bytes: n keys and n weights read, 16 per sum.
 *   EVERYTHING ELSE is rsx_segmented_histogram's contract: d_offsets == NULL is the one segment [0, n); every one of the S * B sums is
 *   written by every accepted call that launches, zeros included; n == 0 with a valid shape still zeroes; d_offsets != NULL with
 *   num_segments == 0 returns RSX_OK and writes nothing.  THE ENGINE'S SORT STATE IS UNTOUCHED, whatever the engine's has_payload: n may
 *   exceed the capacity and an earlier sort's result stays valid; no scratch grows.  Asynchronous on the engine's stream, nothing read
 *   back, capturable once the engine's status words exist.  Offsets are validated on the device: with a bad segment all S * B sums are zero
 *   and the next rsx_sync / rsx_check_status reports RSX_CALCULATION_FAILED once, naming this call and the first such segment; the
 *   engine stays usable.
 *   REFUSED AT ONCE: RSX_CALCULATION_FAILED for a null engine, flag bits other than RSX_WHIST_SIGNED, RSX_WHIST_SIGNED with
 *   RSX_WEIGHT_UINT32, a weight_kind above RSX_WEIGHT_FLOAT64, weight_exp != 0 with RSX_WEIGHT_UINT32 or beyond +-2048, num_bins == 0,
 *   more than 4096 bins in the edges form, the parameter combinations rsx_segmented_histogram rules out, 2^32 - 1 segments or more,
 *   n > 2^31, num_segments * num_bins > 2^30; RSX_HOST_BUFFERS_FAILED for a null d_keys with n > 0 or one that is not 16-byte aligned, a
 *   null d_weights or one not aligned to its element, edges not aligned to the key size, a null d_sums_out or one not 8-byte aligned,
 *   offsets not 8-byte aligned, the sums overlapping an input, anything overlapping the engine's buffers. */
#define RSX_WHIST_SIGNED 256      /* flags bit 8 (bits 0-7 are taken): float weights carry their sign, the sums are int64 */
int rsx_segmented_weighted_histogram(rsx_engine* e, const void* d_keys, const void* d_weights, uint64_t n, const uint64_t* d_offsets /* or NULL */,
                                     uint64_t num_segments, const void* d_edges /* or NULL */, uint64_t lo_bits, uint64_t hi_bits, uint32_t width_shift,
                                     uint64_t num_bins, uint32_t flags, uint32_t weight_kind, int32_t weight_exp, uint64_t* d_sums_out);
/* rsx_segmented_sample: R categorical draws from every segment, an element drawn with probability proportional to its weight, bitwise
 *   reproducibly (torch.multinomial with replacement; top-k / top-p / min-p sampling with a bound; ragged rows).  The caller supplies the
 *   uniforms: there is no random number generator in here.  Nothing is sorted: segment s = [off[s], off[s+1]) has the elements
 *   i = 0 .. L-1 in INPUT order.
 *   MASS.  m_i is exactly rsx_segmented_weighted_select's mass of element i's weight: RSX_WEIGHT_UINT32: the stored word, weight_exp must
 *   be 0; RSX_WEIGHT_FLOAT32 / _FLOAT64: 0 unless w > 0 (NaN, negatives and both zeros weigh nothing), else min(floor(w * 2^(31 -
 *   weight_exp)), 2^31), |weight_exp| <= 2048.  d_weights == NULL: the keys are their own weights (RSX_KEY_FLOAT engines, weight_kind the
 *   float kind of the key width).
 *   BOUND.  With d_bounds (one key per segment) an element the predicate rejects weighs 0.  The predicate is exactly
 *   rsx_segmented_compact's bound form: key k of segment s is kept iff it does not come after d_bounds[s] in the engine's order (key
 *   kind, totalOrder, direction), with RSX_COMPACT_STRICT iff it comes strictly before; RSX_COMPACT_INVERT flips it.  Every tie of the
 *   bound is kept (or, strict, dropped) alike.
 *   DRAW.  P_i = m_0 + ... + m_i and total = P_(L-1) are 64-bit integer sums.  For every draw q < R with target T the answer is the
 *   smallest i with P_i >= T: element i answers exactly the targets in (P_(i-1), P_i], so it always has positive mass.
 *     absolute form: T = ((const uint64_t*)d_targets)[s*R + q]; T == 0 or T > total writes nothing.
 *     fraction form (RSX_WSELECT_FRACTION): u = ((const double*)d_targets)[s*R + q], T = clamp(ceil((double)total * u), 1, total),
 *     rsx_segmented_weighted_select's rule unchanged; NaN or total == 0 writes nothing.  For u uniform on [0, 1) element i is drawn with
 *     probability m_i / total up to the granularity of the doubles.
 *   WRITTEN.  d_index_out[s*R + q] = i, relative to off[s]; d_mass_out[s*R + q] (or NULL) = P_i; d_total_out[s] (or NULL) = total for
 *   every segment, empty ones included (0).  A slot without an answer is not written.
 *   REPRODUCIBLE.  No atomic and no float add decides a result: equal input gives equal bits on every engine, stream, capacity and
 *   graph replay.
 *   HOW.  One pass over the 4096-element tiles sums, per tile, the mass of what crosses a tile edge (a tile that holds whole segments
 *   only is not read); then one wave per (segment, draw) forms the total, the target, walks the segment's tiles 256 at a time to the one
 *   whose piece holds the crossing, and reads that one piece again.  A segment inside one tile is read by its draws alone.  Bytes: the
 *   weights (and the keys, with a bound or as weights) once, 16 per tile written, one tile's piece per draw.
 *   POINTERS AND LIMITS.  Everything is device memory.  d_keys is read only with d_bounds or with d_weights == NULL; otherwise it may be
 *   NULL.  d_offsets == NULL is the one segment [0, n).  R >= 1, num_segments * R <= 2^31, n <= 2^31, fewer than 2^32 - 1 segments.
 *   R == 0, n == 0, or no segments with offsets given return RSX_OK and launch nothing.  Keys, when read: 16-byte aligned; weights,
 *   bounds, targets and outputs: their element size (16-byte aligned weights are read in 16-byte loads).  THE ENGINE'S SORT STATE IS
 *   UNTOUCHED, whatever the engine's has_payload: n may exceed the capacity and an earlier sort's result stays valid; only the per-tile
 *   scratch grows (never inside a capture: run one call of the size first).  Asynchronous on the engine's stream, nothing read back,
 *   capturable.  Offsets are validated on the device: with off[s+1] < off[s] or off[s+1] > n nothing is written and the next rsx_sync /
 *   rsx_check_status reports RSX_CALCULATION_FAILED once, naming this call and the first such segment; the engine stays usable.
 *   REFUSED AT ONCE: RSX_CALCULATION_FAILED for a null engine, flag bits other than RSX_WSELECT_FRACTION, RSX_COMPACT_STRICT and
 *   RSX_COMPACT_INVERT, the last two without d_bounds, a weight_kind above RSX_WEIGHT_FLOAT64, weight_exp != 0 with RSX_WEIGHT_UINT32 or
 *   beyond +-2048, 2^32 - 1 segments or more, n > 2^31, num_segments * R > 2^31; RSX_HOST_BUFFERS_FAILED for d_weights == NULL on an
 *   engine whose keys are not floats of weight_kind's width, keys that are read and null or not 16-byte aligned, weights, bounds,
 *   targets, outputs or offsets not aligned to their element, a null d_targets or d_index_out, an output overlapping an input or another
 *   output, anything overlapping the engine's buffers. */
int rsx_segmented_sample(rsx_engine* e, const void* d_keys /* or NULL */, const void* d_weights /* or NULL: the keys are the weights */, uint64_t n,
                         const uint64_t* d_offsets /* or NULL */, uint64_t num_segments, const void* d_bounds /* or NULL: one key per segment */,
                         const void* d_targets /* [S*R] uint64 masses, or doubles with RSX_WSELECT_FRACTION */, uint32_t draws_per_segment /* R */,
                         uint32_t flags, uint32_t weight_kind, int32_t weight_exp, uint32_t* d_index_out, uint64_t* d_mass_out /* or NULL */,
                         uint64_t* d_total_out /* or NULL */);
/* rsx_segmented_rank: the rank of every key inside its segment, under one of five tie rules, and the size of its tie group
 *   (scipy.stats.rankdata; pandas / cuDF groupby().rank(method=); argsort(argsort(x)) with ties settled).
 *   RESULT.  For every i in [off[s], off[s+1]): d_rank_out[i] is the 0-based rank of d_keys[i] inside segment s in the ENGINE'S ORDER: its
 *   ascending / descending setting and key codec over all six key kinds, floats in IEEE 754 totalOrder (-0.0 before +0.0, NaNs ordered
 *   by sign and payload), equality by bit pattern, exactly as rsx_segmented_unique groups.  d_ties_out[i] (or NULL: skipped) is the
 *   number of keys of segment s with d_keys[i]'s bits.  With run = the keys equal to d_keys[i], before = the keys strictly before them:
 *     RSX_RANK_ORDINAL  the position in the segment's stable sort (ties in index order): rsx_segmented_sort's iota payload, inverted
 *     RSX_RANK_MIN      |before|                       RSX_RANK_MAX      |before| + |run| - 1
 *     RSX_RANK_DENSE    the DISTINCT keys in before     RSX_RANK_AVERAGE  MIN + MAX: twice the average rank, an exact integer
 *   Equal keys on the two sides of a segment boundary are two groups.  Positions outside [off[0], off[S]) are not written; empty
 *   segments write nothing.  d_offsets == NULL is the one segment [0, n).
 *   REPRODUCIBLE.  No atomic and no float operation decides a result: equal input gives equal bits on every engine, stream, capacity
 *   and graph replay.
 *   HOW.  Segments of 2..4096 keys: one workgroup each sorts (encoded key, position) inside LDS in the segmented sort's three class
 *   shapes, flags the heads of the runs, scans them three ways (run start, run end, distinct before) and stores the ranks in index order:
 *   n*K bytes read, n*4 (n*8 with ties) written, nothing else.  Larger segments, and the flat form, are grouped by the segmented chain
 *   (the flat product chain) with generated positions as payload into the engine's buffers; then heads per 4096-key tile, the three
 *   carries per segment over its tiles, and one scattered 4-byte store per key and output.
 *   POINTERS AND LIMITS.  Everything is device memory.  THE ENGINE MUST HAVE has_payload = 1 AND n <= capacity: the positions travel
 *   through the sort of large segments; the engine's buffers and result are overwritten (as after rsx_sort_from_to with outputs).
 *   n <= 2^31, so MIN + MAX fits 32 bits; fewer than 2^32 - 1 segments.  n == 0, or no segments with offsets given, return RSX_OK and
 *   launch nothing.  Keys 16-byte aligned, outputs 4-byte, offsets 8-byte.  Scratch grows on demand, never inside a capture (run one call
 *   of the shape first).  Asynchronous on the engine's stream, nothing read back, capturable, every launch sized from n and num_segments
 *   alone.  Offsets are validated on the device: with off[s+1] < off[s] or off[s+1] > n nothing is written and the next rsx_sync /
 *   rsx_check_status reports RSX_CALCULATION_FAILED once, naming this call and the first such segment; the engine stays usable.
 *   REFUSED AT ONCE: RSX_CALCULATION_FAILED for a null engine, flags != 0, method > RSX_RANK_AVERAGE, 2^32 - 1 segments or more,
 *   n > 2^31; RSX_HOST_BUFFERS_FAILED for an engine without payload, n above the capacity, keys null or not 16-byte aligned, a null or
 *   misaligned d_rank_out, a misaligned d_ties_out or d_offsets, an output overlapping an input or the other output, anything
 *   overlapping the engine's buffers. */
#define RSX_RANK_ORDINAL 0   /* position in the segment's stable sort: ties in index order */
#define RSX_RANK_MIN     1   /* number of keys strictly before it ("competition" rank) */
#define RSX_RANK_MAX     2   /* min + (size of its tie group) - 1 */
#define RSX_RANK_DENSE   3   /* number of DISTINCT keys strictly before it */
#define RSX_RANK_AVERAGE 4   /* min + max: TWICE the average rank, so it stays an exact integer */
int rsx_segmented_rank(rsx_engine* e, const void* d_keys, uint64_t n, const uint64_t* d_offsets /* or NULL: one segment [0, n) */,
                       uint64_t num_segments, uint32_t flags /* must be 0 */, uint32_t method, uint32_t* d_rank_out, uint32_t* d_ties_out /* or NULL */);
/* rsx_segmented_reduce: SUM, MIN, MAX, ARGMIN or ARGMAX of the values of every segment (cub::DeviceSegmentedReduce; torch.segment_reduce;
 *   x.sum(-1), amax, argmax over the rows of a batch).  Nothing is sorted and there are no keys: the engine's key kind does not matter.
 *   RESULT.  d_values_out[s] = op over v[off[s] .. off[s+1]) for EVERY s < S: dense by segment id, not packed.  d_offsets == NULL is the
 *   one segment [0, n), and num_segments must be 1 then.  Values are n entries of RSX_VALUE_INT32, _INT64, _FLOAT32 or _FLOAT64, aligned
 *   to their size; only positions in [off[0], off[S]) are read.  Integer sums wrap (two's complement); float MIN / MAX give NaN if the
 *   segment holds one, as rsx_segmented_reduce_by_key does.
 *   EMPTY SEGMENTS get the op's identity: 0 for SUM, the type's largest value (+inf for floats) for MIN and ARGMIN, its smallest (-inf)
 *   for MAX and ARGMAX; their index is 0xFFFFFFFF.
 *   ARGMIN / ARGMAX.  d_index_out[s] is the position, relative to off[s], of the FIRST element that attains the extreme.  A NaN beats
 *   every number and among NaNs the first wins (torch.argmax); -0.0 and +0.0 tie and the first wins.  d_values_out, if given, gets the
 *   value at that position with its bits unchanged.  d_index_out is required for the two arg ops and must be NULL for SUM, MIN and MAX.
 *   WHAT IS WRITTEN.  Every accepted call with valid offsets writes all S results (and all S indices), also with n == 0 and with
 *   off[0] == off[S], as rsx_segmented_histogram writes all its counters.  num_segments == 0 (with offsets) launches and writes nothing.
 *   FLOAT SUMS ARE BITWISE REPRODUCIBLE.  d_values_out[s] is a function of values, offsets and n alone, through the elements' places on
 *   the grid of 4096-element tiles and the places of the segment boundaries (the association is written at the top of rsx_segreduce.hpp:
 *   a thread folds its 16 elements left to right, a flagged Hillis-Steele scan joins the 64 lanes of a wave, the four wave totals are
 *   folded left to right — the levels of rsx_segmented_scan, the same code, so a segment inside one tile gets the bits the inclusive
 *   scan stores at its last element — and a fixed join runs across the tiles of a longer segment).  It does not depend on the grid size,
 *   the tiles per workgroup, the engine's capacity, the stream, or eager or captured execution.  That is a contract.  No atomic touches a
 *   value and no workgroup waits for another: two launches in stream order after the offsets' check (one fold per tile, then the empty
 *   segments and the segments that cross tile edges), one read of the values.
 *   THE ENGINE'S SORT STATE IS UNTOUCHED, as with rsx_segmented_scan: the call uses none of the capacity-sized buffers (only per-tile
 *   scratch grows, outside stream captures), so n may exceed the capacity and an earlier sort's result stays valid.  n <= 2^31, fewer
 *   than 2^32 - 1 segments.  Asynchronous on the engine's stream, nothing read back, every launch sized from n and num_segments,
 *   capturable once a call of this size has run.  Offsets are validated on the device: with a bad segment (off[s+1] < off[s] or
 *   off[s+1] > n) NOTHING is written and the next rsx_sync / rsx_check_status reports RSX_CALCULATION_FAILED once, naming this call and
 *   the first such segment; the engine stays usable.
 *   REFUSED AT ONCE: RSX_CALCULATION_FAILED for a null engine, flags != 0, an unknown op or value kind, d_offsets == NULL with
 *   num_segments != 1, 2^32 - 1 segments or more, n > 2^31; RSX_HOST_BUFFERS_FAILED for a null d_values with n > 0 or one not aligned
 *   to the value size, a null d_values_out for SUM / MIN / MAX or a misaligned one, a null or misaligned d_index_out for the arg ops or
 *   a given one for the others, offsets not 8-byte aligned, an output overlapping an input or the other output, anything overlapping
 *   the engine's buffers. */
#define RSX_REDUCE_ARGMIN 3
#define RSX_REDUCE_ARGMAX 4   /* RSX_REDUCE_SUM / _MIN / _MAX keep 0 / 1 / 2; the two arg ops are rsx_segmented_reduce's only */
int rsx_segmented_reduce(rsx_engine* e, const void* d_values, uint64_t n, const uint64_t* d_offsets /* or NULL */, uint64_t num_segments,
                         uint32_t flags /* must be 0 */, uint32_t op, uint32_t value_kind, void* d_values_out /* or NULL for the arg ops */,
                         uint32_t* d_index_out /* arg ops only */);
/* rsx_segmented_expand: from offsets back to elements (moderngpu's load-balancing search / interval expand; the decode that
 *   cub::DeviceRunLengthEncode lacks; torch.repeat_interleave with a ranged-gather form).  Nothing is sorted and there are no keys: any
 *   engine serves, whatever its key kind or has_payload.
 *   RESULT.  Let s(i) be the LARGEST s with off[s] <= i, the merge's rule: of several segments that share an offset the last one owns
 *   the position, so an empty segment owns nothing.  For every i in [off[0], off[S]):
 *     d_segment_out[i] = s(i)
 *     d_rank_out[i]    = i - off[s(i)]
 *     d_values_out[i]  = d_values[s(i)]                             fill form (flags == 0): num_values must equal num_segments
 *     d_values_out[i]  = d_values[starts[s(i)] + i - off[s(i)]]     gather form (RSX_EXPAND_GATHER): segment s is a copy of
 *                                                                   d_values[starts[s] .. starts[s] + len_s); ranges may overlap, descend
 *                                                                   and be odd
 *   Values are opaque bits of value_bytes = 4 or 8 bytes.  n is the element count of every output buffer given; positions outside
 *   [off[0], off[S]) are NOT written.  At least one output must be non-NULL; d_values and d_values_out are both NULL or both given;
 *   d_starts (num_segments entries) must be given if and only if RSX_EXPAND_GATHER is set.  num_segments == 0 or n == 0 launches nothing.
 *   ALIGNMENT.  Every pointer is aligned to its element and no further: the kernel stores 16 bytes at a time over the part of each
 *   4096-position tile that is 16-byte aligned in the output at hand and single elements at the ragged ends, per output.
 *   BAD INPUT is a pair with off[s+1] < off[s] or off[s+1] > n and, in gather form, a segment with starts[s] + len_s > num_values
 *   (empty segments included).  Then NOTHING is written and the next rsx_sync / rsx_check_status reports RSX_CALCULATION_FAILED once,
 *   naming this call and the first such segment; the engine stays usable.
 *   THE OUTPUT IS A FUNCTION OF THE INPUTS ALONE: no atomic touches it and no workgroup waits for another, so equal input gives equal
 *   bits eagerly, captured, and on any stream or engine.  Launches in stream order: the checks, one bisection per tile boundary of the
 *   ABSOLUTE grid of 4096 output positions, one pass over the tiles (a tile with no segment start in it is a pure fill; otherwise the
 *   starts are marked in LDS and a max-scan spreads them; rsx_expand.hpp).  A tile that holds more offsets than slots (dense empty
 *   segments) walks them 1024 at a time: slow, correct.
 *   THE ENGINE'S SORT STATE IS UNTOUCHED: the call uses none of the capacity-sized buffers (tiles + 1 words of scratch grow, outside
 *   stream captures), so n may exceed the capacity and an earlier sort's result stays valid.  n <= 2^31, fewer than 2^32 - 1 segments.
 *   Asynchronous on the engine's stream, nothing read back, every launch sized from n and num_segments, capturable once a call of this
 *   size has run.
 *   REFUSED AT ONCE: RSX_CALCULATION_FAILED for a null engine, flag bits other than RSX_EXPAND_GATHER, value_bytes not 4 or 8, d_starts
 *   without the flag or the flag without d_starts, one of d_values / d_values_out without the other, no output at all, the fill form
 *   with num_values != num_segments, 2^32 - 1 segments or more, n > 2^31; RSX_HOST_BUFFERS_FAILED for null offsets, a pointer not
 *   aligned to its element, an output overlapping an input or another output, anything overlapping the engine's buffers. */
#define RSX_EXPAND_GATHER 64       /* flags bit 6 (bits 0-5 are taken): ranged gather instead of fill */
int rsx_segmented_expand(rsx_engine* e, const void* d_values /* or NULL */, uint64_t num_values, uint32_t value_bytes /* 4 or 8 */,
                         const uint64_t* d_offsets, uint64_t num_segments, uint64_t n, const uint64_t* d_starts /* gather form only, else NULL */,
                         uint32_t flags, void* d_values_out /* or NULL */, uint32_t* d_segment_out /* or NULL */, uint32_t* d_rank_out /* or NULL */);
/* rsx_segmented_join: the relational equi-join of sorted segment s of A, d_a[aoff[s] .. aoff[s+1]), with sorted segment s of B,
 *   d_b[boff[s] .. boff[s+1]), for every s (moderngpu's relational join on the load-balancing search; the foreign-key lookup, edge x edge,
 *   sparse x sparse).  Both sorted in the engine's order (key kind, direction, IEEE 754 totalOrder for floats).  Both offsets arrays NULL:
 *   ONE segment; one without the other is refused.  Keys are equal iff their bits are: -0.0 and +0.0 do not join, NaNs of equal bits do.
 *   Unlike RSX_SET_INTERSECTION, whose index and match outputs pair only min(m, n) of a key's m x n occurrences, every A row meets every
 *   partner.
 *   ROWS.  For A element i of segment s (i relative to aoff[s]) let lb_i and ub_i be the lower and the upper bound of its key in B_s and
 *   c_i = ub_i - lb_i.  RSX_JOIN_INNER emits the c_i rows (i, lb_i + r), r < c_i.  RSX_JOIN_LEFT the same and, where c_i == 0, the one row
 *   (i, 0xFFFFFFFF).  RSX_JOIN_SEMI the one row (i, lb_i) iff c_i > 0.  RSX_JOIN_ANTI the one row (i, -) iff c_i == 0 (d_b_index_out is
 *   refused).  Rows are ordered by segment, then i, then B position, and packed from 0: row p writes d_a_index_out[p] = i,
 *   d_b_index_out[p] = the B position relative to boff[s], d_keys_out[p] = the A key, bits unchanged.  d_out_offsets[s] (uint64, S + 1
 *   entries, required) = rows before segment s; d_out_offsets[S] = P, the total.
 *   64-BIT COUNTS AND TRUNCATION.  P can reach La x Lb per segment; all counting is 64-bit and d_out_offsets holds the true counts
 *   whatever out_capacity is.  out_capacity is the element count of each of the three row buffers: exactly the rows p < min(P,
 *   out_capacity) are written and nothing at or past that position is touched.  With the three row outputs NULL the call only counts
 *   (out_capacity is ignored): read d_out_offsets[S], allocate, call again; or size the buffers from a bound you know (P == na for a
 *   foreign-key join, P <= na for SEMI and ANTI).  Truncation is no error: it shows as d_out_offsets[S] > out_capacity.
 *   BAD INPUT is a pair with off[s+1] < off[s] or off[s+1] > n in either offsets array (n = na, nb).  Then d_out_offsets holds zeros,
 *   NOTHING else is written, and the next rsx_sync / rsx_check_status reports RSX_CALCULATION_FAILED once, naming this call and the first
 *   such segment; the engine stays usable.  Segments that are NOT SORTED give unspecified rows, but no access leaves the buffers, the
 *   offsets are non-decreasing, exactly [0, min(P, out_capacity)) is written, every A index is < La and every B index < Lb or 0xFFFFFFFF
 *   (ub is searched inside [lb, Lb]).  na == 0: zero offsets, no rows.  nb == 0: INNER and SEMI have no rows, LEFT and ANTI every A row.
 *   num_segments == 0 (with offsets) launches nothing and writes nothing.
 *   THE OUTPUT IS A FUNCTION OF THE INPUTS ALONE: no atomic decides a destination or touches an output and no workgroup waits for another,
 *   so equal input gives equal bits eagerly, captured, and on any stream or engine.  Launches in stream order: the checks, one pass over
 *   tiles of 4096 A positions (per element the two bounds in B_s, the row count, a 64-bit prefix inside the tile), a 64-bit scan of the
 *   tile totals, the offsets; then, unless the call only counts, one bisection per boundary of the grid of 4096 output rows and one pass
 *   over those tiles (rsx_join.hpp).  An output tile that spans a long run of A elements without a row (sparse matches) walks it: slow,
 *   correct.
 *   THE ENGINE'S SORT STATE IS UNTOUCHED: any engine whatever its has_payload; none of the capacity-sized buffers (scratch of 12 to 16
 *   bytes per A position grows, outside stream captures), so na, nb and P may exceed the capacity and an earlier sort's result stays
 *   valid.  Asynchronous on the engine's stream, nothing read back, every launch sized from na, nb, num_segments and out_capacity,
 *   capturable once a call of this size has run.
 *   REFUSED AT ONCE: RSX_CALCULATION_FAILED for a null engine, op > 3, flags != 0, one offsets array without the other, na or nb above
 *   2^31, 2^32 - 1 segments or more, out_capacity above 2^34 with a row output (the output tile grid is 32-bit), d_b_index_out with
 *   RSX_JOIN_ANTI; RSX_HOST_BUFFERS_FAILED for a missing d_out_offsets, null or misaligned pointers (d_a and d_b 16-byte aligned,
 *   everything else aligned to its element), an output overlapping an input or another output, anything overlapping the engine's
 *   buffers. */
#define RSX_JOIN_INNER 0
#define RSX_JOIN_LEFT  1
#define RSX_JOIN_SEMI  2
#define RSX_JOIN_ANTI  3
int rsx_segmented_join(rsx_engine* e, const void* d_a, uint64_t na, const uint64_t* d_a_offsets /* or NULL */,
                       const void* d_b, uint64_t nb, const uint64_t* d_b_offsets /* or NULL */, uint64_t num_segments,
                       uint32_t op, uint32_t flags /* must be 0 */, uint64_t out_capacity,
                       void* d_keys_out /* or NULL */, uint32_t* d_a_index_out /* or NULL */, uint32_t* d_b_index_out /* or NULL */,
                       uint64_t* d_out_offsets /* required, S + 1 */);
/* Receive buffers other ranks can write to (the peer-store exchange below): rsx_peer_alloc (hipMalloc + an IPC handle to hand to the other
 * PROCESSES, which map it with rsx_peer_open / rsx_peer_close — peer access over xGMI); ranks that are threads of one process use the
 * pointer itself (after rsx_peer_enable, once per other device). */
#define RSX_IPC_HANDLE_BYTES 64
int rsx_peer_alloc(rsx_engine* e, uint64_t bytes, void** d_ptr, void* ipc_handle /* RSX_IPC_HANDLE_BYTES bytes, or NULL */);
int rsx_peer_free(rsx_engine* e, void* d_ptr);
int rsx_peer_open(rsx_engine* e, const void* ipc_handle, void** d_ptr);
int rsx_peer_close(rsx_engine* e, void* d_ptr);
int rsx_peer_enable(rsx_engine* e, int peer_device);
/* ---- exchange step of the sharded sort on the top B <= 8 key bits (nothing in the reference: one device, one in-order
 * queue, Common/ComputeState.cpp:88-101).  world = 1, 2, 4, 8 or 16 ranks own k = 2^bits / world consecutive buckets of the top `bits`
 * bits each; bucket rank * k + w belongs to WAVE w, and every rank receives its k waves one after the other, so that wave w can be sorted —
 * all its keys at a rank share the top `bits` bits: passes [0, ceil((keybits - bits) / 4)) suffice — while wave w + 1 is still on the links.
 * More bits = more, smaller waves = a smaller exposed first wave.  All calls are asynchronous on the engine's stream unless stated.
 *   rsx_msd_count    one read of the shard: d_counts (DEVICE memory, 256 x uint64) receives the keys per bucket in natural bucket order
 *                    (entries past 2^bits are 0) — the row the caller all_gathers; no host synchronisation.
 *   rsx_msd_scatter  must follow on the same keys: groups the shard (stable) into d_staging in wave-major order [wave][destination rank]
 *                    (inside a segment: by the remaining bits of the key's top byte).  Needs only THIS rank's counts, i.e. it may run while
 *                    the all_gather is still in flight.
 *   rsx_msd_plan     from the gathered table d_table[source rank * stride + bucket] (+ every rank's receive and output capacity in keys at
 *                    [.. + cap_at] and [.. + cap_at + 1]) computes ON THE DEVICE, on hip_stream (NULL = the engine's): where each of this
 *                    rank's (wave, destination) segments lands in the destination's receive buffer (sources in rank order; grouping 0: every
 *                    wave starts 16-byte aligned and is sorted by itself; grouping 1, "doubling groups": only waves 0, 1, 2, 4, 8, ... do, the
 *                    waves of a group {0} {1} {2,3} {4..7} ... lie gap-free and are sorted together — radix-sort_amd/host/ShardPlanner.h), what this rank receives per wave, every rank's load, and the capacity verdict — then copies the host's part to
 *                    pinned memory.  rsx_msd_plan_wait blocks the HOST until that copy has landed (the device never waits for the host) and
 *                    returns it: wave_start / wave_count (2^bits / world entries, in keys, THIS rank's receive buffer), loads (world entries),
 *                    verdict (0 = go; bit r = rank r's buffers are too small; bit 32 + r = rank r's status word, [.. + cap_at + 2] of its row, was
 *                    non-zero: its engine reported an error of an earlier step — non-zero on one rank is non-zero on all, and no push writes anything).
 *   rsx_msd_push     wave `wave`: copies this rank's segments of that wave from staging straight into the destinations' receive buffers:
 *                    d_peer_keys / d_peer_payload = DEVICE arrays of `world` base addresses as THIS rank addresses them (rsx_peer_alloc /
 *                    rsx_peer_open / rsx_peer_enable).  `parts` workgroups per destination (<= 0: max(16, 128 / world)): a link-bound copy that leaves the CUs to
 *                    the local sorts.  hip_stream (NULL = the engine's): the stream the copy is enqueued on — a second stream lets wave w + 1
 *                    travel while wave w is sorted on the engine's; the call makes it wait for the plan and for rsx_msd_scatter itself.
 *                    The caller fences the wave across ranks (one tiny all_reduce, or its own flags) before sorting it.
 * Plumbing for hosts that do not link HIP themselves: rsx_copy_to_device / _from_device / _on_device (asynchronous on the engine's
 * stream; pageable host memory serialises, pin it with rsx_pin_host), rsx_wait_for (e's stream waits for everything enqueued on
 * other's stream so far — engines of one process, any devices) and rsx_record_mark / rsx_wait_mark (below). */
int rsx_msd_count(rsx_engine* e, const void* d_keys, uint64_t n, int bits, int world, uint64_t* d_counts);
int rsx_msd_scatter(rsx_engine* e, const void* d_keys, const uint32_t* d_payload, uint64_t n, void* d_staging, uint32_t* d_staging_payload);
int rsx_msd_plan(rsx_engine* e, const uint64_t* d_table, uint32_t stride, uint32_t cap_at, int rank, int grouping, void* hip_stream);
int rsx_msd_plan_wait(rsx_engine* e, uint64_t* wave_start, uint64_t* wave_count, uint64_t* loads, uint64_t* verdict);
int rsx_msd_push(rsx_engine* e, int wave, const void* d_staging, const uint32_t* d_staging_payload, const uint64_t* d_peer_keys, const uint64_t* d_peer_payload, int parts,
                 void* hip_stream);
int rsx_copy_to_device(rsx_engine* e, void* d_dst, const void* host_src, uint64_t bytes);
int rsx_copy_from_device(rsx_engine* e, void* host_dst, const void* d_src, uint64_t bytes);
int rsx_copy_on_device(rsx_engine* e, void* d_dst, const void* d_src, uint64_t bytes);
int rsx_wait_for(rsx_engine* e, rsx_engine* other);
/* Named points of an engine's stream: rsx_record_mark(e, slot) marks "everything enqueued on e's stream so far" (slot 0..RSX_MAX_MARKS-1, re-recordable);
 * rsx_wait_mark(e, other, slot) makes e's stream wait for other's mark — at any later time, whatever has been enqueued on other's stream since
 * (rsx_wait_for = record + wait in one call).  Used by the C++ sharded driver: one mark per wave on the communication stream. */
#define RSX_MAX_MARKS 256
int rsx_record_mark(rsx_engine* e, int slot);
int rsx_wait_mark(rsx_engine* e, rsx_engine* other, int slot);
int rsx_key_range(rsx_engine* e, const void* d_keys, uint64_t n, uint64_t* lo, uint64_t* hi);
int rsx_partition_range(rsx_engine* e, const void* d_keys, const uint32_t* d_payload, uint64_t n, uint64_t lo, int shift, uint64_t mul,
                        void* d_keys_out, uint32_t* d_payload_out, uint64_t* bucket_offsets);
int rsx_result_device(rsx_engine* e, void** d_keys, uint32_t** d_payload);
int rsx_copy_result(rsx_engine* e, void* d_keys_out, uint32_t* d_payload_out);

/* Launch geometry of the tile kernels, as host arithmetic (no device is touched): workgroup b of a launch over
 * num_keys keys in tiles of tile_keys keys works on tile tiles_out[b] (values >= *ntiles mark workgroups that
 * exit at once); *blocks = workgroups launched.  xcd_remap / xcd_phase as RSX_OPT_XCD_REMAP / RSX_OPT_XCD_PHASE.
 * At most cap entries are written.  For tests of the mapping: every tile must appear exactly once. */
int rsx_tile_map(uint64_t num_keys, uint32_t tile_keys, int xcd_remap, int64_t xcd_phase, uint32_t* tiles_out, uint64_t cap,
                 uint32_t* blocks, uint32_t* ntiles);

/* ---- measurements ------------------------------------------------------------
 * rsx_timings synchronises, folds pending HIP-event pairs into the statistics and
 * copies them out (getRuntimes, src/RadixSortGPU.cpp:591-595); reset != 0 clears
 * them afterwards. */
int rsx_timings(rsx_engine* e, rsx_runtimes* out, int reset);

#ifdef __cplusplus
}
#endif
#endif /* RADIXSORT_HIP_H */
