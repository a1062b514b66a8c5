"""radix-sort_amd — MI355X-native LSD radix sort behind the reference's RadixSortGPU API.

This module is the Python-side binding of the C ABI in include/radixsort_hip.h
(ctypes over radix-sort_amd/libradixsort_hip.so).  It carries no sort logic: every
method is one C-ABI call.  The C++20 host mirror of the reference interface
(RadixSortGPU<T>, CRadixSortTask<T>, Dataset<T>, ...) lives in radix-sort_amd/host/.

There is no CPU fallback: if the HIP library is missing, or no GPU is present when an
engine is created, this raises.

The directory name contains a hyphen, so load it with `importlib` (see
__graft_entry__.load_package()) under the module name `radix_sort_amd`.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import sys

import numpy as np

from . import _tensor_args as _args

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RSX_LIB") or os.path.join(_HERE, "libradixsort_hip.so")   # RSX_LIB: A/B builds while tuning

# OperationStatus (reference src/OperationStatus.h:4-17)
STATUS_NAMES = [
    "OK", "HOST_BUFFERS_FAILED", "INITIALIZATION_FAILED", "DATA_UPLOAD_FAILED", "CALCULATION_FAILED",
    "DATA_DOWNLOAD_FAILED", "CLEANUP_FAILED", "RESIZE_FAILED", "KERNEL_CREATION_FAILED",
    "PROGRAM_CREATION_FAILED", "NO_SOURCE_FOUND", "LOADING_SOURCE_FAILED",
]

# rsx_option (include/radixsort_hip.h)
OPT_PROFILE, OPT_XCD_REMAP, OPT_FIRST_PASS, OPT_LAST_PASS, OPT_LOOKAHEAD, OPT_REF_DIAGNOSTICS, OPT_GRAPH, OPT_SMALL_SCAN, OPT_TILE_SORT, OPT_FUSED_SCAN = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
OPT_RADIX_BITS, OPT_SELF_SCAN, OPT_SMALL_TILE_MAX_KEYS, OPT_XCD_PHASE, OPT_SELF_SCAN_MAX_TILES, OPT_FUSED_SCAN_MAX_GROUPS = 10, 11, 12, 13, 14, 15
OPT_DESCENDING = 21
# key kinds of rsx_create (RSX_KEY_*): float keys sort in IEEE 754 totalOrder (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN)
KEY_UNSIGNED, KEY_SIGNED, KEY_FLOAT = 0, 1, 2
UNIQUE_CONSECUTIVE = 1     # RSX_UNIQUE_CONSECUTIVE: flags bit 0 of rsx_segmented_unique and rsx_segmented_reduce_by_key
REDUCE_SUM, REDUCE_MIN, REDUCE_MAX = 0, 1, 2                                   # RSX_REDUCE_*: op of rsx_segmented_reduce_by_key
REDUCE_ARGMIN, REDUCE_ARGMAX = 3, 4                                            # ... and the two that rsx_segmented_reduce adds
VALUE_INT32, VALUE_INT64, VALUE_FLOAT32, VALUE_FLOAT64 = 0, 1, 2, 3           # RSX_VALUE_*: its value kinds
SCAN_EXCLUSIVE = 2         # RSX_SCAN_EXCLUSIVE: flags bit 1 of rsx_segmented_scan
SEARCH_RIGHT = 4           # RSX_SEARCH_RIGHT: flags bit 2 of rsx_segmented_search
COMPACT_PARTITION, COMPACT_INVERT, COMPACT_STRICT = 8, 16, 32                  # RSX_COMPACT_*: flags bits 3, 4, 5 of rsx_segmented_compact
EXPAND_GATHER = 64         # RSX_EXPAND_GATHER: flags bit 6 of rsx_segmented_expand
WSELECT_FRACTION = 128     # RSX_WSELECT_FRACTION: flags bit 7 of rsx_segmented_weighted_select
WEIGHT_UINT32, WEIGHT_FLOAT32, WEIGHT_FLOAT64 = 0, 1, 2                        # RSX_WEIGHT_*: its weight kinds
WHIST_SIGNED = 256         # RSX_WHIST_SIGNED: flags bit 8 of rsx_segmented_weighted_histogram
SET_INTERSECTION, SET_DIFFERENCE, SET_UNION, SET_SYMMETRIC_DIFFERENCE = 0, 1, 2, 3       # RSX_SET_*: op of rsx_segmented_set_op
JOIN_INNER, JOIN_LEFT, JOIN_SEMI, JOIN_ANTI = 0, 1, 2, 3                                 # RSX_JOIN_*: op of rsx_segmented_join
RANK_ORDINAL, RANK_MIN, RANK_MAX, RANK_DENSE, RANK_AVERAGE = 0, 1, 2, 3, 4               # RSX_RANK_*: method of rsx_segmented_rank
RANK_METHODS = {"ordinal": RANK_ORDINAL, "min": RANK_MIN, "max": RANK_MAX, "dense": RANK_DENSE, "average": RANK_AVERAGE}
# rsx_experimental_option (include/radixsort_hip_experiments.h): known to the EXPERIMENTS build only (experiments()); the product library refuses them
XOPT_DEBUG_RAISE_SCAN_TIMEOUT, XOPT_INLINE_SCAN, XOPT_INLINE_SCAN_MAX_GROUPS, XOPT_REORDER8_KERNEL, XOPT_REORDER8_STAY = 16, 17, 18, 19, 20
EXPERIMENTS_LIB_PATH = os.path.join(os.path.dirname(_HERE), "tools", "_variants", "libradixsort_hip_experiments.so")

# every symbol include/radixsort_hip.h declares (tests/test_capi_symbols.py checks the header against this)
SYMBOLS = [
    "rsx_device_count", "rsx_device_name", "rsx_last_error", "rsx_version",
    "rsx_create", "rsx_destroy", "rsx_set_stream", "rsx_get_stream", "rsx_set_option", "rsx_get_geometry", "rsx_resize",
    "rsx_upload", "rsx_fill_pad", "rsx_download", "rsx_pin_host", "rsx_unpin_host", "rsx_pipeline_submit", "rsx_pipeline_wait", "rsx_host_device_pointer",
    "rsx_histogram", "rsx_scan", "rsx_paste", "rsx_reorder", "rsx_sort", "rsx_sync", "rsx_check_status",
    "rsx_sort_from", "rsx_partition", "rsx_partition_count", "rsx_partition_scatter", "rsx_sample_keys", "rsx_partition_count_split", "rsx_partition_scatter_split", "rsx_peer_alloc", "rsx_peer_free", "rsx_peer_open", "rsx_peer_close", "rsx_peer_enable", "rsx_sort_from_to", "rsx_segmented_sort", "rsx_segmented_topk", "rsx_segmented_select", "rsx_segmented_weighted_select", "rsx_segmented_unique", "rsx_segmented_reduce_by_key", "rsx_segmented_scan", "rsx_segmented_search", "rsx_segmented_compact", "rsx_segmented_merge", "rsx_segmented_set_op", "rsx_segmented_histogram", "rsx_segmented_weighted_histogram", "rsx_segmented_sample", "rsx_segmented_rank", "rsx_segmented_reduce", "rsx_segmented_expand", "rsx_segmented_join", "rsx_msd_count", "rsx_msd_scatter", "rsx_msd_plan", "rsx_msd_plan_wait", "rsx_msd_push", "rsx_copy_to_device", "rsx_copy_from_device", "rsx_copy_on_device", "rsx_wait_for", "rsx_record_mark", "rsx_wait_mark", "rsx_key_range", "rsx_partition_range", "rsx_result_device", "rsx_copy_result", "rsx_tile_map", "rsx_timings",
]


class PhaseStat(C.Structure):
    _fields_ = [("min_ms", C.c_double), ("max_ms", C.c_double), ("avg_ms", C.c_double), ("sum_ms", C.c_double), ("n", C.c_uint64)]


class Runtimes(C.Structure):   # RuntimesGPU (reference src/RadixSortGPU.h:18-24)
    _fields_ = [("histogram", PhaseStat), ("scan", PhaseStat), ("paste", PhaseStat), ("reorder", PhaseStat), ("total", PhaseStat)]


class Geometry(C.Structure):
    _fields_ = [
        ("tile_threads", C.c_uint32), ("keys_per_thread", C.c_uint32), ("tile_keys", C.c_uint32), ("scan_block", C.c_uint32),
        ("num_keys", C.c_uint64), ("capacity", C.c_uint64), ("num_tiles", C.c_uint64), ("table_len", C.c_uint64),
        ("num_scan_blocks", C.c_uint64), ("num_passes", C.c_uint32), ("key_bytes", C.c_uint32),
        ("fused_scan_resident", C.c_uint32), ("fused_scan_max_groups", C.c_uint32),
    ]


class RadixSortError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        name = STATUS_NAMES[status] if 0 <= status < len(STATUS_NAMES) else str(status)
        super().__init__(f"{where}: OperationStatus::{name}" + (f" ({detail})" if detail else ""))


_lib = None


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  The PyTorch wheel bundles its own libamdhip64.so
    (soname libamdhip64.so.7, but its users ask for it as `libamdhip64.so`); if this
    library pulled in /opt/rocm's copy first, a later `import torch` would map a second
    runtime and find no GPU.  When PyTorch is installed, map its copy first so both sides
    bind the same one.  RSX_NO_TORCH_RUNTIME=1 opts out (pure C/C++ hosts never get here)."""
    if os.environ.get("RSX_NO_TORCH_RUNTIME") or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library() -> C.CDLL:
    """dlopen the HIP library; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    P, U64, I = C.c_void_p, C.c_uint64, C.c_int
    sig = {
        "rsx_device_count": ([C.POINTER(I)], I),
        "rsx_device_name": ([I, C.c_char_p, C.c_size_t], I),
        "rsx_last_error": ([], C.c_char_p),
        "rsx_version": ([], C.c_char_p),
        "rsx_create": ([C.POINTER(P), I, I, I, I, U64], I),
        "rsx_destroy": ([P], I),
        "rsx_set_stream": ([P, P], I),
        "rsx_get_stream": ([P, C.POINTER(P)], I),
        "rsx_set_option": ([P, I, C.c_int64], I),
        "rsx_get_geometry": ([P, C.POINTER(Geometry)], I),
        "rsx_resize": ([P, U64], I),
        "rsx_upload": ([P, P, P, U64], I),
        "rsx_fill_pad": ([P, U64], I),
        "rsx_download": ([P, P, P, P, U64, P, U64], I),
        "rsx_pin_host": ([P, P, U64], I),
        "rsx_unpin_host": ([P, P], I),
        "rsx_pipeline_submit": ([P, P, P, U64, P, P], I),
        "rsx_pipeline_wait": ([P], I),
        "rsx_host_device_pointer": ([P, P, C.POINTER(P)], I),
        "rsx_histogram": ([P, I], I),
        "rsx_scan": ([P], I),
        "rsx_paste": ([P], I),
        "rsx_reorder": ([P, I], I),
        "rsx_sort": ([P], I),
        "rsx_sync": ([P], I),
        "rsx_check_status": ([P], I),
        "rsx_sort_from": ([P, P, P, U64], I),
        "rsx_partition": ([P, P, P, U64, I, I, P, P, C.POINTER(U64)], I),
        "rsx_partition_count": ([P, P, U64, I, I, C.POINTER(U64)], I),
        "rsx_partition_scatter": ([P, P, P, U64, I, I, P, P], I),
        "rsx_sample_keys": ([P, P, U64, C.c_uint32, C.POINTER(U64)], I),
        "rsx_partition_count_split": ([P, P, U64, C.POINTER(U64), I, C.POINTER(U64)], I),
        "rsx_partition_scatter_split": ([P, P, P, U64, P, P], I),
        "rsx_peer_alloc": ([P, U64, C.POINTER(P), P], I),
        "rsx_peer_free": ([P, P], I),
        "rsx_peer_open": ([P, P, C.POINTER(P)], I),
        "rsx_peer_close": ([P, P], I),
        "rsx_peer_enable": ([P, I], I),
        "rsx_sort_from_to": ([P, P, P, U64, I, I, P, P], I),
        "rsx_segmented_sort": ([P, P, P, U64, P, U64, P, P], I),
        "rsx_segmented_topk": ([P, P, U64, P, U64, C.c_uint32, P, P], I),
        "rsx_segmented_select": ([P, P, U64, P, U64, P, C.c_uint32, P, P], I),
        "rsx_segmented_weighted_select": ([P, P, P, U64, P, U64, P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, P, P, P, P, P], I),
        "rsx_segmented_unique": ([P, P, U64, P, U64, C.c_uint32, P, P, P, P, P], I),
        "rsx_segmented_reduce_by_key": ([P, P, P, U64, P, U64, C.c_uint32, C.c_uint32, C.c_uint32, P, P, P, P], I),
        "rsx_segmented_scan": ([P, P, P, U64, P, U64, C.c_uint32, C.c_uint32, C.c_uint32, P], I),
        "rsx_segmented_search": ([P, P, U64, P, U64, P, U64, P, C.c_uint32, P], I),
        "rsx_segmented_compact": ([P, P, U64, P, U64, P, P, C.c_uint32, P, P, P], I),
        "rsx_segmented_merge": ([P, P, P, U64, P, P, P, U64, P, U64, C.c_uint32, P, P, P, P], I),
        "rsx_segmented_set_op": ([P, P, P, U64, P, P, P, U64, P, U64, C.c_uint32, C.c_uint32, P, P, P, P, P], I),
        "rsx_segmented_histogram": ([P, P, U64, P, U64, P, U64, U64, C.c_uint32, U64, C.c_uint32, P], I),
        "rsx_segmented_weighted_histogram": ([P, P, P, U64, P, U64, P, U64, U64, C.c_uint32, U64, C.c_uint32, C.c_uint32, C.c_int32, P], I),
        "rsx_segmented_sample": ([P, P, P, U64, P, U64, P, P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, P, P, P], I),
        "rsx_segmented_rank": ([P, P, U64, P, U64, C.c_uint32, C.c_uint32, P, P], I),
        "rsx_segmented_reduce": ([P, P, U64, P, U64, C.c_uint32, C.c_uint32, C.c_uint32, P, P], I),
        "rsx_segmented_expand": ([P, P, U64, C.c_uint32, P, U64, U64, P, C.c_uint32, P, P, P], I),
        "rsx_segmented_join": ([P, P, U64, P, P, U64, P, U64, C.c_uint32, C.c_uint32, U64, P, P, P, P], I),
        "rsx_msd_count": ([P, P, U64, I, I, P], I),
        "rsx_msd_scatter": ([P, P, P, U64, P, P], I),
        "rsx_msd_plan": ([P, P, C.c_uint32, C.c_uint32, I, I, P], I),
        "rsx_msd_plan_wait": ([P, C.POINTER(U64), C.POINTER(U64), C.POINTER(U64), C.POINTER(U64)], I),
        "rsx_msd_push": ([P, I, P, P, P, P, I, P], I),
        "rsx_copy_to_device": ([P, P, P, U64], I),
        "rsx_copy_from_device": ([P, P, P, U64], I),
        "rsx_copy_on_device": ([P, P, P, U64], I),
        "rsx_wait_for": ([P, P], I),
        "rsx_record_mark": ([P, I], I),
        "rsx_wait_mark": ([P, P, I], I),
        "rsx_key_range": ([P, P, U64, C.POINTER(U64), C.POINTER(U64)], I),
        "rsx_partition_range": ([P, P, P, U64, U64, I, U64, P, P, C.POINTER(U64)], I),
        "rsx_result_device": ([P, C.POINTER(P), C.POINTER(P)], I),
        "rsx_copy_result": ([P, P, P], I),
        "rsx_timings": ([P, C.POINTER(Runtimes), I], I),
        "rsx_tile_map": ([C.c_uint64, C.c_uint32, I, C.c_int64, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)], I),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def variant(lib_path: str):
    """A second, independent instance of this binding over ANOTHER build of the library (A/B builds, the experiments build):
    its own module object, its own dlopen; engines of the two never mix."""
    if not os.path.exists(lib_path):
        raise FileNotFoundError(f"{lib_path} is missing (tools/build_variant.sh, or __graft_entry__.build())")
    name = __name__ + "_variant_" + os.path.splitext(os.path.basename(lib_path))[0]
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, "__init__.py"), submodule_search_locations=[_HERE])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    mod.LIB_PATH = lib_path
    return mod


def experiments():
    """The binding over the experiments build (-DRSX_EXPERIMENTS: rejected kernel variants, inline table scan, test hooks)."""
    return variant(EXPERIMENTS_LIB_PATH)


def device_count() -> int:
    lib = load_library()
    n = C.c_int(0)
    rc = lib.rsx_device_count(C.byref(n))
    if rc != 0:
        raise RadixSortError(rc, "rsx_device_count", lib.rsx_last_error().decode())
    return n.value


def device_name(device: int = 0) -> str:
    lib = load_library()
    buf = C.create_string_buffer(256)
    rc = lib.rsx_device_name(device, buf, 256)
    if rc != 0:
        raise RadixSortError(rc, "rsx_device_name", lib.rsx_last_error().decode())
    return buf.value.decode()


_KEY_DTYPES = _args.KEY_DTYPES      # dtype name -> (key bytes, key kind)


def _opt(p):
    """an optional device address as ctypes wants it: NULL for None and 0"""
    return C.c_void_p(p) if p else None


class Engine:
    """One device + one stream + one buffer set: the C-ABI `rsx_engine`.

    Float keys sort in IEEE 754 totalOrder, bit patterns unchanged: -0.0 before +0.0 and NaNs by sign and payload bits, where numpy
    and torch treat ±0 as equal and put every NaN last.  descending=True sets OPT_DESCENDING: a stable descending sort (equal keys
    keep their input order).  Float and descending engines refuse the partition, key-range, sampling and sharded-sort calls."""

    def __init__(self, dtype, capacity: int, payload: bool = False, device: int = 0, descending: bool = False):
        self.lib = load_library()
        self.dtype = np.dtype(dtype)
        if self.dtype.name not in _KEY_DTYPES:
            raise TypeError(f"unsupported key type {self.dtype}")
        kb, kind = _KEY_DTYPES[self.dtype.name]
        self.key_kind = kind
        self.descending = bool(descending)
        self.payload = bool(payload)
        self.capacity = int(capacity)
        self.device = int(device)
        self._h = C.c_void_p()
        rc = self.lib.rsx_create(C.byref(self._h), device, kb, kind, int(self.payload), self.capacity)
        if rc != 0:
            raise RadixSortError(rc, "rsx_create", self.lib.rsx_last_error().decode())
        if self.descending:
            self.set_option(OPT_DESCENDING, 1)

    @property
    def codec(self) -> bool:
        """True for float keys and descending order: the engine sorts encoded keys and refuses the sharded-sort calls."""
        return self.key_kind == KEY_FLOAT or self.descending

    # -- plumbing ----------------------------------------------------------
    def _check(self, rc: int, where: str) -> None:
        if rc != 0:
            raise RadixSortError(rc, where, self.lib.rsx_last_error().decode())

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.rsx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, hip_stream: int) -> None:
        self._check(self.lib.rsx_set_stream(self._h, C.c_void_p(hip_stream)), "rsx_set_stream")

    def get_stream(self) -> int:
        s = C.c_void_p()
        self._check(self.lib.rsx_get_stream(self._h, C.byref(s)), "rsx_get_stream")
        return int(s.value or 0)

    def set_option(self, option: int, value: int) -> None:
        self._check(self.lib.rsx_set_option(self._h, option, value), "rsx_set_option")
        if option == OPT_DESCENDING:
            self.descending = value != 0

    def geometry(self) -> Geometry:
        g = Geometry()
        self._check(self.lib.rsx_get_geometry(self._h, C.byref(g)), "rsx_get_geometry")
        return g

    # -- reference-shaped steps ---------------------------------------------
    def resize(self, n: int) -> None:
        self._check(self.lib.rsx_resize(self._h, n), "rsx_resize")

    def upload(self, keys: np.ndarray, perm: np.ndarray | None = None) -> None:
        k = np.ascontiguousarray(keys, dtype=self.dtype)
        p = None if perm is None else np.ascontiguousarray(perm, dtype=np.uint32)
        self._check(self.lib.rsx_upload(self._h, k.ctypes.data, p.ctypes.data if p is not None else None, k.size), "rsx_upload")

    def pin_host(self, arr: np.ndarray) -> None:
        self._check(self.lib.rsx_pin_host(self._h, arr.ctypes.data, arr.nbytes), "rsx_pin_host")

    def unpin_host(self, arr: np.ndarray) -> None:
        self._check(self.lib.rsx_unpin_host(self._h, arr.ctypes.data), "rsx_unpin_host")

    def pipeline_submit(self, keys: np.ndarray, out: np.ndarray, perm: np.ndarray | None = None, perm_out: np.ndarray | None = None) -> None:
        """Asynchronous upload -> sort -> download of one job; `keys`/`out` (pinned) must stay alive and untouched until pipeline_wait()."""
        assert keys.dtype == self.dtype and out.dtype == self.dtype and out.size >= keys.size and keys.flags.c_contiguous and out.flags.c_contiguous
        self._check(self.lib.rsx_pipeline_submit(self._h, keys.ctypes.data, perm.ctypes.data if perm is not None else None, keys.size,
                                                 out.ctypes.data, perm_out.ctypes.data if perm_out is not None else None), "rsx_pipeline_submit")

    def pipeline_wait(self) -> None:
        self._check(self.lib.rsx_pipeline_wait(self._h), "rsx_pipeline_wait")

    def host_device_pointer(self, arr: np.ndarray) -> int:
        p = C.c_void_p()
        self._check(self.lib.rsx_host_device_pointer(self._h, arr.ctypes.data, C.byref(p)), "rsx_host_device_pointer")
        return int(p.value or 0)

    def fill_pad(self, byte_offset: int) -> None:
        self._check(self.lib.rsx_fill_pad(self._h, byte_offset), "rsx_fill_pad")

    def histogram(self, pass_: int) -> None:
        self._check(self.lib.rsx_histogram(self._h, pass_), "rsx_histogram")

    def scan(self) -> None:
        self._check(self.lib.rsx_scan(self._h), "rsx_scan")

    def paste(self) -> None:
        self._check(self.lib.rsx_paste(self._h), "rsx_paste")

    def reorder(self, pass_: int) -> None:
        self._check(self.lib.rsx_reorder(self._h, pass_), "rsx_reorder")

    def sort(self) -> None:
        self._check(self.lib.rsx_sort(self._h), "rsx_sort")

    def sync(self) -> None:
        self._check(self.lib.rsx_sync(self._h), "rsx_sync")

    def check_status(self) -> None:
        """Raises if a fused table scan of a sort that has already finished timed out (no synchronisation; reported once)."""
        self._check(self.lib.rsx_check_status(self._h), "rsx_check_status")

    def download(self, want_perm: bool = False, hist_cap: int = 0, globsum_cap: int = 0):
        n = self.geometry().num_keys
        keys = np.empty(n, dtype=self.dtype)
        perm = np.empty(n, dtype=np.uint32) if (want_perm and self.payload) else None
        hist = np.zeros(hist_cap, dtype=np.uint32) if hist_cap else None
        gs = np.zeros(globsum_cap, dtype=np.uint32) if globsum_cap else None
        self._check(self.lib.rsx_download(
            self._h, keys.ctypes.data, perm.ctypes.data if perm is not None else None,
            hist.ctypes.data if hist is not None else None, hist_cap,
            gs.ctypes.data if gs is not None else None, globsum_cap), "rsx_download")
        out = [keys]
        if want_perm:
            out.append(perm)
        if hist_cap:
            out.append(hist)
        if globsum_cap:
            out.append(gs)
        return out[0] if len(out) == 1 else tuple(out)

    # -- device-resident callers ----------------------------------------------
    def sort_from(self, d_keys: int, n: int, d_payload: int | None = None) -> None:
        self._check(self.lib.rsx_sort_from(self._h, C.c_void_p(d_keys), _opt(d_payload), n), "rsx_sort_from")

    def partition(self, d_keys: int, n: int, shift: int, bits: int, d_keys_out: int,
                  d_payload: int | None = None, d_payload_out: int | None = None) -> list[int]:
        offs = (C.c_uint64 * ((1 << bits) + 1))()
        self._check(self.lib.rsx_partition(
            self._h, C.c_void_p(d_keys), _opt(d_payload), n, shift, bits,
            C.c_void_p(d_keys_out), _opt(d_payload_out), offs), "rsx_partition")
        return [int(v) for v in offs]

    def partition_count(self, d_keys: int, n: int, shift: int, bits: int) -> list[int]:
        counts = (C.c_uint64 * (1 << bits))()
        self._check(self.lib.rsx_partition_count(self._h, C.c_void_p(d_keys), n, shift, bits, counts), "rsx_partition_count")
        return [int(v) for v in counts]

    def partition_scatter(self, d_keys: int, n: int, shift: int, bits: int, d_keys_out: int,
                          d_payload: int | None = None, d_payload_out: int | None = None) -> None:
        self._check(self.lib.rsx_partition_scatter(
            self._h, C.c_void_p(d_keys), _opt(d_payload), n, shift, bits,
            C.c_void_p(d_keys_out), _opt(d_payload_out)), "rsx_partition_scatter")

    def sample_keys(self, d_keys: int, n: int, count: int) -> list[int]:
        out = (C.c_uint64 * count)()
        self._check(self.lib.rsx_sample_keys(self._h, C.c_void_p(d_keys), n, count, out), "rsx_sample_keys")
        return [int(v) for v in out]

    def partition_count_split(self, d_keys: int, n: int, splitters: list[int]) -> list[int]:
        m = len(splitters)
        arr = (C.c_uint64 * max(m, 1))(*splitters)
        counts = (C.c_uint64 * (2 * m + 1))()
        self._check(self.lib.rsx_partition_count_split(self._h, C.c_void_p(d_keys), n, arr, m, counts), "rsx_partition_count_split")
        return [int(v) for v in counts]

    def partition_scatter_split(self, d_keys: int, n: int, d_keys_out: int, d_payload: int | None = None, d_payload_out: int | None = None) -> None:
        self._check(self.lib.rsx_partition_scatter_split(
            self._h, C.c_void_p(d_keys), _opt(d_payload), n,
            C.c_void_p(d_keys_out), _opt(d_payload_out)), "rsx_partition_scatter_split")

    def peer_alloc(self, nbytes: int) -> tuple[int, bytes]:
        """A device buffer other ranks may write to: (address, IPC handle for other processes)."""
        p, h = C.c_void_p(), C.create_string_buffer(64)
        self._check(self.lib.rsx_peer_alloc(self._h, nbytes, C.byref(p), h), "rsx_peer_alloc")
        return int(p.value), h.raw

    def peer_free(self, d_ptr: int) -> None:
        self._check(self.lib.rsx_peer_free(self._h, C.c_void_p(d_ptr)), "rsx_peer_free")

    def peer_open(self, handle: bytes) -> int:
        p = C.c_void_p()
        self._check(self.lib.rsx_peer_open(self._h, C.create_string_buffer(handle, 64), C.byref(p)), "rsx_peer_open")
        return int(p.value)

    def peer_close(self, d_ptr: int) -> None:
        self._check(self.lib.rsx_peer_close(self._h, C.c_void_p(d_ptr)), "rsx_peer_close")

    def peer_enable(self, peer_device: int) -> None:
        self._check(self.lib.rsx_peer_enable(self._h, peer_device), "rsx_peer_enable")

    def sort_from_to(self, d_keys: int, n: int, first_pass: int, last_pass: int, d_keys_out: int,
                     d_payload: int | None = None, d_payload_out: int | None = None) -> None:
        """Device-to-device sort over passes [first_pass, last_pass); the last pass writes to d_keys_out."""
        self._check(self.lib.rsx_sort_from_to(
            self._h, C.c_void_p(d_keys), _opt(d_payload), n, first_pass, last_pass,
            C.c_void_p(d_keys_out), _opt(d_payload_out)), "rsx_sort_from_to")

    def segmented_sort(self, d_keys: int, n: int, d_offsets: int, num_segments: int, d_keys_out: int,
                       d_payload: int | None = None, d_payload_out: int | None = None) -> None:
        """Sorts every segment [off[s], off[s+1]) of n device keys into the same range of d_keys_out (d_offsets: DEVICE memory,
        num_segments + 1 uint64 / non-negative int64), asynchronously on the engine's stream.  Bad offsets are reported by the
        next sync() / check_status()."""
        self._check(self.lib.rsx_segmented_sort(
            self._h, C.c_void_p(d_keys), _opt(d_payload), n, C.c_void_p(d_offsets), num_segments,
            C.c_void_p(d_keys_out), _opt(d_payload_out)), "rsx_segmented_sort")

    def segmented_topk(self, d_keys: int, n: int, d_offsets: int, num_segments: int, k: int, d_keys_out: int, d_index_out: int) -> None:
        """The first min(k, L) entries of the stable sort of every segment [off[s], off[s+1]) (L keys) to d_keys_out[s*k ..] and their
        positions relative to off[s] (uint32) to d_index_out[s*k ..]; other slots are not written.  1 <= k <= 4096 (k == 0: nothing).
        Asynchronous on the engine's stream; bad offsets are reported by the next sync() / check_status()."""
        self._check(self.lib.rsx_segmented_topk(
            self._h, C.c_void_p(d_keys), n, C.c_void_p(d_offsets), num_segments, k, C.c_void_p(d_keys_out), C.c_void_p(d_index_out)),
            "rsx_segmented_topk")

    def segmented_select(self, d_keys: int, n: int, d_offsets: int, num_segments: int, d_ranks: int, ranks_per_segment: int,
                         d_keys_out: int, d_index_out: int) -> None:
        """For every segment s = [off[s], off[s+1]) (L keys) and q < R = ranks_per_segment, with r = d_ranks[s*R + q] (DEVICE memory,
        uint32): entry r of the segment's stable sort goes to d_keys_out[s*R + q], its position relative to off[s] (uint32) to
        d_index_out[s*R + q]; slots with r >= L are not written.  1 <= R <= 8 (R == 0: nothing).  Asynchronous on the engine's stream;
        bad offsets are reported by the next sync() / check_status()."""
        self._check(self.lib.rsx_segmented_select(
            self._h, C.c_void_p(d_keys), n, C.c_void_p(d_offsets), num_segments, C.c_void_p(d_ranks), ranks_per_segment,
            C.c_void_p(d_keys_out), C.c_void_p(d_index_out)), "rsx_segmented_select")

    def segmented_weighted_select(self, d_keys: int, d_weights: int | None, n: int, d_offsets: int, num_segments: int, d_targets: int,
                                  targets_per_segment: int, flags: int, weight_kind: int, weight_exp: int, d_keys_out: int, d_index_out: int,
                                  d_rank_out: int | None = None, d_mass_out: int | None = None, d_total_out: int | None = None) -> None:
        """A select by mass: for every segment s and q < R = targets_per_segment, the entry of the segment's stable sort at which the
        running mass of the weights (WEIGHT_UINT32 / WEIGHT_FLOAT32 / WEIGHT_FLOAT64; d_weights None: the float keys are the weights)
        reaches the target d_targets[s*R + q] (uint64 masses, or doubles — fractions of the segment's total — with WSELECT_FRACTION in
        flags): its key goes to d_keys_out[s*R + q], its position relative to off[s] to d_index_out, its rank to d_rank_out and the mass
        up to and including it to d_mass_out (uint64); d_total_out[s] gets the segment's total mass.  A float weight w > 0 weighs
        min(floor(w * 2^(31 - weight_exp)), 2^31), everything else nothing.  Slots without an answer (target 0 or above the total, NaN) are
        not written.  1 <= R <= 4 (R == 0: nothing).  Asynchronous on the engine's stream; bad offsets are reported by the next sync() /
        check_status()."""
        self._check(self.lib.rsx_segmented_weighted_select(
            self._h, C.c_void_p(d_keys), _opt(d_weights), n, C.c_void_p(d_offsets), num_segments, C.c_void_p(d_targets), targets_per_segment,
            flags, weight_kind, weight_exp, C.c_void_p(d_keys_out), C.c_void_p(d_index_out), _opt(d_rank_out), _opt(d_mass_out),
            _opt(d_total_out)), "rsx_segmented_weighted_select")

    def segmented_unique(self, d_keys: int, n: int, d_offsets: int | None, num_segments: int, d_keys_out: int, d_run_offsets_out: int,
                         d_counts_out: int | None = None, d_first_out: int | None = None, d_inverse_out: int | None = None,
                         consecutive: bool = False) -> None:
        """The distinct keys of every segment [off[s], off[s+1]) (consecutive: its runs of adjacent equal keys, nothing sorted), packed
        densely to d_keys_out, with run_offsets (num_segments + 1 uint64), and optionally counts, first positions relative to off[s] and the
        inverse map (n uint32 each).  d_offsets None: ONE segment [0, n).  First positions / the inverse map of a sorted call need a payload
        engine.  Asynchronous on the engine's stream; bad offsets are reported by the next sync() / check_status()."""
        self._check(self.lib.rsx_segmented_unique(
            self._h, C.c_void_p(d_keys), n, _opt(d_offsets), num_segments, UNIQUE_CONSECUTIVE if consecutive else 0,
            C.c_void_p(d_keys_out), C.c_void_p(d_run_offsets_out), _opt(d_counts_out),
            _opt(d_first_out), _opt(d_inverse_out)), "rsx_segmented_unique")

    def segmented_reduce_by_key(self, d_keys: int, d_values: int, n: int, d_offsets: int | None, num_segments: int, op: int, value_kind: int,
                                d_keys_out: int, d_run_offsets_out: int, d_values_out: int, d_counts_out: int | None = None,
                                consecutive: bool = False) -> None:
        """Per segment [off[s], off[s+1]): the distinct keys (consecutive: the runs of adjacent equal keys, nothing sorted) packed densely to
        d_keys_out as segmented_unique packs them, with run_offsets, and op (REDUCE_SUM / MIN / MAX) over the values of every run's
        elements in d_values_out (value_kind: VALUE_INT32 / INT64 / FLOAT32 / FLOAT64; d_values is indexed like d_keys), optionally the
        counts.  Float sums are added in an order fixed by the input alone: equal input, equal bits.  d_offsets None: ONE segment [0, n).
        A sorted call needs a payload engine.  Asynchronous on the engine's stream; bad offsets are reported by the next sync() /
        check_status()."""
        self._check(self.lib.rsx_segmented_reduce_by_key(
            self._h, C.c_void_p(d_keys), C.c_void_p(d_values), n, _opt(d_offsets), num_segments,
            UNIQUE_CONSECUTIVE if consecutive else 0, op, value_kind, C.c_void_p(d_keys_out), C.c_void_p(d_run_offsets_out),
            C.c_void_p(d_values_out), _opt(d_counts_out)), "rsx_segmented_reduce_by_key")

    def segmented_scan(self, d_keys: int | None, d_values: int, n: int, d_offsets: int | None, num_segments: int, op: int, value_kind: int,
                       d_values_out: int, exclusive: bool = False) -> None:
        """The running op (REDUCE_SUM / MIN / MAX) of d_values inside every segment [off[s], off[s+1]) and, with d_keys, inside every run
        of adjacent equal keys (equal by bits; nothing is sorted) into d_values_out; exclusive: the elements before i only, the identity
        at a restart.  d_keys None: segments only; d_offsets None: ONE segment [0, n).  d_values_out == d_values scans in place.  Float
        sums are added in an order fixed by the input alone: equal input, equal bits.  n may exceed the capacity and the engine's sort
        result is left alone.  Asynchronous on the engine's stream; bad offsets (nothing is written then) are reported by the next
        sync() / check_status()."""
        self._check(self.lib.rsx_segmented_scan(
            self._h, _opt(d_keys), C.c_void_p(d_values), n, _opt(d_offsets), num_segments,
            SCAN_EXCLUSIVE if exclusive else 0, op, value_kind, C.c_void_p(d_values_out)), "rsx_segmented_scan")

    def segmented_reduce(self, d_values: int | None, n: int, d_offsets: int | None, num_segments: int, op: int, value_kind: int,
                         d_values_out: int | None, d_index_out: int | None = None) -> None:
        """op (REDUCE_SUM / MIN / MAX / ARGMIN / ARGMAX) over the values of every segment [off[s], off[s+1]) into d_values_out[s], for
        every s: dense by segment id.  d_offsets None: ONE segment [0, n).  An empty segment gets the op's identity (index 0xFFFFFFFF).
        The arg ops need d_index_out (uint32, the FIRST extreme's position in its segment; NaN beats every number) and may leave
        d_values_out None; the others refuse d_index_out.  Float sums are added in an order fixed by the input alone: equal input, equal
        bits.  n may exceed the capacity and the engine's sort result is left alone.  Asynchronous on the engine's stream; bad offsets
        (nothing is written then) are reported by the next sync() / check_status()."""
        self._check(self.lib.rsx_segmented_reduce(
            self._h, _opt(d_values), n, _opt(d_offsets), num_segments, 0, op, value_kind,
            _opt(d_values_out), _opt(d_index_out)), "rsx_segmented_reduce")

    def segmented_expand(self, d_values: int | None, num_values: int, value_bytes: int, d_offsets: int | None, num_segments: int, n: int,
                         d_starts: int | None = None, d_values_out: int | None = None, d_segment_out: int | None = None,
                         d_rank_out: int | None = None) -> None:
        """From offsets back to elements: for every position i of [off[0], off[S]) the segment s(i) that owns it (the largest s with
        off[s] <= i: empty segments own nothing) into d_segment_out[i], i - off[s(i)] into d_rank_out[i] (both uint32) and a value of
        value_bytes = 4 or 8 opaque bytes into d_values_out[i]: d_values[s(i)] (fill form, num_values == num_segments) or, with
        d_starts, d_values[starts[s(i)] + rank] (gather form, EXPAND_GATHER).  n is the element count of the outputs; positions outside
        [off[0], off[S]) are not written.  Any subset of the outputs, at least one; pointers need their element's alignment only.  n may
        exceed the capacity and the engine's sort result is left alone.  Asynchronous on the engine's stream; bad offsets or starts
        (nothing is written then) are reported by the next sync() / check_status()."""
        self._check(self.lib.rsx_segmented_expand(
            self._h, _opt(d_values), num_values, value_bytes, _opt(d_offsets), num_segments, n,
            _opt(d_starts), EXPAND_GATHER if d_starts else 0, _opt(d_values_out),
            _opt(d_segment_out), _opt(d_rank_out)), "rsx_segmented_expand")

    def segmented_search(self, d_sorted: int | None, n: int, d_offsets: int | None, num_segments: int, d_queries: int, num_queries: int,
                         d_query_offsets: int | None, d_index_out: int, right: bool = False) -> None:
        """For every query, the number of keys of its haystack segment [off[s], off[s+1]) that come strictly before it in the engine's order
        (right: that do not come after it) into d_index_out (uint32, relative to off[s]): lower / upper bound on an ascending engine.  The
        segments must be sorted in the engine's order (key kind, totalOrder for floats, direction).  d_offsets None: one segment [0, n) and
        the queries [0, num_queries); d_query_offsets None: every segment has num_queries / num_segments queries; else query segment s is
        [qoff[s], qoff[s+1]).  n may exceed the capacity and the engine's sort result is left alone.  Asynchronous on the engine's stream;
        bad offsets (nothing is written then) are reported by the next sync() / check_status()."""
        self._check(self.lib.rsx_segmented_search(
            self._h, _opt(d_sorted), n, _opt(d_offsets), num_segments,
            _opt(d_queries), num_queries, _opt(d_query_offsets),
            SEARCH_RIGHT if right else 0, _opt(d_index_out)), "rsx_segmented_search")

    def segmented_compact(self, d_keys: int, n: int, d_offsets: int | None, num_segments: int, d_mask: int | None, d_bounds: int | None,
                          d_keys_out: int | None, d_index_out: int | None, d_kept_offsets_out: int, partition: bool = False, invert: bool = False,
                          strict: bool = False) -> None:
        """Stream compaction of every segment [off[s], off[s+1]): element i is kept iff d_mask[i] != 0 (one byte per element), or - d_bounds,
        one key per segment - iff its key does not come after the segment's bound in the engine's order (strict: comes strictly before);
        invert keeps the others.  The kept elements go densely packed, in input order, to d_keys_out, their positions relative to off[s]
        to d_index_out (uint32), and d_kept_offsets_out (num_segments + 1 uint64) gets the number kept before every segment.  partition:
        nothing is dropped; every segment is rewritten in place of its index range, kept elements first, both sides in input order.
        Either output may be None (both: count only).  d_offsets None: ONE segment [0, n).  n may exceed the capacity and the engine's
        sort result is left alone.  Asynchronous on the engine's stream; bad offsets (the kept offsets are zeros then, nothing else is
        written) are reported by the next sync() / check_status()."""
        flags = (COMPACT_PARTITION if partition else 0) | (COMPACT_INVERT if invert else 0) | (COMPACT_STRICT if strict else 0)
        self._check(self.lib.rsx_segmented_compact(
            self._h, _opt(d_keys), n, _opt(d_offsets), num_segments, _opt(d_mask), _opt(d_bounds), flags, _opt(d_keys_out), _opt(d_index_out),
            _opt(d_kept_offsets_out)), "rsx_segmented_compact")

    def segmented_merge(self, d_a: int | None, na: int, d_a_offsets: int | None, d_b: int | None, nb: int, d_b_offsets: int | None, num_segments: int,
                        d_keys_out: int | None, d_index_out: int | None = None, d_out_offsets: int | None = None, d_a_payload: int | None = None,
                        d_b_payload: int | None = None, d_payload_out: int | None = None, flags: int = 0) -> None:
        """The stable merge of sorted segment s of A, d_a[aoff[s] .. aoff[s+1]), with sorted segment s of B, for every s, in one pass: output
        segment [ooff[s], ooff[s+1]), ooff[s] = (aoff[s] - aoff[0]) + (boff[s] - boff[0]), holds the stable sort in the engine's order of
        A_s ++ B_s (an A key before the B keys equal to it), d_index_out (uint32) the position of every output in that concatenation,
        d_payload_out the 32-bit payload word that came with each key (the three payload pointers all or none), d_out_offsets
        (num_segments + 1 uint64) the ooff.  Both offsets None: ONE segment [0, na) and [0, nb).  The segments must be sorted in the
        engine's order (key kind, totalOrder for floats, direction).  Each output may be None, not all.  na + nb may exceed the capacity,
        the engine's sort result is left alone, and has_payload does not matter.  Asynchronous on the engine's stream; bad offsets
        (d_out_offsets holds zeros then, nothing else is written) are reported by the next sync() / check_status()."""
        self._check(self.lib.rsx_segmented_merge(
            self._h, _opt(d_a), _opt(d_a_payload), na, _opt(d_a_offsets), _opt(d_b), _opt(d_b_payload), nb, _opt(d_b_offsets), num_segments, flags,
            _opt(d_keys_out), _opt(d_payload_out), _opt(d_index_out), _opt(d_out_offsets)), "rsx_segmented_merge")

    def segmented_set_op(self, d_a: int | None, na: int, d_a_offsets: int | None, d_b: int | None, nb: int, d_b_offsets: int | None, num_segments: int,
                         op: int, d_keys_out: int | None, d_out_offsets: int | None, d_index_out: int | None = None, d_match_out: int | None = None,
                         d_a_payload: int | None = None, d_b_payload: int | None = None, d_payload_out: int | None = None, flags: int = 0) -> None:
        """A set operation (op: SET_INTERSECTION, SET_DIFFERENCE - A minus B -, SET_UNION, SET_SYMMETRIC_DIFFERENCE) on sorted segment s
        of A, d_a[aoff[s] .. aoff[s+1]), and sorted segment s of B, for every s, with std::set_*'s rule for duplicates: of a key that occurs
        m times in A_s and n times in B_s the intersection keeps A's first min(m, n), the difference A's last max(m - n, 0), the union all
        of A and B's last max(n - m, 0), the symmetric difference A's last max(m - n, 0) and B's last max(n - m, 0).  The kept elements come
        in the stable merge's order, densely packed; d_out_offsets (num_segments + 1 uint64, required) gets the number kept before every
        segment, d_index_out (uint32) the position in A_s ++ B_s, d_match_out (intersection only) the partner's position in B_s,
        d_payload_out the 32-bit word that came with each key (the three payload pointers all or none).  Output buffers hold na elements
        for intersection and difference, na + nb for the other two.  Both offsets None: ONE segment.  na + nb may exceed the capacity, the
        engine's sort result is left alone, and has_payload does not matter.  Asynchronous on the engine's stream; bad offsets
        (d_out_offsets holds zeros then, nothing else is written) are reported by the next sync() / check_status()."""
        self._check(self.lib.rsx_segmented_set_op(
            self._h, _opt(d_a), _opt(d_a_payload), na, _opt(d_a_offsets), _opt(d_b), _opt(d_b_payload), nb, _opt(d_b_offsets), num_segments, op, flags,
            _opt(d_keys_out), _opt(d_payload_out), _opt(d_index_out), _opt(d_match_out), _opt(d_out_offsets)), "rsx_segmented_set_op")

    def segmented_join(self, d_a: int | None, na: int, d_a_offsets: int | None, d_b: int | None, nb: int, d_b_offsets: int | None, num_segments: int,
                       op: int, out_capacity: int, d_out_offsets: int | None, d_a_index_out: int | None = None, d_b_index_out: int | None = None,
                       d_keys_out: int | None = None, flags: int = 0) -> None:
        """The equi-join (op: JOIN_INNER, JOIN_LEFT, JOIN_SEMI, JOIN_ANTI) of sorted segment s of A, d_a[aoff[s] .. aoff[s+1]), with sorted
        segment s of B, for every s.  An A element i (relative to aoff[s]) whose key has the lower bound lb and c partners in B_s emits:
        INNER the rows (i, lb + r), r < c; LEFT the same and (i, 0xFFFFFFFF) where c == 0; SEMI (i, lb) iff c > 0; ANTI (i, -) iff c == 0
        (no d_b_index_out).  Rows come by segment, A position, B position, densely packed: d_a_index_out / d_b_index_out (uint32, relative
        to the segment), d_keys_out (the A key).  d_out_offsets (num_segments + 1 uint64, required) gets the TRUE number of rows before
        every segment whatever out_capacity is; exactly the rows below min(total, out_capacity) are written (out_capacity: elements of each
        row buffer).  All three row outputs None: count only.  Both offsets None: ONE segment.  Keys are equal iff their bits are.  na,
        nb and the total may exceed the capacity, the engine's sort result is left alone, and has_payload does not matter.  Asynchronous
        on the engine's stream; bad offsets (d_out_offsets holds zeros then, nothing else is written) are reported by the next sync() /
        check_status()."""
        self._check(self.lib.rsx_segmented_join(
            self._h, _opt(d_a), na, _opt(d_a_offsets), _opt(d_b), nb, _opt(d_b_offsets), num_segments, op, flags, out_capacity,
            _opt(d_keys_out), _opt(d_a_index_out), _opt(d_b_index_out), _opt(d_out_offsets)), "rsx_segmented_join")

    def key_bits(self, value) -> int:
        """The bit pattern of the Python number `value` as a key of this engine (two's complement for integers, IEEE 754 for floats)."""
        if self.key_kind == KEY_FLOAT:
            return int(np.array(value, dtype=self.dtype).view(np.uint32 if self.dtype.itemsize == 4 else np.uint64))
        return int(value) & ((1 << (8 * self.dtype.itemsize)) - 1)

    def segmented_histogram(self, d_keys: int | None, n: int, d_offsets: int | None, num_segments: int, num_bins: int, d_counts_out: int,
                            d_edges: int | None = None, lo=0, hi=0, width_shift: int = 0) -> None:
        """The keys of every segment [off[s], off[s+1]) counted per bin into d_counts_out (num_segments x num_bins uint32, row-major; the
        call zeroes them itself; keys that fall into no bin are dropped).  d_edges (num_bins + 1 keys sorted in the engine's order, at most
        4096 bins): bin j holds edges[j] <= k < edges[j+1] in that order, the last bin closed on both sides: numpy.histogram(x, bins=edges)
        on an ascending engine.  Without edges, integer keys: bin (k - lo) >> width_shift (lo = 0, width_shift = 0: bincount); float keys:
        bin min(num_bins - 1, floor((x - lo) * (num_bins / (hi - lo)))) for lo <= x <= hi, NaN dropped (histc).  lo and hi are Python
        numbers.  A descending engine numbers the even forms' bins backwards.  d_offsets None: ONE segment [0, n).  n may exceed the
        capacity and the engine's sort result is left alone.  Asynchronous on the engine's stream; bad offsets (every counter is zero
        then) are reported by the next sync() / check_status()."""
        even = not d_edges
        self._check(self.lib.rsx_segmented_histogram(
            self._h, _opt(d_keys), n, _opt(d_offsets), num_segments, _opt(d_edges), self.key_bits(lo) if even else int(lo),
            self.key_bits(hi) if even else int(hi), width_shift, num_bins, 0, _opt(d_counts_out)), "rsx_segmented_histogram")

    def segmented_weighted_histogram(self, d_keys: int | None, d_weights: int | None, n: int, d_offsets: int | None, num_segments: int, num_bins: int,
                                     d_sums_out: int, weight_kind: int, weight_exp: int = 0, flags: int = 0, d_edges: int | None = None, lo=0, hi=0,
                                     width_shift: int = 0) -> None:
        """The MASSES of the keys of every segment [off[s], off[s+1]) summed per bin into d_sums_out (num_segments x num_bins 64-bit words,
        row-major; the call zeroes them itself).  The bin of a key is segmented_histogram's (d_edges, lo, hi, width_shift, num_bins as
        there).  d_weights: n weights of weight_kind (WEIGHT_UINT32: raw masses, weight_exp 0; WEIGHT_FLOAT32 / WEIGHT_FLOAT64: w > 0
        weighs min(floor(w * 2^(31 - weight_exp)), 2^31), everything else nothing — segmented_weighted_select's rule).  flags
        WHIST_SIGNED (float kinds): the mass of |w|, added negated for a negative weight; the sums are then int64.  All sums are 64-bit
        integer adds: bitwise reproducible.  d_offsets None: ONE segment [0, n).  n may exceed the capacity and the engine's sort result
        is left alone.  Asynchronous on the engine's stream; bad offsets (every sum is zero then) are reported by the next sync() /
        check_status()."""
        even = not d_edges
        self._check(self.lib.rsx_segmented_weighted_histogram(
            self._h, _opt(d_keys), _opt(d_weights), n, _opt(d_offsets), num_segments, _opt(d_edges), self.key_bits(lo) if even else int(lo),
            self.key_bits(hi) if even else int(hi), width_shift, num_bins, flags, weight_kind, weight_exp, _opt(d_sums_out)),
            "rsx_segmented_weighted_histogram")

    def segmented_sample(self, d_keys: int | None, d_weights: int | None, n: int, d_offsets: int | None, num_segments: int, d_bounds: int | None,
                         d_targets: int, draws_per_segment: int, flags: int, weight_kind: int, weight_exp: int, d_index_out: int,
                         d_mass_out: int | None = None, d_total_out: int | None = None) -> None:
        """draws_per_segment categorical draws from every segment [off[s], off[s+1]), in INPUT order and without sorting: for the target T
        of slot s * R + q, d_index_out gets the smallest index i (relative to off[s], uint32) whose running mass m_0 + ... + m_i reaches
        T, d_mass_out (optional) that running mass and d_total_out[s] (optional) the segment's mass.  The mass of a weight is
        segmented_weighted_select's (weight_kind, weight_exp; d_weights None: the float keys are their own weights).  d_bounds (one key
        per segment): an element that segmented_compact's bound predicate rejects weighs nothing (flags COMPACT_STRICT, COMPACT_INVERT).
        d_targets: uint64 masses, or with WSELECT_FRACTION doubles u, T = clamp(ceil(total * u), 1, total).  A slot without an answer
        (T == 0, T > total, NaN, no mass) is not written.  d_keys is read only with d_bounds or without d_weights.  d_offsets None: ONE
        segment [0, n).  n may exceed the capacity and the engine's sort result is left alone.  All sums are 64-bit integer adds:
        bitwise reproducible.  Asynchronous on the engine's stream; bad offsets (nothing is written then) are reported by the next
        sync() / check_status()."""
        self._check(self.lib.rsx_segmented_sample(
            self._h, _opt(d_keys), _opt(d_weights), n, _opt(d_offsets), num_segments, _opt(d_bounds), _opt(d_targets), draws_per_segment, flags,
            weight_kind, weight_exp, _opt(d_index_out), _opt(d_mass_out), _opt(d_total_out)), "rsx_segmented_sample")

    def segmented_rank(self, d_keys: int, n: int, d_offsets: int | None, num_segments: int, method: int, d_rank_out: int,
                       d_ties_out: int | None = None) -> None:
        """The 0-based rank (uint32) of every key inside its segment [off[s], off[s+1]) in the engine's order, under the tie rule `method`
        (RANK_ORDINAL: the position in the stable sort; RANK_MIN / RANK_MAX: the first / last position of its tie group; RANK_DENSE: the
        distinct keys before it; RANK_AVERAGE: min + max, TWICE the average rank), and to d_ties_out (optional) the size of its tie group.
        Keys tie iff their bits are equal (floats: IEEE 754 totalOrder).  d_offsets None: ONE segment [0, n).  Needs a payload engine and
        n <= capacity; the engine's buffers are overwritten.  No atomic and no float operation: bitwise reproducible.  Asynchronous on the
        engine's stream; bad offsets (nothing is written then) are reported by the next sync() / check_status()."""
        self._check(self.lib.rsx_segmented_rank(self._h, _opt(d_keys), n, _opt(d_offsets), num_segments, 0, method, _opt(d_rank_out), _opt(d_ties_out)),
                    "rsx_segmented_rank")

    # -- exchange step of the sharded sort on the top B <= 8 bits ----------------
    def msd_count(self, d_keys: int, n: int, bits: int, world: int, d_counts: int) -> None:
        """Keys per bucket of the top `bits` bits into device memory (256 x uint64 at d_counts, natural order), asynchronously."""
        self._check(self.lib.rsx_msd_count(self._h, C.c_void_p(d_keys), n, bits, world, C.c_void_p(d_counts)), "rsx_msd_count")

    def msd_scatter(self, d_keys: int, n: int, d_staging: int, d_payload: int | None = None, d_staging_payload: int | None = None) -> None:
        self._check(self.lib.rsx_msd_scatter(self._h, C.c_void_p(d_keys), _opt(d_payload), n, C.c_void_p(d_staging),
                                             _opt(d_staging_payload)), "rsx_msd_scatter")

    def msd_plan(self, d_table: int, stride: int, cap_at: int, rank: int, hip_stream: int = 0, grouping: int = 0) -> None:
        self._check(self.lib.rsx_msd_plan(self._h, C.c_void_p(d_table), stride, cap_at, rank, grouping, _opt(hip_stream)), "rsx_msd_plan")

    def msd_plan_wait(self, waves: int, world: int) -> tuple[list[int], list[int], list[int], int]:
        """(first slot of every wave in this rank's receive buffer, keys of every wave, keys every rank ends up with, verdict bits)"""
        ws, wc, ld, v = (C.c_uint64 * waves)(), (C.c_uint64 * waves)(), (C.c_uint64 * world)(), C.c_uint64()
        self._check(self.lib.rsx_msd_plan_wait(self._h, ws, wc, ld, C.byref(v)), "rsx_msd_plan_wait")
        return [int(x) for x in ws], [int(x) for x in wc], [int(x) for x in ld], int(v.value)

    def msd_push(self, wave: int, d_staging: int, d_peer_keys: int, d_staging_payload: int | None = None, d_peer_payload: int | None = None, parts: int = 0,
                 hip_stream: int = 0) -> None:
        """Wave `wave` of the staging buffer into the owners' receive buffers, on hip_stream (0: the engine's stream)."""
        self._check(self.lib.rsx_msd_push(self._h, wave, C.c_void_p(d_staging), _opt(d_staging_payload),
                                          C.c_void_p(d_peer_keys), _opt(d_peer_payload), parts,
                                          _opt(hip_stream)), "rsx_msd_push")

    def wait_for(self, other: "Engine") -> None:
        """This engine's stream waits for everything enqueued on `other`'s stream so far."""
        self._check(self.lib.rsx_wait_for(self._h, other._h), "rsx_wait_for")

    def record_mark(self, slot: int) -> None:
        """Marks "everything enqueued on this engine's stream so far" under `slot` (0..255)."""
        self._check(self.lib.rsx_record_mark(self._h, slot), "rsx_record_mark")

    def wait_mark(self, other: "Engine", slot: int) -> None:
        """This engine's stream waits for `other`'s mark `slot`."""
        self._check(self.lib.rsx_wait_mark(self._h, other._h, slot), "rsx_wait_mark")

    def key_range(self, d_keys: int, n: int) -> tuple[int, int]:
        lo, hi = C.c_uint64(), C.c_uint64()
        self._check(self.lib.rsx_key_range(self._h, C.c_void_p(d_keys), n, C.byref(lo), C.byref(hi)), "rsx_key_range")
        return int(lo.value), int(hi.value)

    def partition_range(self, d_keys: int, n: int, lo: int, shift: int, mul: int, d_keys_out: int,
                        d_payload: int | None = None, d_payload_out: int | None = None) -> list[int]:
        offs = (C.c_uint64 * 17)()
        self._check(self.lib.rsx_partition_range(
            self._h, C.c_void_p(d_keys), _opt(d_payload), n, lo, shift, mul,
            C.c_void_p(d_keys_out), _opt(d_payload_out), offs), "rsx_partition_range")
        return [int(v) for v in offs]

    def result_device(self) -> tuple[int, int]:
        k, p = C.c_void_p(), C.c_void_p()
        self._check(self.lib.rsx_result_device(self._h, C.byref(k), C.byref(p)), "rsx_result_device")
        return int(k.value or 0), int(p.value or 0)

    def copy_result(self, d_keys_out: int, d_payload_out: int | None = None) -> None:
        self._check(self.lib.rsx_copy_result(self._h, C.c_void_p(d_keys_out), _opt(d_payload_out)), "rsx_copy_result")

    def timings(self, reset: bool = False) -> Runtimes:
        r = Runtimes()
        self._check(self.lib.rsx_timings(self._h, C.byref(r), int(reset)), "rsx_timings")
        return r


def tile_map(num_keys: int, tile_keys: int = 4096, xcd_remap: bool = True, xcd_phase: int = -1) -> tuple[np.ndarray, int]:
    """Tile of every workgroup of a launch over num_keys keys (rsx_tile_map: host arithmetic, no GPU) and the tile count."""
    lib = load_library()
    blocks, ntiles = C.c_uint32(0), C.c_uint32(0)
    rc = lib.rsx_tile_map(num_keys, tile_keys, int(xcd_remap), xcd_phase, None, 0, C.byref(blocks), C.byref(ntiles))
    if rc != 0:
        raise RadixSortError(rc, "rsx_tile_map", lib.rsx_last_error().decode())
    out = np.empty(blocks.value, dtype=np.uint32)
    rc = lib.rsx_tile_map(num_keys, tile_keys, int(xcd_remap), xcd_phase, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(blocks), C.byref(ntiles))
    if rc != 0:
        raise RadixSortError(rc, "rsx_tile_map", lib.rsx_last_error().decode())
    return out, ntiles.value


def sort_host(keys: np.ndarray, payload: np.ndarray | None = None, device: int = 0, descending: bool = False):
    """upload -> sort -> download of a host array (the shape of ExecuteTask,
    reference src/CRadixSortTask.cpp:289-314).  Returns sorted keys (and payload).  Stable in both directions."""
    k = np.ascontiguousarray(keys)
    with Engine(k.dtype, max(k.size, 1), payload=payload is not None, device=device, descending=descending) as e:
        e.upload(k, payload)
        e.sort()
        if payload is None:
            return e.download()
        return e.download(want_perm=True)


# -- segmented sort on torch tensors ---------------------------------------------------------------------------------------------
# One engine per (device, stream, dtype, payload, descending), grown to the largest n seen.  The stream is part of the key: an engine's
# ping-pong buffers and segmented scratch serve one call at a time, so calls that may overlap (different torch streams) get their own.
_SEG_ENGINES: dict = {}


def _cached_engine(cache: dict, key: tuple, dtype_name: str, capacity: int, payload: bool = False, descending: bool = False) -> "Engine":
    """The engine of a cache under `key` = (device, stream, ...), created on that device and bound to that stream on first use."""
    eng = cache.get(key)
    if eng is None:
        eng = Engine(dtype_name, capacity, payload=payload, device=key[0], descending=descending)
        eng.set_stream(key[1])
        cache[key] = eng
    return eng


def _segmented_engine(device: int, stream: int, dtype_name: str, payload: bool, descending: bool, n: int) -> "Engine":
    key = (device, stream, dtype_name, payload, descending)
    eng = _SEG_ENGINES.get(key)
    if eng is not None and eng.capacity < n:          # too small: replaced by one of the next power of two
        eng.close()
        del _SEG_ENGINES[key]
    cap = max(n, 1 << 12)
    cap = 1 << (cap - 1).bit_length() if cap < (1 << 31) else cap
    return _cached_engine(_SEG_ENGINES, key, dtype_name, cap, payload, descending)


_aligned_copy = _args.aligned_copy


def _keys_and_offsets(what: str, keys, offsets) -> str:
    """What sort, topk and select ask of their input: 1-D device keys of a key type (its name) and offsets on their device."""
    if keys.dim() != 1 or not keys.is_cuda:
        raise ValueError(f"{what}: keys must be a 1-D device tensor")
    name = _args.key_name(what, keys)
    _args.check_offsets(what, offsets, keys.device)
    return name


def segmented_sort(keys, offsets, payload=None, descending: bool = False):
    """Stable sort of every segment [offsets[s], offsets[s+1]) of the 1-D device tensor `keys` in ONE engine call (rsx_segmented_sort).
    offsets: int64 device tensor of num_segments + 1 non-negative entries; payload: optional int32 / uint32 tensor like keys.
    Returns new (keys, payload) tensors (payload None without one); positions outside [offsets[0], offsets[-1]) are copied unchanged.
    Float keys sort in IEEE 754 totalOrder.  Bad offsets raise at the engine's next synchronisation (this call does not read them)."""
    import torch
    name = _keys_and_offsets("segmented_sort", keys, offsets)
    n = keys.numel()
    nseg = offsets.numel() - 1
    k_in = _aligned_copy(keys)
    k_out = k_in.clone()
    p_in = p_out = None
    if payload is not None:
        if payload.shape != keys.shape or payload.device != keys.device or payload.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
            raise ValueError("segmented_sort: payload must be an int32 / uint32 tensor shaped like keys, on the same device")
        p_in = _aligned_copy(payload)
        p_out = p_in.clone()
    if n == 0 or nseg <= 0:
        return k_out, p_out
    off = _args.as_offsets(offsets)
    eng = _segmented_engine(*_args.device_and_stream(keys), name, p_in is not None, bool(descending), n)
    eng.segmented_sort(k_in.data_ptr(), n, off.data_ptr(), nseg, k_out.data_ptr(), _args.ptr(p_in), _args.ptr(p_out))
    eng.check_status()      # reports bad offsets of calls that have already finished
    return k_out, p_out


def sort_rows(x, descending: bool = False):
    """torch.sort(x, dim=-1, descending=descending, stable=True) of a 2-D device tensor through ONE segmented call: returns
    (values, indices), indices as int64 column positions.  Equal to torch for integer dtypes and for floats without -0.0 and
    without negative-sign NaNs (float keys sort in IEEE 754 totalOrder here)."""
    import torch
    if x.dim() != 2:
        raise ValueError("sort_rows: x must be a 2-D tensor")
    rows, cols = x.shape
    if rows == 0 or cols == 0:
        return x.clone(), torch.zeros(x.shape, dtype=torch.int64, device=x.device)
    _args.check_count("sort_rows", "rsx_segmented_sort", "elements", rows * cols)
    flat = x.contiguous().reshape(-1)
    offsets = torch.arange(0, rows + 1, device=x.device, dtype=torch.int64) * cols
    col = torch.arange(cols, device=x.device, dtype=torch.int64).to(torch.int32).repeat(rows)      # uint32 bits (cols may reach 2^31)
    values, idx = segmented_sort(flat, offsets, col, descending=descending)
    return values.reshape(rows, cols), _args.widen(idx).reshape(rows, cols)      # the uint32 payload, unsigned


# -- top-k on torch tensors ---------------------------------------------------------------------------------------------------------
TOPK_MAX_K = 4096       # rsx_segmented_topk's bound: one LDS tile


def segmented_topk(keys, offsets, k: int, largest: bool = True):
    """The k largest (largest=True) or smallest entries of every segment [offsets[s], offsets[s+1]) of the 1-D device tensor `keys` in ONE
    engine call (rsx_segmented_topk, 1 <= k <= 4096).  offsets: int64 device tensor of num_segments + 1 non-negative entries.
    Returns (values [S, k], indices [S, k] int64), sorted best first, ties lowest index first, indices relative to the segment start.
    Slots past a segment's length hold value 0 and index -1.  Float keys follow IEEE 754 totalOrder (+NaN above +inf; -0.0 below +0.0,
    negative-sign NaNs below -inf).  Bad offsets raise at the engine's next synchronisation (this call does not read them); their rows
    hold 0 / -1."""
    import torch
    name = _keys_and_offsets("segmented_topk", keys, offsets)
    k = int(k)
    if k < 0 or k > TOPK_MAX_K:
        raise ValueError(f"segmented_topk: k must be in [0, {TOPK_MAX_K}] (sort_rows / segmented_sort and a slice for larger k)")
    n = keys.numel()
    nseg = max(offsets.numel() - 1, 0)
    values = torch.zeros((nseg, k), dtype=keys.dtype, device=keys.device)
    idx = torch.full((nseg, k), -1, dtype=torch.int32, device=keys.device)     # the uint32 output's bits: -1 marks an unwritten slot
    if n == 0 or nseg == 0 or k == 0:
        return values, idx.to(torch.int64)
    k_in = _aligned_copy(keys)
    off = _args.as_offsets(offsets)
    eng = _segmented_engine(*_args.device_and_stream(keys), name, False, bool(largest), n)      # largest: a descending engine
    eng.segmented_topk(k_in.data_ptr(), n, off.data_ptr(), nseg, k, values.data_ptr(), idx.data_ptr())
    eng.check_status()      # reports bad offsets of calls that have already finished
    return values, idx.to(torch.int64)      # uint32 positions below 2^31 (n <= 2^31): non-negative as int32


def topk(x, k: int, dim: int = -1, largest: bool = True, sorted: bool = True):
    """torch.topk(x, k, dim, largest) on a device tensor: (values, indices int64) shaped like torch.topk's, always sorted (best first,
    equal values lowest index first; sorted=False is accepted).  Every row along `dim` is one segment of ONE rsx_segmented_topk call.
    Values equal torch.topk's for integer dtypes and for floats without -0.0 and negative-sign NaNs (float keys follow IEEE 754
    totalOrder here); indices equal the first k of torch.sort(stable=True)'s.  For k > 4096 this falls back to sort_rows (one
    segmented sort) and a slice.  Supported dtypes: int32, uint32, int64, uint64, float32, float64 (TypeError otherwise)."""
    import torch
    if not x.is_cuda:
        raise ValueError("topk: x must be a device tensor")
    if _args.dtype_name(x) not in _KEY_DTYPES:
        raise TypeError(f"topk: unsupported dtype {x.dtype}")
    del sorted                                                  # the output is always sorted
    squeeze = x.dim() == 0          # torch.topk of a 0-d tensor: one row of one element, 0-d results
    if squeeze:
        x = x.reshape(1)
    dim = dim % x.dim()
    size = x.shape[dim]
    k = int(k)
    if k < 0 or k > size:
        raise ValueError(f"topk: k = {k} is out of range for dimension {dim} of size {size}")
    xm = x.movedim(dim, -1)
    out_shape = xm.shape[:-1] + (k,)
    rows = xm.numel() // size if size else 0
    if k == 0 or rows == 0:
        v = torch.empty(out_shape, dtype=x.dtype, device=x.device)
        i = torch.empty(out_shape, dtype=torch.int64, device=x.device)
    else:
        flat = xm.contiguous().reshape(rows, size)
        if k > TOPK_MAX_K:
            sv, si = sort_rows(flat, descending=largest)
            v, i = sv[:, :k].contiguous(), si[:, :k].contiguous()
        else:
            _args.check_count("topk", "rsx_segmented_topk", "elements", rows * size)
            offsets = torch.arange(0, rows + 1, device=x.device, dtype=torch.int64) * size
            v, i = segmented_topk(flat.reshape(-1), offsets, k, largest=largest)
        v, i = v.reshape(out_shape), i.reshape(out_shape)
    v, i = v.movedim(-1, dim), i.movedim(-1, dim)
    if squeeze and k == 1:
        v, i = v.reshape(()), i.reshape(())
    return v, i


# -- selection on torch tensors: k-th value, median, quantiles ----------------------------------------------------------------------
SELECT_MAX_RANKS = 8       # rsx_segmented_select's bound per call; more ranks are served in chunks
QUANTILE_MODES = ("linear", "lower", "higher", "midpoint", "nearest")


def segmented_select(keys, offsets, ranks, descending: bool = False):
    """Entry ranks[s, q] of the stable sort of every segment [offsets[s], offsets[s+1]) of the 1-D device tensor `keys`, without sorting
    (rsx_segmented_select; ranks are not limited to 4096 as segmented_topk's k is).  offsets: int64 device tensor of num_segments + 1
    non-negative entries; ranks: integer device tensor [S, R] or [S], 0-based, in the direction given (descending: rank 0 is the largest).
    Returns (values [S, R], indices [S, R] int64), indices relative to the segment start.  A rank that is negative or not below its
    segment's length selects nothing: the slot holds value 0 and index -1.  More than 8 ranks per segment take one engine call per 8.
    Equal keys rank in index order, so the index of a tie is defined (torch leaves it open).  Float keys follow IEEE 754 totalOrder (+NaN
    above +inf; -0.0 below +0.0, negative-sign NaNs below -inf).  Bad offsets raise at the engine's next synchronisation (this call does
    not read them); their rows hold 0 / -1."""
    import torch
    name = _keys_and_offsets("segmented_select", keys, offsets)
    nseg = max(offsets.numel() - 1, 0)
    if ranks.device != keys.device or ranks.is_floating_point() or ranks.dtype == torch.bool or ranks.dim() not in (1, 2) or ranks.shape[0] != nseg:
        raise ValueError("segmented_select: ranks must be an integer tensor [num_segments, R] or [num_segments] on the keys' device")
    r64 = ranks.reshape(nseg, -1).to(torch.int64)
    R = r64.shape[1]
    n = keys.numel()
    values = torch.zeros((nseg, R), dtype=keys.dtype, device=keys.device)
    idx = torch.full((nseg, R), -1, dtype=torch.int32, device=keys.device)     # the uint32 output's bits: -1 marks an unwritten slot
    if n == 0 or nseg == 0 or R == 0:
        return values, idx.to(torch.int64)
    # uint32 bits for the engine; n <= 2^31, so everything outside [0, 2^31) selects nothing anyway: 0xFFFFFFFF
    r32 = torch.where((r64 < 0) | (r64 >= (1 << 31)), torch.full_like(r64, -1), r64).to(torch.int32)
    k_in = _aligned_copy(keys)
    off = _args.as_offsets(offsets)
    eng = _segmented_engine(*_args.device_and_stream(keys), name, False, bool(descending), n)
    if R <= SELECT_MAX_RANKS:
        r_in = r32.contiguous()
        eng.segmented_select(k_in.data_ptr(), n, off.data_ptr(), nseg, r_in.data_ptr(), R, values.data_ptr(), idx.data_ptr())
    else:
        for c in range(0, R, SELECT_MAX_RANKS):
            r_in = r32[:, c:c + SELECT_MAX_RANKS].contiguous()
            v_c = torch.zeros(r_in.shape, dtype=keys.dtype, device=keys.device)
            i_c = torch.full(r_in.shape, -1, dtype=torch.int32, device=keys.device)
            eng.segmented_select(k_in.data_ptr(), n, off.data_ptr(), nseg, r_in.data_ptr(), r_in.shape[1], v_c.data_ptr(), i_c.data_ptr())
            values[:, c:c + SELECT_MAX_RANKS] = v_c
            idx[:, c:c + SELECT_MAX_RANKS] = i_c
    eng.check_status()      # reports bad offsets of calls that have already finished
    return values, idx.to(torch.int64)      # uint32 positions below 2^31 (n <= 2^31): non-negative as int32


def select_ranks(size: int, k=None, q=None, interpolation: str = "linear"):
    """The rank arithmetic of kthvalue / median / quantile, as a pure function of the row length: (lo, hi, weight) such that the result
    is lerp(sorted[lo], sorted[hi], weight) on the ascending row.
      k given (1-based, torch.kthvalue): (k - 1, k - 1, None).
      neither k nor q (torch.median(x, dim), the lower median): ((size - 1) // 2, same, None).
      q given (a floating tensor of quantiles in [0, 1], any device; torch.quantile's arithmetic in q's dtype): pos = q * (size - 1);
        linear: lo = floor(pos), hi = ceil(pos), weight = pos - lo;  midpoint: the same ranks, weight 0.5;  lower / higher / nearest:
        lo = hi = floor / ceil / round-half-to-even of pos, weight None.  lo and hi are int64 tensors shaped like q, clamped to the row."""
    size = int(size)
    if size < 1:
        raise ValueError("select_ranks: the dimension must not be empty")
    if k is not None:
        k = int(k)
        if k < 1 or k > size:
            raise ValueError(f"kthvalue: k = {k} is out of range for a dimension of size {size}")
        return k - 1, k - 1, None
    if q is None:
        return (size - 1) // 2, (size - 1) // 2, None
    import torch
    if interpolation not in QUANTILE_MODES:
        raise ValueError(f"quantile: interpolation must be one of {QUANTILE_MODES}, not {interpolation!r}")
    pos = q * (size - 1)
    if interpolation == "lower":
        pos = pos.floor()
    elif interpolation == "higher":
        pos = pos.ceil()
    elif interpolation == "nearest":
        pos = pos.round()
    lo = pos.to(torch.int64).clamp(0, size - 1)
    if interpolation in ("lower", "higher", "nearest"):
        return lo, lo, None
    hi = pos.ceil().to(torch.int64).clamp(0, size - 1)
    weight = torch.full_like(pos, 0.5) if interpolation == "midpoint" else pos - lo
    return lo, hi, weight


def _select_along(what: str, x, dim: int, ranks):
    """x's rows along `dim` as segments of one segmented_select call each 8 ranks: `ranks` is a list of ints or an int64 tensor [R], the same
    for every row.  Returns (values, indices) shaped x.movedim(dim, -1).shape[:-1] + (R,), and the normalised dim."""
    import torch
    if not x.is_cuda:
        raise ValueError(f"{what}: x must be a device tensor")
    if _args.dtype_name(x) not in _KEY_DTYPES:
        raise TypeError(f"{what}: unsupported dtype {x.dtype}")
    if x.dim() == 0:
        x = x.reshape(1)
    dim = dim % x.dim()
    size = x.shape[dim]
    if size == 0:
        raise ValueError(f"{what}: dimension {dim} is empty")
    if not torch.is_tensor(ranks):
        ranks = torch.tensor(list(ranks), dtype=torch.int64).to(x.device, non_blocking=True)
    xm = x.movedim(dim, -1)
    rows = xm.numel() // size
    out_shape = xm.shape[:-1] + (ranks.numel(),)
    if rows == 0:
        return torch.empty(out_shape, dtype=x.dtype, device=x.device), torch.empty(out_shape, dtype=torch.int64, device=x.device), dim
    _args.check_count(what, "rsx_segmented_select", "elements", rows * size)
    flat = xm.contiguous().reshape(-1)
    offsets = torch.arange(0, rows + 1, device=x.device, dtype=torch.int64) * size
    v, i = segmented_select(flat, offsets, ranks.reshape(1, -1).expand(rows, -1), descending=False)
    return v.reshape(out_shape), i.reshape(out_shape), dim


def kthvalue(x, k: int, dim: int = -1, keepdim: bool = False):
    """torch.kthvalue(x, k, dim, keepdim) on a device tensor: (values, indices int64), the k-th smallest entry (k is 1-based) of every row
    along `dim`, by radix select in ONE rsx_segmented_select call — no sort, any k up to the row length.  Supported dtypes: int32, uint32,
    int64, uint64, float32, float64 (TypeError otherwise).  Two differences from torch: among equal values the index is the one a stable
    sort puts at rank k - 1 (torch leaves it unspecified); float keys follow IEEE 754 totalOrder, so +NaN is the largest key as in
    torch, but -0.0 < +0.0 and negative-sign NaNs rank below -inf."""
    scalar = x.dim() == 0
    size = 1 if scalar else x.shape[dim % x.dim()]
    r, _, _ = select_ranks(size, k=k) if x.is_cuda and size else (0, 0, None)
    v, i, dim = _select_along("kthvalue", x, dim, [r])
    if scalar:
        return v.reshape(()), i.reshape(())
    v, i = v.movedim(-1, dim), i.movedim(-1, dim)
    return (v, i) if keepdim else (v.squeeze(dim), i.squeeze(dim))


def median(x, dim: int = -1, keepdim: bool = False):
    """torch.median(x, dim, keepdim) on a device tensor: (values, indices int64), the lower median (rank (size - 1) // 2 of the ascending
    row) of every row along `dim`, by radix select in ONE rsx_segmented_select call.  Dtypes and the two differences from torch as
    kthvalue: tie indices are defined here (stable order); float keys follow totalOrder (+NaN largest as in torch, -0.0 < +0.0,
    negative-sign NaNs below -inf), so a row's median is NaN only if NaNs reach its middle rank — torch.median returns NaN for any row
    that holds one."""
    scalar = x.dim() == 0
    size = 1 if scalar else x.shape[dim % x.dim()]
    v, i, dim = _select_along("median", x, dim, [(size - 1) // 2 if size else 0])
    if scalar:
        return v.reshape(()), i.reshape(())
    v, i = v.movedim(-1, dim), i.movedim(-1, dim)
    return (v, i) if keepdim else (v.squeeze(dim), i.squeeze(dim))


def quantile(x, q, dim: int = -1, keepdim: bool = False, interpolation: str = "linear"):
    """torch.quantile(x, q, dim, keepdim, interpolation=...) on a float32 / float64 device tensor, by radix select: the ranks floor and
    ceil of q * (size - 1) of every row along `dim` go through one rsx_segmented_select call (8 ranks per call, i.e. 4 interpolated
    quantiles), and the result is torch.lerp(lo, hi, pos - floor(pos)) (midpoint: weight 0.5; lower / higher / nearest: one rank each,
    nearest rounding half to even as torch does).  q: a float, a sequence of floats or a 0-D / 1-D tensor in [0, 1] (a device tensor is
    not read back: its entries are clamped to the row instead of checked).  Shape as torch.quantile: a 1-D q comes first.
    Differences from torch: float keys follow IEEE 754 totalOrder (+NaN largest, -0.0 < +0.0, negative-sign NaNs below -inf) and NaN is
    not propagated — a row holding NaNs yields NaN only where a selected rank reaches them."""
    import torch
    if not x.is_cuda:
        raise ValueError("quantile: x must be a device tensor")
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"quantile: unsupported dtype {x.dtype} (float32 and float64)")
    if interpolation not in QUANTILE_MODES:
        raise ValueError(f"quantile: interpolation must be one of {QUANTILE_MODES}, not {interpolation!r}")
    if torch.is_tensor(q):
        if q.dim() > 1:
            raise ValueError("quantile: q must be a scalar or 1-D")
        if not q.is_cuda and q.numel() and not bool(((q >= 0) & (q <= 1)).all()):
            raise ValueError("quantile: q must be in [0, 1]")
        qt = q.to(device=x.device, dtype=x.dtype, non_blocking=True)
    else:
        ql = [float(v) for v in q] if isinstance(q, (list, tuple)) else float(q)
        if not all(0.0 <= v <= 1.0 for v in (ql if isinstance(ql, list) else [ql])):
            raise ValueError("quantile: q must be in [0, 1]")
        qt = torch.tensor(ql, dtype=x.dtype).to(x.device, non_blocking=True)
    scalar_q = qt.dim() == 0
    qt = qt.reshape(-1)
    nq = qt.numel()
    xs = x.reshape(1) if x.dim() == 0 else x
    d = dim % xs.dim()
    if xs.shape[d] == 0:
        raise ValueError(f"quantile: dimension {d} is empty")
    lo, hi, weight = select_ranks(xs.shape[d], q=qt, interpolation=interpolation)
    ranks = lo if weight is None else torch.cat([lo, hi])
    v, _, d = _select_along("quantile", xs, d, ranks)
    out = v[..., :nq] if weight is None else torch.lerp(v[..., :nq], v[..., nq:], weight)
    out = out.movedim(-1, 0)                       # [Q, rows...]
    if keepdim:
        out = out.unsqueeze(d + 1)
    if x.dim() == 0 and not keepdim:
        out = out.reshape(nq)
    return out[0] if scalar_q else out


# -- selection by mass on torch tensors: top-p cut-off, weighted quantiles ------------------------------------------------------------
WSELECT_MAX_TARGETS = 4    # rsx_segmented_weighted_select's bound per call; more targets are served in chunks


def _wselect_targets(what: str, targets, fractions, nseg: int, device):
    """Exactly one of targets (int64 masses) and fractions (float64): ([S, R] tensor, whether it holds fractions)."""
    import torch
    if (targets is None) == (fractions is None):
        raise ValueError(f"{what}: give exactly one of targets (int64 masses) and fractions (float64, of each segment's total mass)")
    t, want, word = (targets, torch.int64, "targets") if fractions is None else (fractions, torch.float64, "fractions")
    if not torch.is_tensor(t) or t.device != device or t.dtype != want or t.dim() not in (1, 2) or t.shape[0] != nseg:
        raise ValueError(f"{what}: {word} must be a {str(want).replace('torch.', '')} tensor [num_segments, R] or [num_segments] on the keys' device")
    return t.reshape(nseg, -1), fractions is not None


def segmented_weighted_select(keys, offsets, weights=None, targets=None, fractions=None, descending: bool = False, weight_exp: int = 0):
    """A select by MASS (rsx_segmented_weighted_select): for every segment [offsets[s], offsets[s+1]) of the 1-D device tensor `keys` and every
    target, the entry of the segment's stable sort (in the direction given) at which the running weight reaches the target — without
    sorting.  weights: a tensor like keys of float32 / float64 (a weight w > 0 weighs min(floor(w * 2^(31 - weight_exp)), 2^31) units of
    mass, NaN, negatives and zeros nothing; weights of 2^weight_exp or more saturate) or of int32 / uint32 (raw masses, i.e. frequency
    weights; weight_exp must be 0; int32 weights are meant to be non-negative, which is not checked — a check would synchronise — and a
    negative one is read as its uint32 bits, a mass near 2^32); None: the float keys are their own weights.  Exactly one of targets
    (int64, masses; not checked either: a negative target is read as its uint64 bits, which lie above every total and select nothing)
    and fractions (float64, of the segment's total mass: T = clamp(ceil(total * f), 1, total)) is given, shaped [S] or [S, R].
    Returns (values [S, R], index [S, R] int64 relative to the segment start, rank [S, R] int64 — rank + 1 elements are kept —, mass [S, R]
    int64 up to and including the answer, total [S] int64).  The answer is the smallest rank whose mass-so-far reaches the target; it
    always has positive mass, and among equal keys the mass advances in index order.  A target of 0 or above the total, a NaN fraction
    and a segment without mass select nothing: the slot holds value 0, index -1, rank -1 and mass 0.  All sums are 64-bit integer adds,
    so the result is bitwise reproducible.  More than 4 targets per segment take one engine call per 4.  Float keys follow IEEE 754
    totalOrder.  Bad offsets raise at the engine's next synchronisation (this call does not read them)."""
    import torch
    what = "segmented_weighted_select"
    name = _keys_and_offsets(what, keys, offsets)
    nseg = max(offsets.numel() - 1, 0)
    if weights is None:
        if name not in ("float32", "float64"):
            raise TypeError(f"{what}: without weights the keys are the weights, which takes float32 or float64 keys, not {keys.dtype}")
        kind = WEIGHT_FLOAT32 if name == "float32" else WEIGHT_FLOAT64
    else:
        if not torch.is_tensor(weights) or not weights.is_cuda or weights.device != keys.device or weights.shape != keys.shape:
            raise ValueError(f"{what}: weights must be a device tensor shaped like keys, on the same device")
        kind = _args.weight_kind(what, weights)
    weight_exp = int(weight_exp)
    if kind == WEIGHT_UINT32 and weight_exp != 0:
        raise ValueError(f"{what}: integer weights are masses themselves: weight_exp must be 0")
    tt, frac = _wselect_targets(what, targets, fractions, nseg, keys.device)
    R = tt.shape[1]
    n = keys.numel()
    values = torch.zeros((nseg, R), dtype=keys.dtype, device=keys.device)
    idx = torch.full((nseg, R), -1, dtype=torch.int32, device=keys.device)      # the uint32 outputs' bits: -1 marks an unwritten slot
    rank = torch.full((nseg, R), -1, dtype=torch.int32, device=keys.device)
    mass = torch.zeros((nseg, R), dtype=torch.int64, device=keys.device)
    total = torch.zeros((nseg,), dtype=torch.int64, device=keys.device)
    if n == 0 or nseg == 0 or R == 0:
        return values, idx.to(torch.int64), rank.to(torch.int64), mass, total
    k_in = _aligned_copy(keys)
    w_in = None if weights is None else _aligned_copy(weights)
    off = _args.as_offsets(offsets)
    flags = WSELECT_FRACTION if frac else 0
    eng = _segmented_engine(*_args.device_and_stream(keys), name, False, bool(descending), n)
    if R <= WSELECT_MAX_TARGETS:
        t_in = tt.contiguous()
        eng.segmented_weighted_select(k_in.data_ptr(), _args.ptr(w_in), n, off.data_ptr(), nseg, t_in.data_ptr(), R, flags, kind, weight_exp,
                                      values.data_ptr(), idx.data_ptr(), rank.data_ptr(), mass.data_ptr(), total.data_ptr())
    else:
        for c in range(0, R, WSELECT_MAX_TARGETS):
            t_in = tt[:, c:c + WSELECT_MAX_TARGETS].contiguous()
            v_c = torch.zeros(t_in.shape, dtype=keys.dtype, device=keys.device)
            i_c = torch.full(t_in.shape, -1, dtype=torch.int32, device=keys.device)
            r_c = torch.full(t_in.shape, -1, dtype=torch.int32, device=keys.device)
            m_c = torch.zeros(t_in.shape, dtype=torch.int64, device=keys.device)
            eng.segmented_weighted_select(k_in.data_ptr(), _args.ptr(w_in), n, off.data_ptr(), nseg, t_in.data_ptr(), t_in.shape[1], flags, kind,
                                          weight_exp, v_c.data_ptr(), i_c.data_ptr(), r_c.data_ptr(), m_c.data_ptr(), total.data_ptr())
            values[:, c:c + WSELECT_MAX_TARGETS] = v_c
            idx[:, c:c + WSELECT_MAX_TARGETS] = i_c
            rank[:, c:c + WSELECT_MAX_TARGETS] = r_c
            mass[:, c:c + WSELECT_MAX_TARGETS] = m_c
    eng.check_status()      # reports bad offsets of calls that have already finished
    return values, idx.to(torch.int64), rank.to(torch.int64), mass, total      # uint32 positions and ranks below 2^31: non-negative as int32


def _wselect_along(what: str, x, weights, dim: int, fr, descending: bool, weight_exp: int):
    """x's rows along `dim` as segments of one segmented_weighted_select call each 4 targets; fr(rows, shape of the rows) gives the float64
    fractions [rows, R].  Returns the five results with the rows' shape in front ([..., R], total [...]) and the normalised dim."""
    import torch
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError(f"{what}: x must be a device tensor")
    if _args.dtype_name(x) not in _KEY_DTYPES:
        raise TypeError(f"{what}: unsupported dtype {x.dtype}")
    if weights is not None:
        if not torch.is_tensor(weights) or not weights.is_cuda or weights.device != x.device or weights.shape != x.shape:
            raise ValueError(f"{what}: weights must be a device tensor shaped like x, on the same device")
        _args.weight_kind(what, weights)
    if x.dim() == 0:
        x = x.reshape(1)
        weights = None if weights is None else weights.reshape(1)
    dim = dim % x.dim()
    size = x.shape[dim]
    if size == 0:
        raise ValueError(f"{what}: dimension {dim} is empty")
    xm = x.movedim(dim, -1)
    lead = xm.shape[:-1]
    rows = xm.numel() // size
    f = fr(rows, lead)
    R = f.shape[1]
    if rows == 0:
        e = lambda dt, *tail: torch.empty(lead + tail, dtype=dt, device=x.device)
        return e(x.dtype, R), e(torch.int64, R), e(torch.int64, R), e(torch.int64, R), e(torch.int64), dim
    _args.check_count(what, "rsx_segmented_weighted_select", "elements", rows * size)
    flat = xm.contiguous().reshape(-1)
    wflat = None if weights is None else weights.movedim(dim, -1).contiguous().reshape(-1)
    offsets = torch.arange(0, rows + 1, device=x.device, dtype=torch.int64) * size
    v, i, r, m, t = segmented_weighted_select(flat, offsets, wflat, fractions=f, descending=descending, weight_exp=weight_exp)
    return v.reshape(lead + (R,)), i.reshape(lead + (R,)), r.reshape(lead + (R,)), m.reshape(lead + (R,)), t.reshape(lead), dim


def top_p(probs, p, dim: int = -1):
    """The top-p (nucleus) cut-off of every row of the float32 / float64 device tensor `probs` along `dim`, in ONE
    rsx_segmented_weighted_select call and without sorting: with the row in descending order (stable: equal probabilities in index
    order), the shortest prefix whose mass reaches p times the row's mass.  p: a float, or a tensor with one entry per row (probs' shape
    without `dim`).  Returns (threshold, count, kept), shaped like probs without `dim`: threshold is the smallest probability of the
    nucleus, count (int64) the number of entries in it (the answer's rank + 1) and kept (float64) their mass over the row's mass.
    The keys are their own weights with weight_exp = 0: a probability weighs floor(p * 2^31) units (1.0 and above: 2^31; NaN, zeros and
    negatives nothing), so one-hot rows are exact and sums are integers — bitwise reproducible.  p <= 0 gives the largest entry, p >= 1
    the whole support.  A row without mass, and a NaN p, give threshold 0, count 0 and kept NaN.
    The nucleus itself is compact_rows(probs, bound=threshold, descending=True): the probabilities at or above each row's threshold.
    Ties of the threshold beyond `count` come with it (count says how many entries the exact prefix has)."""
    import torch
    what = "top_p"
    if torch.is_tensor(probs) and probs.is_cuda and probs.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: unsupported dtype {probs.dtype} (float32 and float64)")

    def fr(rows, lead):
        if torch.is_tensor(p):
            if tuple(p.shape) != tuple(lead):
                raise ValueError(f"{what}: a tensor p must have one entry per row: shape {tuple(lead)}")
            return p.to(device=probs.device, dtype=torch.float64, non_blocking=True).reshape(rows, 1)
        return torch.full((rows, 1), float(p), dtype=torch.float64, device=probs.device)

    squeeze = torch.is_tensor(probs) and probs.dim() == 0
    v, _, r, m, t, _ = _wselect_along(what, probs, None, dim, fr, True, 0)
    kept = m[..., 0].to(torch.float64) / t.to(torch.float64)
    out = v[..., 0], r[..., 0] + 1, kept
    return tuple(o.reshape(()) for o in out) if squeeze else out


def _weight_exp_of(weight_max: float) -> int:
    """The smallest e with weight_max <= 2^e: the weights then use the 31 bits of the mass without saturating.  0 for a maximum that is
    not a positive finite number."""
    import math
    if not (weight_max > 0.0) or math.isinf(weight_max):
        return 0
    m, e = math.frexp(weight_max)           # weight_max = m * 2^e, 0.5 <= m < 1
    return e - 1 if m == 0.5 else e


def weighted_quantile(x, weights, q, dim: int = -1, weight_max=None):
    """The weighted quantiles of every row of the device tensor `x` along `dim`, without interpolation: the smallest x whose
    weight-so-far, in ascending stable order, reaches q times the row's weight (rsx_segmented_weighted_select, no sort).  weights: shaped
    like x; float32 / float64 (w > 0 weighs min(floor(w * 2^(31 - e)), 2^31), NaN, zeros and negatives nothing, with e the smallest
    exponent such that weight_max <= 2^e) or int32 / uint32 (exact frequency weights: the result is the plain quantile of x with every
    element repeated; int32 weights are meant to be non-negative, which is not checked: a negative one is read as its uint32 bits).  weight_max: an upper bound of the float weights; None reads weights.amax() back once — the one
    host synchronisation of this call (pass a bound to avoid it; weights above it saturate).  q: a float, or a sequence of floats (any
    number: one engine call per 4).  Returns (values, index int64): shaped like x without `dim` for a float q, with the quantiles in
    front ([Q, ...], as torch.quantile) for a sequence.  A row without weight, and a NaN q, give value 0 and index -1.  Supported
    dtypes of x: int32, uint32, int64, uint64, float32, float64."""
    import torch
    what = "weighted_quantile"
    scalar_q = not isinstance(q, (list, tuple))
    ql = [float(q)] if scalar_q else [float(v) for v in q]
    if not ql:
        raise ValueError(f"{what}: q must not be empty")
    wexp = 0
    if torch.is_tensor(weights) and weights.is_cuda and weights.is_floating_point() and weights.dtype in (torch.float32, torch.float64):
        if weight_max is None:
            weight_max = float(weights.amax().item()) if weights.numel() else 0.0
        wexp = _weight_exp_of(float(weight_max))

    def fr(rows, lead):
        return torch.tensor(ql, dtype=torch.float64).to(x.device, non_blocking=True).reshape(1, -1).expand(rows, -1)

    squeeze = torch.is_tensor(x) and x.dim() == 0
    v, i, _, _, _, _ = _wselect_along(what, x, weights, dim, fr, False, wexp)
    v, i = v.movedim(-1, 0), i.movedim(-1, 0)       # [Q, rows...]
    if squeeze:
        v, i = v.reshape(len(ql)), i.reshape(len(ql))
    return (v[0], i[0]) if scalar_q else (v, i)


def weighted_median(x, weights, dim: int = -1):
    """weighted_quantile(x, weights, 0.5, dim): the smallest x whose weight-so-far reaches half of the row's weight, and its index."""
    return weighted_quantile(x, weights, 0.5, dim=dim)


# -- unique on torch tensors ----------------------------------------------------------------------------------------------------------
def _unique_call(what: str, keys, offsets, want_inverse: bool, want_counts: bool, want_first: bool, descending: bool, consecutive: bool):
    """One rsx_segmented_unique call on a 1-D device tensor (offsets None: one segment).  Returns (values, run_offsets, inverse, counts,
    first) with the per-run tensors trimmed to run_offsets[-1] and None for what was not asked for."""
    import torch
    if not keys.is_cuda:
        raise ValueError(f"{what}: the input must be a device tensor (there is no CPU path)")
    name = _args.key_name(what, keys)
    n = keys.numel()
    _args.check_count(what, "rsx_segmented_unique", "elements", n)
    nseg = 1 if offsets is None else max(offsets.numel() - 1, 0)
    dev = keys.device
    run_offsets = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
    values = torch.empty(n, dtype=keys.dtype, device=dev)
    # the uint32 outputs as int32 tensors: positions and counts stay below 2^31 (n <= 2^31; a count of exactly 2^31 is masked below)
    inverse = torch.zeros(n, dtype=torch.int32, device=dev) if want_inverse else None
    counts = torch.empty(n, dtype=torch.int32, device=dev) if want_counts else None
    first = torch.empty(n, dtype=torch.int32, device=dev) if want_first else None
    total = 0
    if n > 0 and nseg > 0:
        k_in = _aligned_copy(keys)
        off = _args.as_offsets(offsets)
        positions = (want_inverse or want_first) and not consecutive         # only these travel through the sort as its payload
        eng = _segmented_engine(*_args.device_and_stream(keys), name, positions, bool(descending), n)
        eng.segmented_unique(k_in.data_ptr(), n, _args.ptr(off), nseg, values.data_ptr(), run_offsets.data_ptr(),
                             _args.ptr(counts), _args.ptr(first), _args.ptr(inverse), consecutive=consecutive)
        total = int(run_offsets[-1].item())         # the one read-back (a host synchronisation): how many runs there are
        eng.check_status()      # reports bad offsets (the call has finished)
    widen = _args.widen
    return values[:total], run_offsets, widen(inverse), widen(None if counts is None else counts[:total]), widen(None if first is None else first[:total])


def segmented_unique(keys, offsets, return_inverse: bool = False, return_counts: bool = False, return_first: bool = False, descending: bool = False,
                     consecutive: bool = False):
    """The distinct keys of every segment [offsets[s], offsets[s+1]) of the 1-D device tensor `keys` in ONE engine call
    (rsx_segmented_unique): returns (values, run_offsets, [inverse], [counts], [first]).  values holds the distinct keys of segment s,
    ascending (descending=True: descending), at [run_offsets[s], run_offsets[s+1]); counts and first (position of the key's first
    occurrence relative to the segment start) are indexed like values; inverse is shaped like keys, inverse[i] = index of keys[i] among
    its segment's distinct keys (0 outside [offsets[0], offsets[-1])).  All three are int64.  consecutive=True sorts nothing and collapses
    runs of adjacent equal keys instead (torch.unique_consecutive per segment).  Keys are distinct iff their bit patterns are: float keys
    follow IEEE 754 totalOrder, so -0.0 and +0.0 are two values and NaNs with equal bits are one (torch.unique merges the zeros and keeps
    every NaN apart).  values and the per-run outputs are trimmed to run_offsets[-1], which reads one int64 back: one host synchronisation
    per call, as torch.unique has.  Bad offsets raise RadixSortError."""
    if keys.dim() != 1:
        raise ValueError("segmented_unique: keys must be a 1-D device tensor")
    if not keys.is_cuda:
        raise ValueError("segmented_unique: keys must be a 1-D device tensor (there is no CPU path)")
    _args.check_offsets("segmented_unique", offsets, keys.device)
    v, ro, inv, cnt, fst = _unique_call("segmented_unique", keys, offsets, return_inverse, return_counts, return_first, descending, consecutive)
    return (v, ro) + ((inv,) if return_inverse else ()) + ((cnt,) if return_counts else ()) + ((fst,) if return_first else ())


def _unique_flat(what: str, x, return_inverse: bool, return_counts: bool, dim, consecutive: bool):
    if dim is not None:
        raise NotImplementedError(f"{what}: dim other than None (unique slices) is not implemented")
    flat = x.reshape(-1)
    v, _, inv, cnt, _ = _unique_call(what, flat, None, return_inverse, return_counts, False, False, consecutive)
    if not return_inverse and not return_counts:
        return v
    return (v,) + ((inv.reshape(x.shape),) if return_inverse else ()) + ((cnt,) if return_counts else ())


def unique(x, sorted: bool = True, return_inverse: bool = False, return_counts: bool = False, dim=None):
    """torch.unique(x, sorted, return_inverse, return_counts) of a device tensor, flattened, in ONE rsx_segmented_unique call (the flat sort
    chain, then the run detection): values ascending, inverse int64 shaped like x, counts int64.  sorted=False is accepted and sorts.
    dim other than None raises NotImplementedError.  Equal to torch for integer dtypes and for floats without -0.0 and NaN: here keys are
    distinct iff their bits are (IEEE 754 totalOrder: -0.0 and +0.0 are two values, equal-bit NaNs are one).  Reads the number of distinct
    values back: one host synchronisation, as torch.unique has.  Supported dtypes: int32, uint32, int64, uint64, float32, float64."""
    del sorted
    return _unique_flat("unique", x, return_inverse, return_counts, dim, False)


def unique_consecutive(x, return_inverse: bool = False, return_counts: bool = False, dim=None):
    """torch.unique_consecutive(x, return_inverse, return_counts) of a device tensor, flattened: runs of adjacent equal elements collapsed,
    nothing sorted (rsx_segmented_unique with RSX_UNIQUE_CONSECUTIVE).  Semantics, dtypes and the one host synchronisation as unique()."""
    return _unique_flat("unique_consecutive", x, return_inverse, return_counts, dim, True)


# -- reduce by key on torch tensors -----------------------------------------------------------------------------------------------------
_REDUCE_OPS = {"sum": REDUCE_SUM, "min": REDUCE_MIN, "max": REDUCE_MAX, "mean": REDUCE_SUM}
_VALUE_KINDS = _args.VALUE_KINDS    # dtype name -> value kind


def _reduce_call(what: str, keys, values, offsets, op: str, descending: bool, consecutive: bool):
    """One rsx_segmented_reduce_by_key call on 1-D device tensors (offsets None: one segment).  Returns (unique_keys, run_offsets, reduced,
    counts) with the per-run tensors trimmed to run_offsets[-1]; counts are always taken (mean needs them)."""
    import torch
    if op not in _REDUCE_OPS:
        raise ValueError(f"{what}: op must be one of 'sum', 'min', 'max', 'mean', not {op!r}")
    name = _args.key_name(what, keys)
    vkind = _args.value_kind(what, values)
    if op == "mean" and not values.dtype.is_floating_point:
        raise TypeError(f"{what}: the mean of integer values is not defined here (convert them to a float type)")
    if not keys.is_cuda or not values.is_cuda:
        raise ValueError(f"{what}: keys and values must be device tensors (there is no CPU path)")
    if values.shape != keys.shape or values.device != keys.device:
        raise ValueError(f"{what}: values must be shaped like keys and live on the same device")
    n = keys.numel()
    _args.check_count(what, "rsx_segmented_reduce_by_key", "elements", n)
    nseg = 1 if offsets is None else max(offsets.numel() - 1, 0)
    dev = keys.device
    run_offsets = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
    ukeys = torch.empty(n, dtype=keys.dtype, device=dev)
    reduced = torch.empty(n, dtype=values.dtype, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    total = 0
    if n > 0 and nseg > 0:
        k_in = _aligned_copy(keys)
        v_in = values.contiguous()
        off = _args.as_offsets(offsets)
        eng = _segmented_engine(*_args.device_and_stream(keys), name, not consecutive, bool(descending), n)      # the positions travel as the sort's payload
        eng.segmented_reduce_by_key(k_in.data_ptr(), v_in.data_ptr(), n, _args.ptr(off), nseg, _REDUCE_OPS[op], vkind, ukeys.data_ptr(),
                                    run_offsets.data_ptr(), reduced.data_ptr(), counts.data_ptr(), consecutive=consecutive)
        total = int(run_offsets[-1].item())         # the one read-back (a host synchronisation): how many runs there are
        eng.check_status()      # reports bad offsets (the call has finished)
    cnt = _args.widen(counts[:total])
    red = reduced[:total]
    if op == "mean":
        red = red / cnt.to(red.dtype)
    return ukeys[:total], run_offsets, red, cnt


def segmented_reduce_by_key(keys, values, offsets, op: str = "sum", descending: bool = False, consecutive: bool = False, return_counts: bool = False):
    """Per segment [offsets[s], offsets[s+1]) of the 1-D device tensors `keys` and `values`, in ONE engine call
    (rsx_segmented_reduce_by_key): returns (unique_keys, run_offsets, reduced[, counts]).  unique_keys and run_offsets are
    segmented_unique's; reduced[run_offsets[s] + u] is op ('sum', 'min', 'max' or 'mean') over the values whose key is that distinct key of
    segment s.  Values: int32, int64, float32, float64; integer sums wrap, float min / max return NaN if the run holds one, 'mean' (float
    values only) is the sum divided by the count.  Float sums are added in an order fixed by the input alone: the same call gives the same
    bits every time, which index_add_ does not.  consecutive=True sorts nothing and reduces the runs of adjacent equal keys.  Reads the
    number of runs back: one host synchronisation per call.  Bad offsets raise RadixSortError."""
    if keys.dim() != 1 or values.dim() != 1:
        raise ValueError("segmented_reduce_by_key: keys and values must be 1-D device tensors")
    _args.check_offsets("segmented_reduce_by_key", offsets, keys.device)
    k, ro, red, cnt = _reduce_call("segmented_reduce_by_key", keys, values, offsets, op, descending, consecutive)
    return (k, ro, red) + ((cnt,) if return_counts else ())


def reduce_by_key(keys, values, op: str = "sum", consecutive: bool = False, return_counts: bool = False):
    """The distinct elements of `keys` (flattened, ascending; consecutive=True: its runs of adjacent equal elements) and op over the
    elements of `values` (same shape, flattened) that came with each: (unique_keys, reduced[, counts]).  What
    torch.unique(return_inverse=True) followed by index_add_ / scatter_reduce_ computes, in one rsx_segmented_reduce_by_key call, without
    the inverse map and with float sums that are bitwise reproducible.  Ops, dtypes and the one host synchronisation as
    segmented_reduce_by_key."""
    if tuple(keys.shape) != tuple(values.shape):
        raise ValueError("reduce_by_key: keys and values must have the same shape")
    k, _, red, cnt = _reduce_call("reduce_by_key", keys.reshape(-1), values.reshape(-1), None, op, False, consecutive)
    return (k, red) + ((cnt,) if return_counts else ())


# -- scan on torch tensors --------------------------------------------------------------------------------------------------------------
_SCAN_OPS = {"sum": REDUCE_SUM, "min": REDUCE_MIN, "max": REDUCE_MAX}
# One small engine per (device, stream, key width): the scan uses none of an engine's capacity-sized buffers, so nobody allocates two sort
# buffers to take a prefix sum.  The stream is part of the key for the reason given at _SEG_ENGINES (the per-tile scratch serves one call).
_SCAN_ENGINES: dict = {}
_SCAN_ENGINE_CAPACITY = 1 << 12


def _scan_engine(device: int, stream: int, key_bytes: int) -> "Engine":
    return _cached_engine(_SCAN_ENGINES, (device, stream, key_bytes), "uint32" if key_bytes == 4 else "uint64", _SCAN_ENGINE_CAPACITY)


def _scan_call(what: str, keys, values, offsets, op: str, exclusive: bool, out):
    """One rsx_segmented_scan call on 1-D device tensors (keys None: segments only; offsets None: one segment)."""
    if op not in _SCAN_OPS:
        raise ValueError(f"{what}: op must be one of 'sum', 'min', 'max', not {op!r}")
    vkind = _args.value_kind(what, values)
    key_bytes = 4 if keys is None else _KEY_DTYPES[_args.key_name(what, keys)][0]
    if not values.is_cuda or (keys is not None and not keys.is_cuda):
        raise ValueError(f"{what}: keys and values must be device tensors (there is no CPU path)")
    if values.dim() != 1 or (keys is not None and (keys.shape != values.shape or keys.device != values.device)):
        raise ValueError(f"{what}: values must be 1-D, and keys shaped like them on the same device")
    _args.check_offsets(what, offsets, values.device, none_ok=True, whose="values'")
    if out is not None and (out.dtype != values.dtype or out.shape != values.shape or out.device != values.device or not out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous tensor like values (out=values scans in place)")
    n = values.numel()
    _args.check_count(what, "rsx_segmented_scan", "elements", n)
    in_place = out is not None and out.data_ptr() == values.data_ptr() and values.is_contiguous()
    v_in = values if values.is_contiguous() else values.contiguous()          # (aligned to its element size either way)
    if out is None:
        out = v_in.clone()                                                      # positions outside [offsets[0], offsets[-1]) keep the input
    elif not in_place:
        out.copy_(v_in)
    nseg = 1 if offsets is None else max(offsets.numel() - 1, 0)
    if n == 0 or nseg == 0:
        return out
    k_in = None if keys is None else _aligned_copy(keys)
    off = _args.as_offsets(offsets)
    eng = _scan_engine(*_args.device_and_stream(values), key_bytes)
    eng.segmented_scan(_args.ptr(k_in), out.data_ptr() if in_place else v_in.data_ptr(), n, _args.ptr(off), nseg, _SCAN_OPS[op], vkind,
                       out.data_ptr(), exclusive=bool(exclusive))
    eng.check_status()      # reports bad offsets of calls that have already finished; no synchronisation
    return out


def segmented_scan(values, offsets, op: str = "sum", exclusive: bool = False, keys=None, out=None):
    """The running op ('sum', 'min' or 'max') of the 1-D device tensor `values` inside every segment [offsets[s], offsets[s+1]) in ONE engine
    call (rsx_segmented_scan).  keys (optional, shaped like values): the scan also restarts wherever two adjacent keys differ by bits.
    exclusive=True folds the elements before each position only; a segment or run start then holds the identity (0, the largest or the
    smallest value of the dtype).  Returns a tensor like values; positions outside [offsets[0], offsets[-1]) keep their input value.
    out=values scans in place, any other out receives the result.  offsets None: one segment.  Values: int32, int64, float32, float64;
    integer sums wrap; a NaN poisons the rest of its run for float min / max.  Float sums are added in an order fixed by the input alone:
    the same call gives the same bits every time.  Never synchronises with the host; bad offsets (nothing is written then) raise
    RadixSortError at a later call or synchronisation of the engine."""
    return _scan_call("segmented_scan", keys, values, offsets, op, exclusive, out)


def scan_by_key(keys, values, op: str = "sum", exclusive: bool = False):
    """The running op of `values` inside every run of adjacent equal elements of `keys` (same shape, both flattened; equal by bits; nothing
    is sorted — sort first for a scan grouped by sorted keys): thrust's inclusive / exclusive_scan_by_key.  Returns a tensor shaped like
    values.  Ops, dtypes and reproducibility as segmented_scan."""
    if tuple(keys.shape) != tuple(values.shape):
        raise ValueError("scan_by_key: keys and values must have the same shape")
    return _scan_call("scan_by_key", keys.reshape(-1), values.reshape(-1), None, op, exclusive, None).reshape(values.shape)


def cumsum(x, dim: int = -1):
    """torch.cumsum(x, dim) on a device tensor: every row along `dim` is one segment of ONE rsx_segmented_scan call.  The result keeps
    x's dtype: an integer dtype narrower than int64 (int32 here) is NOT promoted to int64 as torch does, its sums wrap.  Float sums are
    bitwise reproducible (segmented_scan).  Supported dtypes: int32, int64, float32, float64 (TypeError otherwise)."""
    import torch
    if _args.dtype_name(x) not in _VALUE_KINDS:
        raise TypeError(f"cumsum: unsupported dtype {x.dtype} (int32, int64, float32 or float64)")
    if not x.is_cuda:
        raise ValueError("cumsum: x must be a device tensor")
    if x.dim() == 0:
        return x.clone()
    dim = dim % x.dim()
    size = x.shape[dim]
    xm = x.movedim(dim, -1)
    if x.numel() == 0:
        return x.clone()
    rows = xm.numel() // size
    flat = xm.contiguous().reshape(-1)
    if flat.data_ptr() == x.data_ptr():
        flat = flat.clone()                                                     # the scan runs in place on a tensor of our own
    offsets = None if rows == 1 else torch.arange(0, rows + 1, device=x.device, dtype=torch.int64) * size
    res = _scan_call("cumsum", None, flat, offsets, "sum", False, flat)
    return res.reshape(xm.shape).movedim(-1, dim)


# -- reduce on torch tensors ------------------------------------------------------------------------------------------------------------
_SEGREDUCE_OPS = {"sum": REDUCE_SUM, "min": REDUCE_MIN, "max": REDUCE_MAX, "mean": REDUCE_SUM, "argmin": REDUCE_ARGMIN, "argmax": REDUCE_ARGMAX}


def _segreduce_check(what: str, values, op: str) -> int:
    """the op, then the value type (its kind), then the device"""
    if op not in _SEGREDUCE_OPS:
        raise ValueError(f"{what}: op must be one of 'sum', 'min', 'max', 'mean', 'argmin', 'argmax', not {op!r}")
    vkind = _args.value_kind(what, values)
    if op == "mean" and not values.dtype.is_floating_point:
        raise TypeError(f"{what}: 'mean' needs float32 or float64 values, not {values.dtype}")
    if not values.is_cuda:
        raise ValueError(f"{what}: values must be a device tensor (there is no CPU path)")
    return vkind


def _segreduce_call(what: str, values, offsets, nseg: int, op: str, want_values: bool, want_index: bool):
    """One rsx_segmented_reduce call on a 1-D contiguous device tensor; offsets None: one segment.  Returns (values or None, the uint32
    indices viewed as int32, i.e. -1 for an empty segment, or None)."""
    import torch
    vkind = _segreduce_check(what, values, op)
    n = values.numel()
    _args.check_count(what, "rsx_segmented_reduce", "elements", n)
    dev = values.device
    code = _SEGREDUCE_OPS[op]
    if want_index and code == REDUCE_MIN:
        code = REDUCE_ARGMIN
    elif want_index and code == REDUCE_MAX:
        code = REDUCE_ARGMAX
    arg = code >= REDUCE_ARGMIN
    vout = torch.empty(nseg, dtype=values.dtype, device=dev) if want_values or not arg else None
    iout = torch.empty(nseg, dtype=torch.int32, device=dev) if arg else None
    if nseg == 0:
        return vout, iout
    off = _args.as_offsets(offsets)
    eng = _scan_engine(*_args.device_and_stream(values), 4)
    eng.segmented_reduce(_args.ptr_nonempty(values), n, _args.ptr(off), nseg, code, vkind, _args.ptr(vout), _args.ptr(iout))
    eng.check_status()      # reports bad offsets of calls that have already finished; no synchronisation
    return vout, iout


def segmented_reduce(values, offsets, op: str = "sum", return_index: bool = False):
    """op over every segment [offsets[s], offsets[s+1]) of the 1-D device tensor `values` in ONE engine call (rsx_segmented_reduce): a
    tensor of shape [S], one entry per segment id, empty segments included (0 for 'sum', the dtype's largest / smallest value or +inf /
    -inf for 'min' / 'max', NaN for 'mean').  ops: 'sum', 'min', 'max', 'mean' (sum / length on the device, float dtypes only), 'argmin',
    'argmax' (int64 positions inside the segment of the FIRST extreme, -1 for an empty segment; a NaN beats every number, as in torch).
    return_index=True, for 'min' and 'max', returns (values, indices).  Values: int32, int64, float32, float64; integer sums keep their
    dtype and wrap; float min / max give NaN if the segment holds one.  Float sums are added in an order fixed by the input alone: the same
    call gives the same bits every time.  Never synchronises with the host; bad offsets (nothing is written then) raise RadixSortError at
    a later call or synchronisation of the engine."""
    import torch
    _segreduce_check("segmented_reduce", values, op)
    if return_index and op not in ("min", "max"):
        raise ValueError("segmented_reduce: return_index goes with op 'min' or 'max'")
    if values.dim() != 1:
        raise ValueError("segmented_reduce: values must be 1-D")
    _args.check_offsets("segmented_reduce", offsets, values.device, whose="values'")
    nseg = max(offsets.numel() - 1, 0)
    v_in = values if values.is_contiguous() else values.contiguous()
    arg = op in ("argmin", "argmax")
    vout, iout = _segreduce_call("segmented_reduce", v_in, offsets, nseg, op, not arg, return_index)
    if op == "mean":
        return vout / (offsets[1:] - offsets[:-1]).to(vout.dtype)               # (0 / 0 = NaN for an empty segment)
    if arg:
        return iout.to(torch.int64)
    return (vout, iout.to(torch.int64)) if return_index else vout


def _reduce_along(what: str, x, op: str, dim: int, keepdim: bool, want_values: bool, want_index: bool):
    import torch
    _segreduce_check(what, x, op)
    if x.dim() == 0:
        raise ValueError(f"{what}: x must have at least one dimension")
    dim = dim % x.dim()
    size = x.shape[dim]
    if size == 0 and op not in ("sum", "mean"):
        raise ValueError(f"{what}: '{op}' over an empty dimension has no result")
    xm = x.movedim(dim, -1)
    shape = tuple(xm.shape[:-1])
    rows = 1
    for d in shape:
        rows *= d
    flat = xm.contiguous().reshape(-1)                                          # (a non-contiguous input is copied, as topk does)
    offsets = None if rows == 1 else torch.arange(0, rows + 1, device=x.device, dtype=torch.int64) * size
    vout, iout = _segreduce_call(what, flat, offsets, rows, op, want_values, want_index)

    def shaped(t):
        t = t.reshape(shape)
        return t.unsqueeze(dim) if keepdim else t

    if vout is not None and op == "mean":
        vout = vout / size
    return (None if vout is None else shaped(vout)), (None if iout is None else shaped(iout.to(torch.int64)))


def reduce_rows(x, op: str = "sum", dim: int = -1, keepdim: bool = False):
    """op ('sum', 'min', 'max', 'mean', 'argmin', 'argmax') along `dim` of a device tensor: the rows along `dim` are the segments of ONE
    rsx_segmented_reduce call.  The result has x's shape without `dim` (kept with size 1 if keepdim).  int32 sums stay int32 and wrap,
    as cumsum's do; dtypes and reproducibility as segmented_reduce."""
    arg = op in ("argmin", "argmax")
    vout, iout = _reduce_along("reduce_rows", x, op, dim, keepdim, not arg, False)
    return iout if arg else vout


def amax(x, dim: int = -1, keepdim: bool = False):
    """torch.amax(x, dim) on a device tensor, the rows in one call (reduce_rows)."""
    return _reduce_along("amax", x, "max", dim, keepdim, True, False)[0]


def amin(x, dim: int = -1, keepdim: bool = False):
    """torch.amin(x, dim) on a device tensor, the rows in one call (reduce_rows)."""
    return _reduce_along("amin", x, "min", dim, keepdim, True, False)[0]


def argmax(x, dim: int = -1, keepdim: bool = False):
    """torch.argmax(x, dim) on a device tensor: the first maximum of every row, a NaN beating every number."""
    return _reduce_along("argmax", x, "argmax", dim, keepdim, False, False)[1]


def argmin(x, dim: int = -1, keepdim: bool = False):
    """torch.argmin(x, dim) on a device tensor: the first minimum of every row, a NaN beating every number."""
    return _reduce_along("argmin", x, "argmin", dim, keepdim, False, False)[1]


# -- expand on torch tensors ------------------------------------------------------------------------------------------------------------
_EXPAND_VIEWS = {4: "int32", 8: "int64"}


def _expand_offsets(what: str, offsets, torch):
    if offsets is None or not hasattr(offsets, "is_cuda") or not offsets.is_cuda:
        raise ValueError(f"{what}: offsets must be a device tensor (there is no CPU path)")
    if offsets.dtype != torch.int64 or offsets.dim() != 1:
        raise ValueError(f"{what}: offsets must be a 1-D int64 device tensor")
    return _args.as_offsets(offsets)


def _expand_total(what: str, off, n):
    """The element count of the outputs: n as given (no synchronisation), else offsets[-1] read back once, as torch does."""
    if n is None:
        n = int(off[-1].item()) if off.numel() else 0
    n = int(n)
    if n < 0 or n > (1 << 31):
        raise ValueError(f"{what}: n must lie in [0, 2^31] (rsx_segmented_expand's bound)")
    return n


def _expand_call(what: str, off, n: int, values=None, starts=None, want_segment: bool = False, want_rank: bool = False, fill=None):
    """One rsx_segmented_expand call.  values: 1-D contiguous device tensor of 4- or 8-byte elements or None; returns (values_out or None,
    int32 segment ids or None, int32 ranks or None), each of n elements; positions outside [off[0], off[-1]) hold `fill` (default 0)."""
    import torch
    dev = off.device
    nseg = max(off.numel() - 1, 0)
    vout = sout = rout = None
    if values is not None:
        vout = torch.zeros(n, dtype=values.dtype, device=dev) if fill is None else torch.full((n,), fill, dtype=values.dtype, device=dev)
    if want_segment:
        sout = torch.zeros(n, dtype=torch.int32, device=dev)
    if want_rank:
        rout = torch.zeros(n, dtype=torch.int32, device=dev)
    if n and nseg:
        ptr = _args.ptr
        eng = _scan_engine(*_args.device_and_stream(off), 4)
        eng.segmented_expand(ptr(values), 0 if values is None else values.numel(), 4 if values is None else values.element_size(),
                             off.data_ptr(), nseg, n, ptr(starts), ptr(vout), ptr(sout), ptr(rout))
        eng.check_status()      # reports bad input of calls that have already finished; no synchronisation
    return vout, sout, rout


def _expand_values(what: str, off, n: int, values, starts, want_segment: bool, want_rank: bool):
    """values of any dtype and shape [num_values, ...]: 4- and 8-byte 1-D values go through the kernel, everything else expands indices
    (the kernel again) and uses torch.index_select."""
    import torch
    if not values.is_cuda or values.device != off.device:
        raise ValueError(f"{what}: values must be a device tensor on the offsets' device (there is no CPU path)")
    nseg = max(off.numel() - 1, 0)
    if starts is None and values.shape[0] != nseg:
        raise ValueError(f"{what}: the fill form has one value per segment ({nseg}), not {values.shape[0]}")
    if values.dim() == 1 and values.element_size() in _EXPAND_VIEWS and not values.is_complex():
        v = values if values.is_contiguous() else values.contiguous()
        if v.numel() == 0:
            v = torch.zeros(1, dtype=values.dtype, device=values.device)      # (nothing can be read from it: n or S is 0, or the starts are refused)
        vout, sout, rout = _expand_call(what, off, n, v, starts, want_segment, want_rank)
        return vout, sout, rout
    if starts is None:
        _, sout, rout = _expand_call(what, off, n, None, None, True, want_rank)
        return torch.index_select(values, 0, sout.to(torch.int64)), sout if want_segment else None, rout
    iota = torch.arange(values.shape[0], device=values.device, dtype=torch.int64)
    idx, sout, rout = _expand_call(what, off, n, iota, starts, want_segment, want_rank)
    return torch.index_select(values, 0, idx), sout, rout


def segmented_expand(offsets, values=None, n=None, starts=None, return_segment: bool = False, return_rank: bool = False):
    """From offsets back to elements in ONE engine call (rsx_segmented_expand).  For every position i of [offsets[0], offsets[-1]): the
    segment s(i) that owns it (the largest s with offsets[s] <= i, so empty segments own nothing), its rank i - offsets[s(i)], and, with
    `values`, values[s(i)] (one value per segment) or, with `starts` (int64, one per segment), values[starts[s(i)] + rank]: segment s is a
    copy of values[starts[s] : starts[s] + length].  Returns values[, segment][, rank] (just the ids and / or ranks without values; int64),
    each of n elements.  n is the length of the result: given, nothing synchronises with the host; None reads offsets[-1] back once.
    Positions outside [offsets[0], offsets[-1]) hold 0.  Bad offsets or starts (nothing is written then) raise RadixSortError at a later
    call or synchronisation of the engine."""
    import torch
    off = _expand_offsets("segmented_expand", offsets, torch)
    n = _expand_total("segmented_expand", off, n)
    st = None
    if starts is not None:
        if values is None:
            raise ValueError("segmented_expand: starts go with values")
        if not hasattr(starts, "is_cuda") or not starts.is_cuda or starts.dtype != torch.int64 or starts.dim() != 1 or starts.numel() != max(off.numel() - 1, 0) or starts.device != off.device:
            raise ValueError("segmented_expand: starts must be a 1-D int64 device tensor with one entry per segment")
        st = starts if starts.is_contiguous() else starts.contiguous()
    if values is None:
        if not (return_segment or return_rank):
            raise ValueError("segmented_expand: nothing to return (values, return_segment or return_rank)")
        _, sout, rout = _expand_call("segmented_expand", off, n, None, None, return_segment, return_rank)
        res = [t.to(torch.int64) for t in (sout, rout) if t is not None]
        return res[0] if len(res) == 1 else tuple(res)
    vout, sout, rout = _expand_values("segmented_expand", off, n, values, st, return_segment, return_rank)
    res = [vout] + [t.to(torch.int64) for t, w in ((sout, return_segment), (rout, return_rank)) if w]
    return res[0] if len(res) == 1 else tuple(res)


def segment_ids(offsets, n=None):
    """The segment id of every element (CSR -> COO): int64, n entries (None: offsets[-1], read back once)."""
    return segmented_expand(offsets, n=n, return_segment=True)


def segment_ranks(offsets, n=None):
    """The position of every element inside its segment: int64, n entries (None: offsets[-1], read back once)."""
    return segmented_expand(offsets, n=n, return_rank=True)


def broadcast_segments(per_segment, offsets, n=None):
    """The [S] result of segmented_reduce (or any tensor with one entry, or one row, per segment) spread over the segments' elements:
    out[i] = per_segment[s(i)], n entries (None: offsets[-1], read back once)."""
    import torch
    off = _expand_offsets("broadcast_segments", offsets, torch)
    n = _expand_total("broadcast_segments", off, n)
    return _expand_values("broadcast_segments", off, n, per_segment, None, False, False)[0]


def _offsets_of(what: str, lengths, torch):
    """[0, cumsum(lengths)] with the library's own scan, on int64; negative lengths make descending pairs, which the call reports."""
    if not hasattr(lengths, "is_cuda") or not lengths.is_cuda:
        raise ValueError(f"{what}: lengths must be a device tensor (there is no CPU path)")
    if lengths.dim() != 1 or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
        raise ValueError(f"{what}: lengths must be a 1-D integer tensor")
    off = torch.zeros(lengths.numel() + 1, dtype=torch.int64, device=lengths.device)
    if lengths.numel():
        off[1:] = lengths.to(torch.int64)
        off = _scan_call(what, None, off, None, "sum", False, off)
    return off


def repeat_interleave(x, repeats=None, dim=None, output_size=None):
    """torch.repeat_interleave in its three call forms: (repeats_tensor) -> the index i repeated repeats[i] times; (x, int) and
    (x, repeats_tensor), over the flattened x or along `dim`.  With output_size nothing synchronises with the host; without it the
    total is read back once, as torch does.  1-D values of 4 and 8 bytes go through rsx_segmented_expand itself; other dtypes, and `dim`
    on N-D input, expand indices and use torch.index_select.  An int `repeats` uses uniform offsets.  Negative repeats are reported as bad
    offsets at a later call or synchronisation of the engine."""
    import torch
    if not hasattr(x, "is_cuda") or not x.is_cuda:
        raise ValueError("repeat_interleave: x must be a device tensor (there is no CPU path)")
    if repeats is None:                                                          # form 1: x holds the repeats
        off = _offsets_of("repeat_interleave", x, torch)
        n = _expand_total("repeat_interleave", off, output_size)
        return _expand_call("repeat_interleave", off, n, None, None, True, False)[1].to(torch.int64)
    if dim is None:
        x = x.reshape(-1)
        dim = 0
    dim = dim % max(x.dim(), 1)
    if x.dim() == 0:
        x = x.reshape(1)
    size = x.shape[dim]
    if isinstance(repeats, int) or (hasattr(repeats, "dim") and repeats.dim() == 0 and not repeats.is_cuda):
        r = int(repeats)
        if r < 0:
            raise ValueError("repeat_interleave: repeats must not be negative")
        off = torch.arange(0, size + 1, device=x.device, dtype=torch.int64) * r
        n = size * r
        if output_size is not None and int(output_size) != n:
            raise ValueError("repeat_interleave: output_size does not match size * repeats")
    else:
        if not repeats.is_cuda:
            raise ValueError("repeat_interleave: repeats must be an int or a device tensor (there is no CPU path)")
        rep = repeats.reshape(-1)
        if rep.numel() == 1 and size != 1:
            rep = rep.expand(size)
        if rep.numel() != size:
            raise ValueError("repeat_interleave: repeats must have one entry per element along dim")
        off = _offsets_of("repeat_interleave", rep, torch)
        n = _expand_total("repeat_interleave", off, output_size)
    if x.dim() == 1:
        return _expand_values("repeat_interleave", off, n, x, None, False, False)[0]
    sout = _expand_call("repeat_interleave", off, n, None, None, True, False)[1]
    return torch.index_select(x, dim, sout.to(torch.int64))


def gather_ranges(src, starts, lengths):
    """The ragged slices src[starts[s] : starts[s] + lengths[s]] packed one behind the other: returns (values, offsets) with offsets =
    [0, cumsum(lengths)] (int64).  Slices may overlap and come in any order.  The total is read back once (the result's size)."""
    import torch
    off = _offsets_of("gather_ranges", lengths, torch)
    if not hasattr(starts, "is_cuda") or not starts.is_cuda or starts.dim() != 1 or starts.numel() != lengths.numel():
        raise ValueError("gather_ranges: starts must be a 1-D device tensor with one entry per slice")
    st = starts.to(torch.int64).contiguous()
    n = _expand_total("gather_ranges", off, None)
    flat = src if src.dim() >= 1 else src.reshape(1)
    return _expand_values("gather_ranges", off, n, flat, st, False, False)[0], off


def pack_rows(x, lengths):
    """A padded batch x of shape [B, W(, ...)] to ragged storage: row b contributes its first lengths[b] entries.  Returns (values,
    offsets); the slice of row b starts at b * W.  The total is read back once (the result's size)."""
    import torch
    if not hasattr(x, "is_cuda") or not x.is_cuda or x.dim() < 2:
        raise ValueError("pack_rows: x must be a device tensor of shape [B, W, ...]")
    B, W = x.shape[0], x.shape[1]
    if not hasattr(lengths, "numel") or lengths.numel() != B:
        raise ValueError("pack_rows: lengths must have one entry per row")
    starts = torch.arange(0, B, device=x.device, dtype=torch.int64) * W
    flat = (x if x.is_contiguous() else x.contiguous()).reshape((B * W,) + tuple(x.shape[2:]))
    return gather_ranges(flat, starts, lengths.reshape(-1))


def max_rows(x, dim: int = -1, keepdim: bool = False):
    """(values, indices) like torch.max(x, dim), in one call; the index is the FIRST maximum's."""
    return _reduce_along("max_rows", x, "max", dim, keepdim, True, True)


def min_rows(x, dim: int = -1, keepdim: bool = False):
    """(values, indices) like torch.min(x, dim), in one call; the index is the FIRST minimum's."""
    return _reduce_along("min_rows", x, "min", dim, keepdim, True, True)


# -- search on torch tensors ------------------------------------------------------------------------------------------------------------
# One small engine per (device, stream, dtype, direction): the search uses none of an engine's capacity-sized buffers, but its order map
# depends on key kind and direction, so the scan's engines (unsigned, ascending) cannot serve it.
_SEARCH_ENGINES: dict = {}


def _search_engine(device: int, stream: int, dtype_name: str, descending: bool) -> "Engine":
    return _cached_engine(_SEARCH_ENGINES, (device, stream, dtype_name, descending), dtype_name, _SCAN_ENGINE_CAPACITY, descending=descending)


def _search_call(what: str, hay, offsets, values, value_offsets, right: bool, descending: bool):
    """One rsx_segmented_search call on 1-D device tensors: the uint32 results as an int32 tensor of values.numel() entries (entries outside
    [value_offsets[0], value_offsets[-1]) are 0)."""
    import torch
    for name, t in (("the sorted keys", hay), ("values", values)):
        if not torch.is_tensor(t):
            raise TypeError(f"{what}: {name} must be a tensor")
    name = _args.key_name(what, hay)
    if values.dtype != hay.dtype:
        raise TypeError(f"{what}: values are {values.dtype}, the sorted keys {hay.dtype} (convert one of them: the search compares keys of one type)")
    if not hay.is_cuda or not values.is_cuda:
        raise ValueError(f"{what}: the sorted keys and the values must be device tensors (there is no CPU path)")
    if hay.dim() != 1 or values.dim() != 1 or values.device != hay.device:
        raise ValueError(f"{what}: the sorted keys and the values must be 1-D tensors on one device")
    _args.check_offsets(what, offsets, hay.device, none_ok=True)
    _args.check_offsets(what, value_offsets, hay.device, "value_offsets", none_ok=True)
    if value_offsets is not None and (offsets is None or value_offsets.numel() != offsets.numel()):
        raise ValueError(f"{what}: value_offsets needs offsets with the same number of entries")
    n, nq = hay.numel(), values.numel()
    _args.check_count(what, "rsx_segmented_search", "keys and 2^31 values", n, nq)
    nseg = 1 if offsets is None else max(offsets.numel() - 1, 0)
    if offsets is not None and value_offsets is None and nseg > 0 and nq % nseg != 0:
        raise ValueError(f"{what}: without value_offsets every segment has the same number of values, and {nq} is no multiple of {nseg} segments")
    out = torch.zeros(nq, dtype=torch.int32, device=hay.device)
    if nq == 0 or nseg == 0:
        return out
    k_in = _aligned_copy(hay)
    q_in = values if values.is_contiguous() else values.contiguous()          # (aligned to its element size either way)
    off, qoff = _args.as_offsets(offsets), _args.as_offsets(value_offsets)
    eng = _search_engine(*_args.device_and_stream(hay), name, bool(descending))
    eng.segmented_search(_args.ptr_nonempty(k_in), n, _args.ptr(off), nseg, q_in.data_ptr(), nq, _args.ptr(qoff), out.data_ptr(), right=bool(right))
    eng.check_status()      # reports bad offsets of calls that have already finished; no synchronisation
    return out


def segmented_searchsorted(sorted_keys, offsets, values, value_offsets=None, right: bool = False, descending: bool = False):
    """For every element of the 1-D device tensor `values`, where it would go in its segment of `sorted_keys` in ONE engine call
    (rsx_segmented_search): the number of keys of segment [offsets[s], offsets[s+1]) that come before it (right=True: that do not come
    after it), as int64 relative to offsets[s].  value_offsets (int64, like offsets): values[value_offsets[s] : value_offsets[s+1]] are
    searched in segment s; None: every segment has values.numel() / num_segments values.  The segments must be sorted as this library
    sorts them (segmented_sort / sort_rows with the same `descending`): floats in IEEE 754 totalOrder, -0.0 before +0.0, NaN an ordinary
    largest or smallest key.  values must have the keys' dtype.  Never synchronises with the host; bad offsets (nothing is written then)
    raise RadixSortError at a later call or synchronisation of the engine."""
    import torch
    if offsets is None:
        raise ValueError("segmented_searchsorted: offsets are required (searchsorted takes one segment)")
    if torch.is_tensor(values) and values.dim() != 1:
        raise ValueError("segmented_searchsorted: values must be a 1-D tensor")
    return _search_call("segmented_searchsorted", sorted_keys, offsets, values, value_offsets, right, descending).to(torch.int64).reshape(values.shape)


def _search_side(what: str, right: bool, side) -> bool:
    if side is None:
        return bool(right)
    if side not in ("left", "right"):
        raise ValueError(f"{what}: side must be 'left' or 'right', not {side!r}")
    if side == "left" and right:
        raise ValueError(f"{what}: side='left' conflicts with right=True")
    return side == "right"


def searchsorted(sorted_sequence, values, right: bool = False, side=None, out_int32: bool = False, descending: bool = False, sorter=None):
    """torch.searchsorted(sorted_sequence, values, right=right, side=side, out_int32=out_int32) on device tensors.  A 1-D sorted_sequence
    takes values of any shape (or a Python scalar); an N-D one takes values whose leading dimensions match, and its rows are the segments
    of ONE rsx_segmented_search call in the even form.  descending=True searches rows sorted in descending order.  Differences from torch:
    the rows must be in this library's order, which for floats is IEEE 754 totalOrder (what sort_rows returns): -0.0 sorts before +0.0
    and NaN is an ordinary largest or smallest key; values must have the sequence's dtype.  Integer dtypes, and floats without -0.0 and
    NaN, equal torch exactly.  sorter= is not implemented (sort first)."""
    import torch
    if sorter is not None:
        raise NotImplementedError("searchsorted: sorter= is not implemented; sort the sequence first (sort_rows / segmented_sort)")
    right = _search_side("searchsorted", right, side)
    if not torch.is_tensor(sorted_sequence):
        raise TypeError("searchsorted: sorted_sequence must be a tensor")
    if not torch.is_tensor(values):
        values = torch.tensor(values, dtype=sorted_sequence.dtype, device=sorted_sequence.device)
    seq = sorted_sequence
    if seq.dim() == 0:
        raise ValueError("searchsorted: sorted_sequence must have at least one dimension")
    if seq.dim() == 1:
        res = _search_call("searchsorted", seq, None, values.reshape(-1), None, right, descending).reshape(values.shape)
    else:
        if values.dim() != seq.dim() or tuple(values.shape[:-1]) != tuple(seq.shape[:-1]):
            raise ValueError("searchsorted: the leading dimensions of values must match those of an N-D sorted_sequence")
        cols = seq.shape[-1]
        rows = 1
        for d in seq.shape[:-1]:
            rows *= d
        offsets = torch.arange(0, rows + 1, device=seq.device, dtype=torch.int64) * cols
        res = _search_call("searchsorted", seq.contiguous().reshape(-1), offsets, values.contiguous().reshape(-1), None, right, descending).reshape(values.shape)
    return res if out_int32 else res.to(torch.int64)


def bucketize(input, boundaries, right: bool = False, out_int32: bool = False):
    """torch.bucketize(input, boundaries, right=right, out_int32=out_int32) on device tensors: for every element of `input` (any shape, or
    a Python scalar) its bucket among the 1-D ascending `boundaries`.  Order, dtypes and differences from torch as searchsorted."""
    import torch
    if torch.is_tensor(boundaries) and boundaries.dim() != 1:
        raise ValueError("bucketize: boundaries must be a 1-D tensor")
    return searchsorted(boundaries, input, right=right, out_int32=out_int32)


# -- compaction on torch tensors --------------------------------------------------------------------------------------------------------
def _compact_keys_check(what: str, keys) -> str:
    """the key type first (TypeError), then the device (ValueError): the name of the dtype"""
    import torch
    if not torch.is_tensor(keys):
        raise TypeError(f"{what}: the input must be a tensor")
    name = _args.key_name(what, keys)
    if not keys.is_cuda:
        raise ValueError(f"{what}: the input must be a device tensor (there is no CPU path)")
    return name


def _compact_call(what: str, keys, offsets, mask, bounds, strict: bool, invert: bool, descending: bool, partition: bool, want_keys: bool,
                  want_index: bool):
    """One rsx_segmented_compact call on a 1-D device tensor (offsets None: one segment).  Returns (values, kept_offsets, index): compact
    mode trims values and index to kept_offsets[-1] (ONE host synchronisation); partition mode returns them whole and reads nothing back."""
    import torch
    name = _compact_keys_check(what, keys)
    if (mask is None) == (bounds is None):
        raise ValueError(f"{what}: exactly one of mask and bound must be given")
    if mask is not None:
        if strict:
            raise ValueError(f"{what}: strict belongs to the bound form (a mask has no ties)")
        if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"{what}: the mask must be a torch.bool or torch.uint8 tensor")
        if mask.device != keys.device or mask.shape != keys.shape:
            raise ValueError(f"{what}: the mask must be on the keys' device and of the keys' shape")
    n = keys.numel()
    _args.check_count(what, "rsx_segmented_compact", "elements", n)
    nseg = 1 if offsets is None else max(offsets.numel() - 1, 0)
    if bounds is not None:
        if not torch.is_tensor(bounds) or bounds.dtype != keys.dtype:
            raise TypeError(f"{what}: the bound must be a tensor of the keys' dtype {keys.dtype}")
        if bounds.device != keys.device or bounds.numel() != nseg:
            raise ValueError(f"{what}: the bound must be on the keys' device and hold one key per segment ({nseg})")
    dev = keys.device
    kept = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
    # partition mode writes only [offsets[0], offsets[-1]): the rest of the outputs is the input's keys and zeros
    values = (keys.reshape(-1).clone() if partition else torch.empty(n, dtype=keys.dtype, device=dev)) if want_keys else None
    index = (torch.zeros if partition else torch.empty)(n, dtype=torch.int32, device=dev) if want_index else None
    total = n
    if n > 0 and nseg > 0:
        ptr = _args.ptr
        k_in = _aligned_copy(keys)
        off = _args.as_offsets(offsets)
        m_in = None if mask is None else mask if mask.is_contiguous() else mask.contiguous()
        b_in = None if bounds is None else bounds.contiguous().reshape(-1)
        eng = _search_engine(*_args.device_and_stream(keys), name, bool(descending))
        eng.segmented_compact(k_in.data_ptr(), n, ptr(off), nseg, ptr(m_in), ptr(b_in), ptr(values), ptr(index), kept.data_ptr(),
                              partition=partition, invert=invert, strict=strict)
        if not partition:
            total = int(kept[-1].item())            # the one read-back (a host synchronisation): how many were kept
        eng.check_status()      # reports bad offsets of calls that have already finished
    elif not partition:
        total = 0
    return (None if values is None else values[:total]), kept, _args.widen(None if index is None else index[:total])


def segmented_compact(keys, offsets, mask=None, bound=None, strict: bool = False, invert: bool = False, descending: bool = False,
                      partition: bool = False, return_index: bool = False):
    """Stream compaction of every segment [offsets[s], offsets[s+1]) of the 1-D device tensor `keys` in ONE engine call
    (rsx_segmented_compact): returns (values, kept_offsets, [index]).  mask (torch.bool / uint8, keys' shape): element i is kept iff
    mask[i] != 0.  bound (keys' dtype, one per segment): a key is kept iff it does not come after its segment's bound in this library's
    order - k <= bound ascending, k >= bound with descending=True; strict=True drops the ties; floats compare in IEEE 754 totalOrder
    (-0.0 before +0.0, NaN an ordinary largest or smallest key).  invert=True keeps what the predicate rejects.  values holds the kept
    keys of segment s, in input order, at [kept_offsets[s], kept_offsets[s+1]); index (int64) their positions relative to offsets[s].
    values and index are trimmed to kept_offsets[-1], which reads one int64 back: one host synchronisation per call.  partition=True
    drops nothing: values and index are shaped like keys, every segment holds its kept elements first and the others behind them, both in
    input order, kept_offsets[s+1] - kept_offsets[s] is the split of segment s, positions outside [offsets[0], offsets[-1]) hold the
    input's keys and index 0, and nothing is read back.  Bad offsets raise RadixSortError."""
    _compact_keys_check("segmented_compact", keys)
    if keys.dim() != 1:
        raise ValueError("segmented_compact: keys must be a 1-D device tensor")
    _args.check_offsets("segmented_compact", offsets, keys.device, none_ok=True, hint=" (or None: one segment)")
    v, ko, idx = _compact_call("segmented_compact", keys, offsets, mask, bound, strict, invert, descending, partition, True, return_index)
    return (v, ko) + ((idx,) if return_index else ())


def masked_select(x, mask):
    """torch.masked_select(x, mask) on device tensors: the elements of x where mask (torch.bool or uint8, broadcastable with x) is set,
    in row-major order, 1-D.  The call moves bits: NaNs and -0.0 come back as they went in.  One host synchronisation (the length)."""
    import torch
    if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError("masked_select: the mask must be a torch.bool or torch.uint8 tensor")
    _compact_keys_check("masked_select", x)
    if not mask.is_cuda:
        raise ValueError("masked_select: x and mask must be device tensors (there is no CPU path)")
    xb, mb = torch.broadcast_tensors(x, mask)
    v, _, _ = _compact_call("masked_select", xb.contiguous().reshape(-1), None, mb.contiguous().reshape(-1), None, False, False, False, False, True, False)
    return v


def nonzero(x, as_tuple: bool = False):
    """torch.nonzero(x, as_tuple=as_tuple) on a device tensor: the indices of the elements that differ from zero (-0.0 is zero, NaN is
    not), int64, in row-major order.  The mask x != 0 is compacted with positions only and the flat positions are unravelled on the
    device.  At most 2^31 elements.  One host synchronisation (the length)."""
    import torch
    if not torch.is_tensor(x):
        raise TypeError("nonzero: x must be a tensor")
    if not x.is_cuda:
        raise ValueError("nonzero: x must be a device tensor (there is no CPU path)")
    _args.check_count("nonzero", "rsx_segmented_compact", "elements", x.numel())
    flat_mask = (x != 0).contiguous().reshape(-1)
    # positions only: in mask form without a key output the call does not read the keys, so the (16-byte aligned) mask stands in for them
    flat_mask = _aligned_copy(flat_mask)
    idx = torch.empty(flat_mask.numel(), dtype=torch.int32, device=x.device)
    kept = torch.zeros(2, dtype=torch.int64, device=x.device)
    total = 0
    if flat_mask.numel() > 0:
        eng = _search_engine(*_args.device_and_stream(x), "uint32", False)
        eng.segmented_compact(flat_mask.data_ptr(), flat_mask.numel(), None, 1, flat_mask.data_ptr(), None, None, idx.data_ptr(), kept.data_ptr())
        total = int(kept[-1].item())                # the one read-back (a host synchronisation): how many there are
        eng.check_status()
    idx = _args.widen(idx[:total])
    cols = []
    rem = idx
    for size in reversed(x.shape):
        cols.append(rem % size)
        rem = torch.div(rem, size, rounding_mode="floor")
    cols.reverse()
    if as_tuple:
        return tuple(cols) if cols else (idx,)
    return torch.stack(cols, dim=1) if cols else idx.new_zeros((idx.numel(), 0))


def compact_rows(x, mask=None, bound=None, strict: bool = False, invert: bool = False, descending: bool = False, return_index: bool = False):
    """The ragged result of filtering a padded batch: the rows of x along its last dimension are the segments of ONE rsx_segmented_compact
    call.  mask: shaped like x (or broadcastable to it); bound: one key per row, shaped like x without its last dimension (or a scalar
    tensor for all rows).  Returns (values, row_offsets, [index]): row r's survivors are values[row_offsets[r] : row_offsets[r+1]], in
    input order; index (int64) their columns.  strict / invert / descending as segmented_compact."""
    import torch
    _compact_keys_check("compact_rows", x)
    if x.dim() == 0:
        raise ValueError("compact_rows: x must be a device tensor with at least one dimension")
    cols = x.shape[-1]
    rows = x.numel() // cols if cols else 0
    offsets = torch.arange(0, rows + 1, device=x.device, dtype=torch.int64) * cols
    flat = x.contiguous().reshape(-1)
    m = b = None
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError("compact_rows: the mask must be a torch.bool or torch.uint8 tensor")
        m = mask.expand(x.shape).contiguous().reshape(-1)
    if bound is not None:
        if not torch.is_tensor(bound):
            raise TypeError("compact_rows: the bound must be a tensor of x's dtype")
        b = bound.expand(x.shape[:-1]).contiguous().reshape(-1)
    v, ko, idx = _compact_call("compact_rows", flat, offsets, m, b, strict, invert, descending, False, True, return_index)
    return (v, ko) + ((idx,) if return_index else ())


# -- histograms on torch tensors --------------------------------------------------------------------------------------------------------
_INT_KEY_DTYPES = ("uint32", "int32", "uint64", "int64")
_HIST_MAX_COUNTERS = 1 << 31


def _hist_bins(what: str, keys, bins, lo, hi, width_shift: int):
    """The key and bin arguments that the histogram and the weighted histogram share, checked in one order: (dtype name, edges or None,
    B, lo, hi).  bins: an int (even form) or a 1-D tensor of B + 1 edges of the keys' dtype."""
    import torch
    name = _compact_keys_check(what, keys)
    edges = None
    if torch.is_tensor(bins):
        if bins.dtype != keys.dtype:
            raise TypeError(f"{what}: the edges are {bins.dtype}, the keys {keys.dtype} (convert one of them: the bins are compared as keys of one type)")
        if bins.dim() != 1 or bins.numel() < 2 or bins.device != keys.device:
            raise ValueError(f"{what}: the edges must be a 1-D tensor of at least 2 entries on the keys' device")
        if bins.numel() - 1 > 4096:
            raise ValueError(f"{what}: at most 4096 bins in the edges form (use searchsorted, then bincount)")
        if lo is not None or hi is not None or width_shift:
            raise ValueError(f"{what}: lo, hi and width_shift belong to the even form (bins an int)")
        edges = bins.contiguous()
        nb = edges.numel() - 1
    else:
        nb = int(bins)
        if nb < 1:
            raise ValueError(f"{what}: at least one bin")
        if name in _INT_KEY_DTYPES:
            if hi is not None:
                raise ValueError(f"{what}: hi belongs to float keys (integer keys: lo and width_shift)")
            lo = 0 if lo is None else lo
        elif lo is None or hi is None:
            raise ValueError(f"{what}: float keys need lo and hi in the even form")
    return name, edges, nb, lo, hi


def _hist_call(what: str, keys, offsets, nseg: int, bins, lo, hi, width_shift: int, descending: bool):
    """One rsx_segmented_histogram call on a 1-D device tensor (offsets None: one segment): the counters as an int64 tensor [nseg, B].
    bins: an int (even form) or a 1-D tensor of B + 1 edges of the keys' dtype.  Reads nothing back."""
    import torch
    name, edges, nb, lo, hi = _hist_bins(what, keys, bins, lo, hi, width_shift)
    n = keys.numel()
    if n > _args.MAX_ELEMENTS or nseg * nb > _HIST_MAX_COUNTERS:
        raise ValueError(f"{what}: at most 2^31 elements and 2^31 counters (rsx_segmented_histogram's bounds)")
    counts = torch.zeros((nseg, nb), dtype=torch.int32, device=keys.device)
    if nseg > 0:
        k_in = _aligned_copy(keys)
        off = _args.as_offsets(offsets)
        eng = _search_engine(*_args.device_and_stream(keys), name, bool(descending))
        eng.segmented_histogram(_args.ptr_nonempty(k_in), n, _args.ptr(off), nseg, nb, counts.data_ptr(), d_edges=_args.ptr(edges), lo=lo or 0,
                                hi=hi or 0, width_shift=int(width_shift))
        eng.check_status()      # reports bad offsets of calls that have already finished; no synchronisation
    return _args.widen(counts)


def segmented_histogram(keys, offsets, bins, lo=None, hi=None, width_shift: int = 0, descending: bool = False):
    """The keys of every segment [offsets[s], offsets[s+1]) of the 1-D device tensor `keys` counted per bin in ONE engine call
    (rsx_segmented_histogram): an int64 tensor [S, B].  bins a 1-D tensor of B + 1 edges of the keys' dtype, sorted in this library's
    order (floats: IEEE 754 totalOrder, -0.0 before +0.0; descending=True: descending), at most 4096 bins: numpy.histogram(x, bins=edges)
    per segment, the last bin closed on both sides.  bins an int: integer keys go to bin (k - lo) >> width_shift (lo defaults to 0),
    float keys to bin min(B - 1, floor((x - lo) * (B / (hi - lo)))) for lo <= x <= hi; descending=True numbers those bins backwards.
    Keys that fall into no bin are dropped.  offsets None: one segment.  Never synchronises with the host; bad offsets (all counters are
    zero then) raise RadixSortError at a later call or synchronisation of the engine."""
    _compact_keys_check("segmented_histogram", keys)
    if keys.dim() != 1:
        raise ValueError("segmented_histogram: keys must be a 1-D device tensor")
    _args.check_offsets("segmented_histogram", offsets, keys.device, none_ok=True, hint=" (or None: one segment)")
    nseg = 1 if offsets is None else max(offsets.numel() - 1, 0)
    return _hist_call("segmented_histogram", keys, offsets, nseg, bins, lo, hi, width_shift, descending)


_WHIST_MAX_SUMS = 1 << 30


def _whist_weight_type(what: str, weights) -> int:
    """the weights are a tensor of a weight dtype (TypeError, with _tensor_args' wording): the RSX_WEIGHT_* kind"""
    import torch
    if not torch.is_tensor(weights):
        raise TypeError(f"{what}: the weights must be a tensor")
    return _args.weight_kind(what, weights)


def _whist_scale(sums, k: int):
    """sums (int64) * 2^k as float64: one rounding, in the conversion, and only from 2^53 units on; the scaling is exact"""
    import math
    import torch
    out = sums.to(torch.float64)
    while k:
        step = max(min(k, 1000), -1000)
        out = out * math.ldexp(1.0, step)
        k -= step
    return out


def _whist_call(what: str, keys, offsets, nseg: int, weights, bins, lo, hi, width_shift: int, descending: bool, weight_max, signed: bool,
                return_mass: bool):
    """One rsx_segmented_weighted_histogram call on 1-D device tensors (offsets None: one segment): [nseg, B], float64 sums of the
    weights as quantised (mass * 2^(e - 31)), or the int64 masses (return_mass, and integer weights).  weight_max None reads the largest
    |weight| back once; otherwise nothing is read back."""
    import torch
    kind = _whist_weight_type(what, weights)
    name, edges, nb, lo, hi = _hist_bins(what, keys, bins, lo, hi, width_shift)
    if not weights.is_cuda or weights.device != keys.device:
        raise ValueError(f"{what}: the weights must be a device tensor on the keys' device (there is no CPU path)")
    if weights.shape != keys.shape:
        raise ValueError(f"{what}: the weights must be shaped like the keys: one weight per key")
    n = keys.numel()
    if n > _args.MAX_ELEMENTS or nseg * nb > _WHIST_MAX_SUMS:
        raise ValueError(f"{what}: at most 2^31 elements and 2^30 sums (rsx_segmented_weighted_histogram's bounds)")
    wexp, flags = 0, 0
    if kind != WEIGHT_UINT32:
        if weight_max is None:
            weight_max = float(weights.abs().amax().item()) if n else 0.0       # the one read-back
        wexp = _weight_exp_of(float(weight_max))
        flags = WHIST_SIGNED if signed else 0
    sums = torch.zeros((nseg, nb), dtype=torch.int64, device=keys.device)
    if nseg > 0 and n > 0:
        k_in = _aligned_copy(keys)
        w_in = weights.contiguous()
        off = _args.as_offsets(offsets)
        eng = _search_engine(*_args.device_and_stream(keys), name, bool(descending))
        eng.segmented_weighted_histogram(k_in.data_ptr(), w_in.data_ptr(), n, _args.ptr(off), nseg, nb, sums.data_ptr(), kind, wexp, flags,
                                         d_edges=_args.ptr(edges), lo=lo or 0, hi=hi or 0, width_shift=int(width_shift))
        eng.check_status()      # reports bad offsets of calls that have already finished; no synchronisation
    if return_mass or kind == WEIGHT_UINT32:
        return sums
    return _whist_scale(sums, wexp - 31)


def segmented_weighted_histogram(keys, offsets, weights, bins, lo=None, hi=None, width_shift: int = 0, descending: bool = False, weight_max=None,
                                 signed: bool = True, return_mass: bool = False):
    """The WEIGHTS of the keys of every segment [offsets[s], offsets[s+1]) of the 1-D device tensor `keys` summed per bin in ONE engine call
    (rsx_segmented_weighted_histogram), bitwise reproducibly: a tensor [S, B].  keys, offsets, bins, lo, hi, width_shift and descending
    are segmented_histogram's, and so is the bin of every key.  weights: a tensor shaped like keys.  float32 / float64: every weight
    is quantised once to an integer mass, floor(|w| * 2^(31 - e)) units with e the smallest exponent such that weight_max <= 2^e
    (weights beyond it saturate at 2^31 units; NaN weighs nothing), negated for a negative weight — signed=False: negative weights weigh
    nothing, the mass rule of segmented_weighted_select —, and the masses are added as 64-bit integers, in any order the same.  The result
    is float64, sum * 2^(e - 31): the sum of the weights as quantised, each within 2^(e - 31) of its value.  weight_max: an upper bound of
    |weights|; None reads weights.abs().amax() back once, the one host synchronisation of this call.  return_mass=True gives the int64
    masses themselves.  int32 (non-negative; not checked) / uint32 weights are masses as they stand: exact frequency weights, int64
    sums, `signed` does not apply.  Bad offsets (all sums are zero then) raise RadixSortError at a later call or synchronisation of the
    engine."""
    what = "segmented_weighted_histogram"
    _whist_weight_type(what, weights)
    _compact_keys_check(what, keys)
    if keys.dim() != 1:
        raise ValueError(f"{what}: keys must be a 1-D device tensor")
    _args.check_offsets(what, offsets, keys.device, none_ok=True, hint=" (or None: one segment)")
    nseg = 1 if offsets is None else max(offsets.numel() - 1, 0)
    return _whist_call(what, keys, offsets, nseg, weights, bins, lo, hi, width_shift, descending, weight_max, signed, return_mass)


def _hist_int_check(what: str, x) -> str:
    import torch
    if torch.is_tensor(x) and _args.dtype_name(x) not in _INT_KEY_DTYPES:
        raise TypeError(f"{what}: the input must be an integer tensor (int32, int64, uint32 or uint64), not {x.dtype}")
    return _compact_keys_check(what, x)


def bincount(x, minlength: int = 0, num_bins=None, *, weights=None, weight_max=None):
    """torch.bincount(x, minlength=minlength) on a 1-D integer device tensor: int64 counts of max(x) + 1 entries, at least
    minlength.  The length needs max(x): ONE read-back (Engine.key_range), as torch has one; negative values raise ValueError there.
    num_bins given: exactly max(num_bins, minlength) counters, values from there on and negative ones are dropped, and nothing is read
    back: no host synchronisation.  weights (a tensor shaped like x): torch.bincount(x, weights=weights) as a float64 tensor, bitwise
    reproducible — the signed form of segmented_weighted_histogram, which see for the quantisation and for weight_max (None: one more
    read-back); int32 / uint32 weights give int64 sums."""
    import torch
    wkind = None if weights is None else _whist_weight_type("bincount", weights)
    name = _hist_int_check("bincount", x)
    if x.dim() != 1:
        raise ValueError("bincount: x must be a 1-D device tensor")
    if minlength < 0:
        raise ValueError("bincount: minlength must be non-negative")
    if num_bins is not None:
        nb = max(int(num_bins), int(minlength))
    elif x.numel() == 0:
        nb = int(minlength)
    else:
        k_in = _aligned_copy(x)
        eng = _search_engine(*_args.device_and_stream(x), name, False)
        lo, hi = eng.key_range(k_in.data_ptr(), k_in.numel())          # of key ^ sign bit for signed keys: the one read-back
        sign = (1 << (8 * _KEY_DTYPES[name][0] - 1)) if _KEY_DTYPES[name][1] == KEY_SIGNED else 0
        if lo < sign:
            raise ValueError("bincount: the input holds negative values")
        nb = max(hi - sign + 1, int(minlength))
        x = k_in
    if nb == 0:
        return torch.zeros(0, dtype=torch.int64 if wkind in (None, WEIGHT_UINT32) else torch.float64, device=x.device)
    if nb > _HIST_MAX_COUNTERS:
        raise ValueError("bincount: at most 2^31 bins (rsx_segmented_histogram's bound)")
    if weights is not None:
        return _whist_call("bincount", x, None, 1, weights, nb, 0, None, 0, False, weight_max, True, False).reshape(-1)
    return _hist_call("bincount", x, None, 1, nb, 0, None, 0, False).reshape(-1)


def bincount_rows(ids, num_bins: int, *, weights=None, weight_max=None):
    """bincount of every row of the integer device tensor `ids` along its last dimension, in ONE rsx_segmented_histogram call: int64
    counts [..., num_bins]; ids outside [0, num_bins) are dropped.  No host synchronisation.  (torch.bincount is 1-D only.)  weights (a
    tensor shaped like ids, e.g. a router's gate values): the weights of every row summed per id in ONE
    rsx_segmented_weighted_histogram call, float64, bitwise reproducible (the signed form of segmented_weighted_histogram; weight_max
    None: one read-back; int32 / uint32 weights: int64 sums)."""
    import torch
    if weights is not None:
        _whist_weight_type("bincount_rows", weights)
    _hist_int_check("bincount_rows", ids)
    if ids.dim() == 0:
        raise ValueError("bincount_rows: ids must be a device tensor with at least one dimension")
    cols = ids.shape[-1]
    rows = ids.numel() // cols if cols else int(np.prod(ids.shape[:-1], dtype=np.int64))
    offsets = torch.arange(0, rows + 1, device=ids.device, dtype=torch.int64) * cols
    if weights is not None:
        if not weights.is_cuda or weights.shape != ids.shape:
            raise ValueError("bincount_rows: the weights must be a device tensor shaped like ids")
        res = _whist_call("bincount_rows", ids.contiguous().reshape(-1), offsets, rows, weights.contiguous().reshape(-1), int(num_bins), 0, None, 0, False,
                          weight_max, True, False)
    else:
        res = _hist_call("bincount_rows", ids.contiguous().reshape(-1), offsets, rows, int(num_bins), 0, None, 0, False)
    return res.reshape(tuple(ids.shape[:-1]) + (int(num_bins),))


def _hist_float_range(what: str, x, lo, hi):
    """(lo, hi) of an even float histogram: the caller's, or - lo == hi - the data's range (ONE read-back; torch.aminmax, because
    Engine.key_range refuses float engines), widened by 1 either side when empty: torch.histc's rule."""
    import torch
    lo, hi = float(lo), float(hi)
    if lo == hi and x.numel() > 0:
        mn, mx = torch.aminmax(x)
        lo, hi = float(mn), float(mx)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"{what}: the range [{lo}, {hi}] is not finite")
    if lo > hi:
        raise ValueError(f"{what}: max must be larger than min")
    if lo == hi:
        lo, hi = lo - 1.0, hi + 1.0
    return lo, hi


def _hist_float_check(what: str, x) -> str:
    import torch
    if torch.is_tensor(x) and x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: the input must be a float32 or float64 tensor, not {x.dtype}")
    return _compact_keys_check(what, x)


def histc(x, bins: int = 100, min=0, max=0):
    """torch.histc(x, bins=bins, min=min, max=max) on a float32 / float64 device tensor of any shape: the counts of `bins` equal-width
    bins over [min, max] as a tensor of x's dtype; elements outside the range and NaNs are dropped; min == max takes the data's range (one
    read-back).  The bin of x is min(bins - 1, floor((x - min) * (bins / (max - min)))), each operation rounded once in x's precision:
    for values and ranges that are exact in that arithmetic this is torch's result; elsewhere the two may differ in a few bins, as
    torch and numpy do."""
    import torch
    _hist_float_check("histc", x)
    lo, hi = _hist_float_range("histc", x, min, max)
    return _hist_call("histc", x.contiguous().reshape(-1), None, 1, int(bins), lo, hi, 0, False).reshape(-1).to(x.dtype)


def _whist_flat(what: str, x, weight):
    """the weights of a wrapper that flattens x, flattened alike"""
    if not weight.is_cuda or weight.shape != x.shape:
        raise ValueError(f"{what}: the weights must be a device tensor shaped like the input")
    return weight.contiguous().reshape(-1)


def histogram(x, bins, range=None, *, weight=None, weight_max=None):
    """torch.histogram(x, bins, range=range) without density on a device tensor: (counts int64, bin_edges).  bins a 1-D tensor
    of edges of x's dtype (any of the six key dtypes; ascending in this library's order; at most 4096 bins): numpy.histogram(x,
    bins=edges).  bins an int (float dtypes): equal-width bins over range = (lo, hi), or over the data's range (one read-back);
    bin_edges = torch.linspace(lo, hi, bins + 1); the bin arithmetic is histc's.  weight (a tensor shaped like x): the first result is
    the sum of the weights per bin, float64 and bitwise reproducible, as numpy.histogram(x, bins, weights=weight) — the signed form of
    segmented_weighted_histogram, which see for the quantisation and for weight_max (None: one read-back); int32 / uint32 weights give
    int64 sums."""
    import torch
    if weight is not None:
        _whist_weight_type("histogram", weight)
    if torch.is_tensor(bins):
        _compact_keys_check("histogram", x)
        if range is not None:
            raise ValueError("histogram: range belongs to an int bins")
        if weight is not None:
            w = _whist_flat("histogram", x, weight)
            return _whist_call("histogram", x.contiguous().reshape(-1), None, 1, w, bins, None, None, 0, False, weight_max, True, False).reshape(-1), bins
        return _hist_call("histogram", x.contiguous().reshape(-1), None, 1, bins, None, None, 0, False).reshape(-1), bins
    _hist_float_check("histogram", x)
    lo, hi = _hist_float_range("histogram", x, *(range if range is not None else (0, 0)))
    if weight is not None:
        w = _whist_flat("histogram", x, weight)
        counts = _whist_call("histogram", x.contiguous().reshape(-1), None, 1, w, int(bins), lo, hi, 0, False, weight_max, True, False).reshape(-1)
    else:
        counts = _hist_call("histogram", x.contiguous().reshape(-1), None, 1, int(bins), lo, hi, 0, False).reshape(-1)
    return counts, torch.linspace(lo, hi, int(bins) + 1, dtype=x.dtype, device=x.device)


def histogram_rows(x, bins, range=None, *, weight=None, weight_max=None):
    """histogram of every row of the device tensor x along its last dimension, in ONE rsx_segmented_histogram call: (counts int64
    [..., B], bin_edges).  bins and range as histogram; the edges or the range are shared by all rows (an int bins without a range takes
    the range of the whole tensor).  weight (a tensor shaped like x): the sums of the weights per row and bin, as histogram's."""
    import torch
    if weight is not None:
        _whist_weight_type("histogram_rows", weight)
    if x.dim() == 0:
        raise ValueError("histogram_rows: x must be a device tensor with at least one dimension")
    if torch.is_tensor(bins):
        _compact_keys_check("histogram_rows", x)
        if range is not None:
            raise ValueError("histogram_rows: range belongs to an int bins")
        lo = hi = None
        edges, nb = bins, bins.numel() - 1
    else:
        _hist_float_check("histogram_rows", x)
        lo, hi = _hist_float_range("histogram_rows", x, *(range if range is not None else (0, 0)))
        nb = int(bins)
        edges = torch.linspace(lo, hi, nb + 1, dtype=x.dtype, device=x.device)
    cols = x.shape[-1]
    rows = x.numel() // cols if cols else int(np.prod(x.shape[:-1], dtype=np.int64))
    offsets = torch.arange(0, rows + 1, device=x.device, dtype=torch.int64) * cols
    if weight is not None:
        res = _whist_call("histogram_rows", x.contiguous().reshape(-1), offsets, rows, _whist_flat("histogram_rows", x, weight),
                          bins if torch.is_tensor(bins) else nb, lo, hi, 0, False, weight_max, True, False)
    else:
        res = _hist_call("histogram_rows", x.contiguous().reshape(-1), offsets, rows, bins if torch.is_tensor(bins) else nb, lo, hi, 0, False)
    return res.reshape(tuple(x.shape[:-1]) + (nb,)), edges


# -- categorical draws on torch tensors ---------------------------------------------------------------------------------------------------
def _sample_weights_check(what: str, weights, word: str = "weights") -> int:
    """the weight type first (TypeError), then the device (ValueError): the RSX_WEIGHT_* kind"""
    import torch
    if not torch.is_tensor(weights):
        raise TypeError(f"{what}: {word} must be a tensor")
    kind = _args.weight_kind(what, weights)
    if not weights.is_cuda:
        raise ValueError(f"{what}: {word} must be a device tensor (there is no CPU path)")
    return kind


def _sample_targets(what: str, u, targets, nseg: int, device):
    """Exactly one of u (float64 uniforms; float32 is widened) and targets (int64 / uint64 masses): ([S, R] 8-byte tensor, whether it
    holds fractions, whether the caller's was 1-D)."""
    import torch
    if (u is None) == (targets is None):
        raise ValueError(f"{what}: give exactly one of u (float64 uniforms in [0, 1)) and targets (int64 masses)")
    t, word = (targets, "targets") if u is None else (u, "u")
    if not torch.is_tensor(t) or not t.is_cuda or t.device != device:
        raise ValueError(f"{what}: {word} must be a device tensor on the weights' device (there is no CPU path)")
    words = (torch.float32, torch.float64) if u is not None else (torch.int64, getattr(torch, "uint64", torch.int64))
    if t.dtype not in words:
        raise TypeError(f"{what}: {word} must be {'float64 (or float32)' if u is not None else 'int64 / uint64 masses'}, not {t.dtype}")
    if t.dim() not in (1, 2) or t.shape[0] != nseg:
        raise ValueError(f"{what}: {word} must be shaped [num_segments, R] or [num_segments]")
    if t.dtype == torch.float32:
        t = t.to(torch.float64)
    return t.reshape(nseg, -1).contiguous(), u is not None, t.dim() == 1


def segmented_sample(weights, offsets, u=None, targets=None, keys=None, bound=None, strict: bool = False, invert: bool = False,
                     descending: bool = False, weight_exp: int = 0):
    """Categorical draws from every segment [offsets[s], offsets[s+1]) of the 1-D device tensor `weights` in ONE engine call
    (rsx_segmented_sample), bitwise reproducibly and without sorting: element i of a segment, in input order, is drawn with probability
    mass_i / total.  weights: float32 / float64 (a weight w > 0 weighs min(floor(w * 2^(31 - weight_exp)), 2^31) units, NaN, negatives
    and zeros nothing) or int32 / uint32 (raw masses; weight_exp must be 0) — segmented_weighted_select's rule.  Exactly one of u
    (float64 uniforms, float32 is widened: T = clamp(ceil(total * u), 1, total)) and targets (int64 / uint64 masses T) is given, shaped
    [S, R] or [S]; the answer is the smallest i whose running mass reaches T.  bound (one key per segment): an element that
    segmented_compact's predicate rejects weighs nothing — a key is kept iff it does not come after the bound (k <= bound ascending,
    k >= bound with descending=True; strict drops the ties, invert flips; every tie of the bound is treated alike).  The keys the bound
    is compared with are `keys` (a tensor like weights of a key dtype), or with keys=None the float weights themselves.  Returns
    (index, mass, total): index int64 [S, R] (or [S] for 1-D u / targets) relative to the segment start, -1 where nothing was drawn
    (T == 0, T > total, NaN u, a segment without mass); mass int64, the running mass up to and including the answer (0 where nothing was
    drawn); total int64 [S].  offsets None: one segment.  No host synchronisation; bad offsets raise RadixSortError at a later call or
    synchronisation of the engine."""
    import torch
    what = "segmented_sample"
    kind = _sample_weights_check(what, weights)
    if weights.dim() != 1:
        raise ValueError(f"{what}: weights must be a 1-D device tensor")
    _args.check_offsets(what, offsets, weights.device, none_ok=True, whose="weights'", hint=" (or None: one segment)")
    nseg = 1 if offsets is None else max(offsets.numel() - 1, 0)
    weight_exp = int(weight_exp)
    if kind == WEIGHT_UINT32 and weight_exp != 0:
        raise ValueError(f"{what}: integer weights are masses themselves: weight_exp must be 0")
    if bound is None:
        if keys is not None:
            raise ValueError(f"{what}: keys are compared with the bound only: give a bound, or no keys")
        if strict or invert:
            raise ValueError(f"{what}: strict and invert belong to the bound")
        key_name = None
    else:
        ktensor = weights if keys is None else keys
        if keys is None and kind == WEIGHT_UINT32:
            raise TypeError(f"{what}: without keys the weights are the keys the bound is compared with, which takes float32 or float64 weights, not {weights.dtype}")
        if keys is not None:
            if not torch.is_tensor(keys):
                raise TypeError(f"{what}: keys must be a tensor")
            _args.key_name(what, keys)
            if not keys.is_cuda or keys.device != weights.device or keys.shape != weights.shape:
                raise ValueError(f"{what}: keys must be a device tensor shaped like weights, on the same device")
        key_name = _args.key_name(what, ktensor)
        if not torch.is_tensor(bound) or bound.dtype != ktensor.dtype:
            raise TypeError(f"{what}: the bound must be a tensor of the keys' dtype {ktensor.dtype}")
        if bound.device != weights.device or bound.numel() != nseg:
            raise ValueError(f"{what}: the bound must be on the weights' device and hold one key per segment ({nseg})")
    tt, frac, flat = _sample_targets(what, u, targets, nseg, weights.device)
    R = tt.shape[1]
    n = weights.numel()
    _args.check_count(what, "rsx_segmented_sample", "elements and draws", n, nseg * R)
    dev = weights.device
    idx = torch.full((nseg, R), -1, dtype=torch.int32, device=dev)          # the uint32 output's bits: -1 marks an unwritten slot
    mass = torch.zeros((nseg, R), dtype=torch.int64, device=dev)
    total = torch.zeros((nseg,), dtype=torch.int64, device=dev)
    if n > 0 and nseg > 0 and R > 0:
        ptr = _args.ptr
        self_weights = bound is not None and keys is None
        w_in = _aligned_copy(weights) if self_weights else weights.contiguous()
        k_in = w_in if self_weights else None if keys is None else _aligned_copy(keys)
        b_in = None if bound is None else bound.contiguous().reshape(-1)
        off = _args.as_offsets(offsets)
        flags = (WSELECT_FRACTION if frac else 0) | (COMPACT_STRICT if strict else 0) | (COMPACT_INVERT if invert else 0)
        eng = _search_engine(*_args.device_and_stream(weights), key_name or "uint32", bool(descending) if key_name else False)
        eng.segmented_sample(ptr(k_in), None if self_weights else w_in.data_ptr(), n, ptr(off), nseg, ptr(b_in), tt.data_ptr(), R, flags, kind, weight_exp,
                             idx.data_ptr(), mass.data_ptr(), total.data_ptr())
        eng.check_status()      # reports bad offsets of calls that have already finished; no synchronisation
    idx = idx.to(torch.int64)                                                # (positions below 2^31: non-negative as int32)
    return (idx.reshape(nseg), mass.reshape(nseg), total) if flat else (idx, mass, total)


def _sample_uniforms(what: str, u, shape, device, generator):
    import torch
    if u is None:
        return torch.rand(shape, dtype=torch.float64, device=device, generator=generator)
    if not torch.is_tensor(u) or not u.is_cuda or u.device != device:
        raise ValueError(f"{what}: u must be a device tensor on probs' device (there is no CPU path)")
    if u.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: u must be float64 (or float32), not {u.dtype}")
    if tuple(u.shape) != tuple(shape):
        raise ValueError(f"{what}: u must be shaped {tuple(shape)}: one uniform per draw")
    return u


def multinomial(probs, num_samples: int, dim: int = -1, u=None, generator=None, weight_max=None):
    """torch.multinomial(probs, num_samples, replacement=True) on a device tensor, for the rows along `dim` in ONE rsx_segmented_sample
    call: int64 [..., num_samples], the drawn positions along `dim`.  The draws are WITH replacement (replacement=False is not offered).
    u: the uniforms in [0, 1), float64 shaped like the result; None draws them with torch.rand(..., dtype=float64, generator=generator).
    Given u the result is a pure function of (probs, u): equal bits on every run, stream and engine, which torch's float prefix sums do
    not promise.  Weights are quantised once to integer masses: a weight w weighs floor(w * 2^(31 - e)) units with e the smallest
    exponent such that weight_max <= 2^e.  weight_max=None assumes PROBABILITIES (e = 0): weights above 1 then saturate at 2^31 units
    and are drawn as if they were 1 — pass an upper bound of the weights for unnormalised ones; nothing is read back to find one.
    Weights below 2^(e - 31) weigh nothing.  A row without mass gives -1 where torch raises.  dtypes: float32, float64 (int32 / uint32
    are masses as they stand).  No host synchronisation."""
    import torch
    what = "multinomial"
    kind = _sample_weights_check(what, probs, "probs")
    num_samples = int(num_samples)
    if num_samples < 1:
        raise ValueError(f"{what}: num_samples must be at least 1")
    if probs.dim() == 0:
        raise ValueError(f"{what}: probs must have at least one dimension")
    dim = dim % probs.dim()
    pm = probs.movedim(dim, -1)
    lead, size = tuple(pm.shape[:-1]), pm.shape[-1]
    rows = int(np.prod(lead, dtype=np.int64))
    uu = _sample_uniforms(what, u, lead + (num_samples,), probs.device, generator)
    if rows == 0 or size == 0:
        return torch.full(lead + (num_samples,), -1, dtype=torch.int64, device=probs.device)
    wexp = 0 if weight_max is None or kind == WEIGHT_UINT32 else _weight_exp_of(float(weight_max))
    offsets = torch.arange(0, rows + 1, device=probs.device, dtype=torch.int64) * size
    idx, _, _ = segmented_sample(pm.contiguous().reshape(-1), offsets, u=uu.reshape(rows, num_samples), weight_exp=wexp)
    return idx.reshape(lead + (num_samples,))


def sample_rows(probs, u=None, top_k=None, top_p=None, min_p=None, generator=None):
    """One token per row of the float32 / float64 device tensor `probs` (rows along the last dimension), drawn with probability
    proportional to its entry among the entries that pass the filters given: int64, probs' shape without its last dimension.
    Every threshold is taken from the UNFILTERED row by the existing calls — top_p: the nucleus threshold of top_p(probs, top_p); top_k:
    the k-th largest value (kthvalue); min_p: min_p * amax(row) — and the row's bound is the largest of those given.  Then ONE
    rsx_segmented_sample call draws among the entries >= bound, the probabilities being their own weights (weight_exp = 0: an entry
    weighs floor(p * 2^31) units).  Nothing is written out, sorted or read back: no host synchronisation.  u: float64 uniforms, one per
    row; None draws them with torch.rand(..., dtype=float64, generator=generator).  Given u the result is bitwise reproducible.
    Two differences from sequential filtering with renormalisation (the order of Hugging Face's logits warpers: top-k, then top-p of the
    renormalised survivors, then min-p): (1) each filter sees the whole row, so top_p=0.9 after top_k keeps the nucleus of the ORIGINAL
    distribution cut at the k-th value — the intersection of the filters — where the sequential order keeps 90 % of the top-k mass;
    (2) every entry that ties with the bound is kept, as compact_rows does, so more than k entries pass top_k when the k-th value
    repeats.  Renormalisation itself is implied: the draw is proportional among the survivors.  A row without mass gives -1."""
    import torch
    what = "sample_rows"
    if torch.is_tensor(probs) and _args.weight_kind(what, probs) == WEIGHT_UINT32:
        raise TypeError(f"{what}: unsupported dtype {probs.dtype} (float32 and float64)")
    _sample_weights_check(what, probs, "probs")
    if probs.dim() == 0:
        raise ValueError(f"{what}: probs must have at least one dimension")
    lead, size = tuple(probs.shape[:-1]), probs.shape[-1]
    rows = int(np.prod(lead, dtype=np.int64))
    uu = _sample_uniforms(what, u, lead, probs.device, generator)
    if rows == 0 or size == 0:
        return torch.full(lead, -1, dtype=torch.int64, device=probs.device)
    bound = None
    if top_p is not None:
        bound = globals()["top_p"](probs, top_p, dim=-1)[0]
    if top_k is not None:
        k = int(top_k)
        if k < 1:
            raise ValueError(f"{what}: top_k must be at least 1")
        kth = kthvalue(probs, size - min(k, size) + 1, dim=-1)[0]
        bound = kth if bound is None else torch.maximum(bound, kth)
    if min_p is not None:
        floor = amax(probs, dim=-1) * min_p
        bound = floor if bound is None else torch.maximum(bound, floor)
    offsets = torch.arange(0, rows + 1, device=probs.device, dtype=torch.int64) * size
    flat = probs.contiguous().reshape(-1)
    if bound is None:
        idx, _, _ = segmented_sample(flat, offsets, u=uu.reshape(rows))
    else:
        idx, _, _ = segmented_sample(flat, offsets, u=uu.reshape(rows), bound=bound.to(probs.dtype).reshape(rows), descending=True)
    return idx.reshape(lead)


# -- ranks on torch tensors -------------------------------------------------------------------------------------------------------------
def _rank_check(what: str, x, method) -> int:
    """The method's code and the rules of the input that need no device: an unknown method and a host tensor raise ValueError, a dtype
    that is no key type (bfloat16, float16, bool, ...) TypeError."""
    code = RANK_METHODS.get(method) if isinstance(method, str) else None
    if code is None:
        raise ValueError(f"{what}: method must be one of {', '.join(RANK_METHODS)}, not {method!r}")
    _args.key_name(what, x)
    if not x.is_cuda:
        raise ValueError(f"{what}: the input must be a device tensor (there is no CPU path)")
    return code


def _rank_call(what: str, keys, offsets, nseg: int, code: int, descending: bool, want_ties: bool):
    """One rsx_segmented_rank call on a 1-D device tensor (offsets None: one segment).  Returns (ranks, ties) as int32 tensors holding the
    uint32 results (below 2^32: min + max of 2^31 keys), zero outside the segments; nothing is read back."""
    import torch
    n = keys.numel()
    _args.check_count(what, "rsx_segmented_rank", "elements", n)
    ranks = torch.zeros(n, dtype=torch.int32, device=keys.device)
    ties = torch.zeros(n, dtype=torch.int32, device=keys.device) if want_ties else None
    if n > 0 and nseg > 0:
        k_in = _aligned_copy(keys)
        off = _args.as_offsets(offsets)
        eng = _segmented_engine(*_args.device_and_stream(keys), _args.dtype_name(keys), True, bool(descending), n)
        eng.segmented_rank(k_in.data_ptr(), n, _args.ptr(off), nseg, code, ranks.data_ptr(), _args.ptr(ties))
        eng.check_status()      # reports bad offsets of calls that have already finished
    return ranks, ties


def _rank_result(ranks, code: int):
    """int64 ranks; float64 (min + max) / 2 for the average"""
    import torch
    wide = _args.widen(ranks)
    return wide.to(torch.float64) / 2 if code == RANK_AVERAGE else wide


def segmented_rank(keys, offsets, method: str = "average", descending: bool = False, return_ties: bool = False):
    """The 0-based rank of every key inside its segment [offsets[s], offsets[s+1]) of the 1-D device tensor `keys` in ONE engine call
    (rsx_segmented_rank).  method: "ordinal" (the position in the segment's stable sort), "min", "max" (the first / last position of the
    key's tie group), "dense" (the distinct keys before it) or "average" ((min + max) / 2).  Returns ranks shaped like keys, int64, for
    "average" float64; with return_ties also the int64 size of every key's tie group.  Entries outside [offsets[0], offsets[-1]) are 0.
    descending=True ranks the largest key 0.  Keys tie iff their bits are equal: float keys follow IEEE 754 totalOrder, so -0.0 ranks
    below +0.0 and NaNs rank by sign and payload.  Bad offsets raise at the engine's next synchronisation (this call does not read
    them); nothing is written then."""
    code = _rank_check("segmented_rank", keys, method)
    if keys.dim() != 1:
        raise ValueError("segmented_rank: keys must be a 1-D device tensor")
    _args.check_offsets("segmented_rank", offsets, keys.device)
    ranks, ties = _rank_call("segmented_rank", keys, offsets, max(offsets.numel() - 1, 0), code, descending, return_ties)
    out = _rank_result(ranks, code)
    return (out, _args.widen(ties)) if return_ties else out


def rankdata(x, method: str = "average", dim=-1, descending: bool = False, pct: bool = False):
    """scipy.stats.rankdata(x, method, axis=dim) on a device tensor: 1-based ranks shaped like x, float64 for "average" and int64
    otherwise; the rows along `dim` are the segments of ONE rsx_segmented_rank call, dim=None ranks the flattened tensor (the flat sort
    chain).  pct=True divides by the row length (float64), as pandas' rank(pct=True).  descending=True ranks the largest entry first.
    Equal to scipy for integers and for floats without -0.0 and NaN.  Differences: keys tie iff their bits are equal and float keys
    follow IEEE 754 totalOrder, so -0.0 ranks below +0.0 (scipy ties them), and NaNs rank by sign and payload, equal-bit NaNs tying
    (scipy's default propagates NaN to the whole row).  Supported dtypes: int32, uint32, int64, uint64, float32, float64."""
    import torch
    code = _rank_check("rankdata", x, method)
    if dim is None:
        flat = x.reshape(-1)
        size = flat.numel()
        ranks, _ = _rank_call("rankdata", flat, None, 1, code, descending, False)
        out = _rank_result(ranks, code).reshape(x.shape) + 1
    else:
        if x.dim() == 0:
            raise ValueError("rankdata: a 0-d tensor has no dimension to rank along (dim=None ranks it flattened)")
        dim = dim % x.dim()
        size = x.shape[dim]
        xm = x.movedim(dim, -1)
        rows = xm.numel() // size if size else 0
        flat = xm.contiguous().reshape(-1)
        offsets = torch.arange(0, rows + 1, device=x.device, dtype=torch.int64) * size
        ranks, _ = _rank_call("rankdata", flat, offsets, rows, code, descending, False)
        out = (_rank_result(ranks, code) + 1).reshape(xm.shape).movedim(-1, dim)
    if pct:
        # (by a device scalar: a true IEEE division; torch multiplies by the reciprocal of a host scalar, which is not the same number)
        out = out.to(torch.float64) / torch.full((), float(max(size, 1)), dtype=torch.float64, device=x.device)
    return out


# -- merge on torch tensors -------------------------------------------------------------------------------------------------------------
def _merge_call(what: str, a, a_offsets, b, b_offsets, payload_a, payload_b, descending: bool, want_index: bool):
    """One rsx_segmented_merge call on 1-D device tensors (both offsets None: one segment).  Returns (keys, out_offsets, payload, index):
    keys, payload and index have na + nb entries, zero (index: -1) from out_offsets[-1] on; nothing is read back."""
    import torch
    name = _args.pair_key_name(what, a, b, "the merge compares keys of one type")
    nseg = _args.check_pair(what, a, b, a_offsets, b_offsets)
    _args.check_pair_payloads(what, a, b, payload_a, payload_b)
    na, nb = a.numel(), b.numel()
    _args.check_count(what, "rsx_segmented_merge", "keys together", na + nb)
    dev = a.device
    keys = torch.zeros(na + nb, dtype=a.dtype, device=dev)
    ooff = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
    pay = None if payload_a is None else torch.zeros(na + nb, dtype=payload_a.dtype, device=dev)
    index = torch.full((na + nb,), -1, dtype=torch.int32, device=dev) if want_index else None
    if na + nb > 0 and nseg > 0:
        ptr, cont = _args.ptr_nonempty, _args.as_offsets
        a_in, b_in = _aligned_copy(a), _aligned_copy(b)
        ao, bo, pa, pb = cont(a_offsets), cont(b_offsets), cont(payload_a), cont(payload_b)
        eng = _search_engine(*_args.device_and_stream(a), name, bool(descending))
        if pay is not None:             # (an empty side has no storage: any aligned address stands in for its payload, which is not read)
            pa_ptr, pb_ptr = (pa.data_ptr() if na else pay.data_ptr() + 4 * (na + nb)), (pb.data_ptr() if nb else pay.data_ptr() + 4 * (na + nb))
        else:
            pa_ptr = pb_ptr = None
        eng.segmented_merge(ptr(a_in), na, ptr(ao), ptr(b_in), nb, ptr(bo), nseg, keys.data_ptr(), ptr(index), ooff.data_ptr(),
                            d_a_payload=pa_ptr, d_b_payload=pb_ptr, d_payload_out=ptr(pay))
        eng.check_status()      # reports bad offsets of calls that have already finished; no synchronisation
    return keys, ooff, pay, (None if index is None else index.to(torch.int64))


def segmented_merge(a, a_offsets, b, b_offsets, payload_a=None, payload_b=None, descending: bool = False, return_index: bool = False):
    """The stable merge of sorted segment a[a_offsets[s] : a_offsets[s+1]] with sorted segment b[b_offsets[s] : b_offsets[s+1]], for every
    s, in ONE engine call (rsx_segmented_merge) that reads every key once: returns (keys, out_offsets[, payload][, index]).  a and b are
    1-D device tensors of one dtype, the offsets int64 (both None: one segment each).  out_offsets[s] = (a_offsets[s] - a_offsets[0]) +
    (b_offsets[s] - b_offsets[0]); keys[out_offsets[s] : out_offsets[s+1]] is the stable sort of the concatenation of the two segments in
    this library's order: equal keys keep the order of their side and those of a come before those of b.  The segments must be sorted as
    this library sorts them (segmented_sort / sort_rows with the same `descending`): floats in IEEE 754 totalOrder, -0.0 before +0.0, NaN an
    ordinary largest or smallest key; inputs that are not sorted give an unspecified order.  payload_a / payload_b (int32 / uint32, both
    or neither): the word that came with each key.  index (int64): the position of every output in the concatenation of its two segments
    (below the a segment's length: from a).  The outputs have a.numel() + b.numel() entries and are zero (index: -1) from out_offsets[-1]
    on.  Never synchronises with the host; bad offsets raise RadixSortError at a later call or synchronisation of the engine."""
    k, oo, p, idx = _merge_call("segmented_merge", a, a_offsets, b, b_offsets, payload_a, payload_b, descending, return_index)
    return (k, oo) + ((p,) if p is not None else ()) + ((idx,) if return_index else ())


def _pair_rows(what: str, a, b, payload_a=None, payload_b=None):
    """The rows of two tensors with equal leading shape as the segments of a call with two sides: (a, a_offsets, b, b_offsets, payload_a,
    payload_b), all flattened; 1-D inputs are one segment (offsets None)."""
    import torch
    for name, t in (("a", a), ("b", b)):
        if not torch.is_tensor(t):
            raise TypeError(f"{what}: {name} must be a tensor")
    if a.dim() == 0 or a.dim() != b.dim() or tuple(a.shape[:-1]) != tuple(b.shape[:-1]):
        raise ValueError(f"{what}: a and b must have the same number of dimensions (at least one) and equal leading shape")
    for pname, p, k in (("payload_a", payload_a, a), ("payload_b", payload_b, b)):
        if p is not None and (not torch.is_tensor(p) or p.shape != k.shape):
            raise ValueError(f"{what}: {pname} must be a tensor shaped like its keys")
    la, lb = a.shape[-1], b.shape[-1]
    flat = lambda t: None if t is None else t.contiguous().reshape(-1)
    ao = bo = None
    if a.dim() > 1:
        rows = a.numel() // la if la else (b.numel() // lb if lb else 0)
        steps = torch.arange(0, rows + 1, device=a.device, dtype=torch.int64)
        ao, bo = steps * la, steps * lb
    return flat(a), ao, flat(b), bo, flat(payload_a), flat(payload_b)


def merge(a, b, payload_a=None, payload_b=None, descending: bool = False, return_index: bool = False):
    """The stable merge of two sorted device tensors along their last dimension: 1-D inputs are one segment; N-D inputs with equal leading
    shape are merged row by row, the rows being the segments of ONE rsx_segmented_merge call.  Returns keys of shape [..., La + Lb]
    (with payloads: (keys, payload); with return_index=True the int64 positions in torch.cat([a, b], -1) of every output last).  Equal to
    torch.sort(torch.cat([a, b], -1), dim=-1, stable=True, descending=descending) for rows sorted in this library's order (integer dtypes,
    and floats without -0.0 and NaN, equal torch exactly).  Order, payloads and errors as segmented_merge."""
    k, _, p, idx = _merge_call("merge", *_pair_rows("merge", a, b, payload_a, payload_b), descending, return_index)
    shape = tuple(a.shape[:-1]) + (a.shape[-1] + b.shape[-1],)
    res = (k.reshape(shape),) + ((p.reshape(shape),) if p is not None else ()) + ((idx.reshape(shape),) if return_index else ())
    return res[0] if len(res) == 1 else res


# -- set operations on torch tensors ----------------------------------------------------------------------------------------------------
_SET_OPS = {"intersection": SET_INTERSECTION, "difference": SET_DIFFERENCE, "union": SET_UNION, "symmetric_difference": SET_SYMMETRIC_DIFFERENCE}


def _set_op_code(what: str, op) -> int:
    if isinstance(op, str) and op in _SET_OPS:
        return _SET_OPS[op]
    if isinstance(op, int) and not isinstance(op, bool) and 0 <= op <= 3:
        return op
    raise ValueError(f"{what}: unknown op {op!r} (one of {', '.join(_SET_OPS)}, or SET_INTERSECTION .. SET_SYMMETRIC_DIFFERENCE)")


def _setop_call(what: str, a, a_offsets, b, b_offsets, op, payload_a, payload_b, descending: bool, want_index: bool, want_match: bool):
    """One rsx_segmented_set_op call on 1-D device tensors (both offsets None: one segment).  Returns (keys, out_offsets, payload, index,
    match), trimmed to out_offsets[-1] (ONE host synchronisation)."""
    import torch
    name = _args.pair_key_name(what, a, b, "a set operation compares keys of one type")
    code = _set_op_code(what, op)
    if want_match and code != SET_INTERSECTION:
        raise ValueError(f"{what}: return_match belongs to the intersection (no other op pairs its outputs with b)")
    nseg = _args.check_pair(what, a, b, a_offsets, b_offsets)
    _args.check_pair_payloads(what, a, b, payload_a, payload_b)
    na, nb = a.numel(), b.numel()
    _args.check_count(what, "rsx_segmented_set_op", "keys together", na + nb)
    cap = na if code in (SET_INTERSECTION, SET_DIFFERENCE) else na + nb
    dev = a.device
    keys = torch.empty(cap, dtype=a.dtype, device=dev)
    koff = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
    pay = None if payload_a is None else torch.empty(cap, dtype=payload_a.dtype, device=dev)
    index = torch.empty(cap, dtype=torch.int32, device=dev) if want_index else None
    match = torch.empty(cap, dtype=torch.int32, device=dev) if want_match else None
    total = 0
    if na + nb > 0 and nseg > 0:
        ptr, cont = _args.ptr_nonempty, _args.as_offsets
        a_in, b_in = _aligned_copy(a), _aligned_copy(b)
        ao, bo, pa, pb = cont(a_offsets), cont(b_offsets), cont(payload_a), cont(payload_b)
        eng = _search_engine(*_args.device_and_stream(a), name, bool(descending))
        spare = None
        if pay is not None:             # (an empty side or an empty output has no storage: a spare word stands in; it is neither read nor written)
            spare = torch.empty(4, dtype=torch.int32, device=dev)
            pa_ptr, pb_ptr, po_ptr = (pa.data_ptr() if na else spare.data_ptr()), (pb.data_ptr() if nb else spare.data_ptr()), (pay.data_ptr() if cap else spare.data_ptr())
        else:
            pa_ptr = pb_ptr = po_ptr = None
        eng.segmented_set_op(ptr(a_in), na, ptr(ao), ptr(b_in), nb, ptr(bo), nseg, code, ptr(keys), koff.data_ptr(), ptr(index), ptr(match),
                             d_a_payload=pa_ptr, d_b_payload=pb_ptr, d_payload_out=po_ptr)
        total = int(koff[-1].item())            # the one read-back (a host synchronisation): how many were kept
        eng.check_status()      # reports bad offsets of calls that have already finished
    index, match = (None if t is None else _args.widen(t[:total]) for t in (index, match))
    return keys[:total], koff, (None if pay is None else pay[:total]), index, match


def segmented_set_op(a, a_offsets, b, b_offsets, op, payload_a=None, payload_b=None, descending: bool = False, return_index: bool = False,
                     return_match: bool = False):
    """A set operation on sorted segment a[a_offsets[s] : a_offsets[s+1]] and sorted segment b[b_offsets[s] : b_offsets[s+1]], for every s, in
    ONE engine call (rsx_segmented_set_op): returns (keys, out_offsets[, payload][, index][, match]).  op: "intersection", "difference"
    (a minus b), "union", "symmetric_difference" (or the SET_* constants).  Duplicates follow std::set_*: of a key that occurs m times in
    a's segment and n times in b's the intersection keeps a's first min(m, n), the difference a's last max(m - n, 0), the union all of a's
    and b's last max(n - m, 0), the symmetric difference a's last max(m - n, 0) and b's last max(n - m, 0).  Keys are equal iff their bits
    are (-0.0 and +0.0 differ; NaNs with equal bits are one key).  keys[out_offsets[s] : out_offsets[s+1]] holds segment s's kept elements
    in the stable merge's order (a before equal b).  The segments must be sorted as this library sorts them (segmented_sort / sort_rows
    with the same `descending`); inputs that are not sorted give an unspecified result.  payload_a / payload_b (int32 / uint32, both or
    neither): the word that came with each key.  index (int64): the position of every kept element in the concatenation of its two
    segments (below the a segment's length: from a).  match (int64, intersection only): the position in b's segment of the element a kept
    element is paired with: a[a_offsets[s] + index] and b[b_offsets[s] + match] are an inner join.  The outputs are trimmed to
    out_offsets[-1], which reads one int64 back: one host synchronisation per call.  Bad offsets raise RadixSortError."""
    k, oo, p, idx, mt = _setop_call("segmented_set_op", a, a_offsets, b, b_offsets, op, payload_a, payload_b, descending, return_index, return_match)
    return (k, oo) + ((p,) if p is not None else ()) + ((idx,) if return_index else ()) + ((mt,) if return_match else ())


def _set_rows(what: str, op: int, a, b, payload_a, payload_b, descending: bool, return_index: bool, return_match: bool):
    fa, ao, fb, bo, pa, pb = _pair_rows(what, a, b, payload_a, payload_b)
    k, oo, p, idx, mt = _setop_call(what, fa, ao, fb, bo, op, pa, pb, descending, return_index, return_match)
    res = (k,) + ((oo,) if a.dim() > 1 else ()) + ((p,) if p is not None else ()) + ((idx,) if return_index else ()) + ((mt,) if return_match else ())
    return res[0] if len(res) == 1 else res


def intersect_sorted(a, b, payload_a=None, payload_b=None, descending: bool = False, return_index: bool = False, return_match: bool = False):
    """The multiset intersection of two sorted device tensors along their last dimension: 1-D inputs are one segment and the values come
    back (then payload, index, match as asked for); N-D inputs with equal leading shape are intersected row by row, the rows being the
    segments of ONE rsx_segmented_set_op call, and (values, row_offsets, ...) comes back: row r's result is
    values[row_offsets[r] : row_offsets[r+1]].  The kept elements are a's; index are their columns in a, match their partners' columns in
    b.  Order, duplicates, payloads and errors as segmented_set_op."""
    return _set_rows("intersect_sorted", SET_INTERSECTION, a, b, payload_a, payload_b, descending, return_index, return_match)


def difference_sorted(a, b, payload_a=None, payload_b=None, descending: bool = False, return_index: bool = False):
    """The multiset difference a minus b of two sorted device tensors along their last dimension; shapes and results as intersect_sorted."""
    return _set_rows("difference_sorted", SET_DIFFERENCE, a, b, payload_a, payload_b, descending, return_index, False)


def union_sorted(a, b, payload_a=None, payload_b=None, descending: bool = False, return_index: bool = False):
    """The multiset union of two sorted device tensors along their last dimension; shapes and results as intersect_sorted.  index: the
    position in torch.cat([a, b], -1) of the row (below a's row length: from a)."""
    return _set_rows("union_sorted", SET_UNION, a, b, payload_a, payload_b, descending, return_index, False)


def symmetric_difference_sorted(a, b, payload_a=None, payload_b=None, descending: bool = False, return_index: bool = False):
    """The multiset symmetric difference of two sorted device tensors along their last dimension; shapes, results and index as union_sorted."""
    return _set_rows("symmetric_difference_sorted", SET_SYMMETRIC_DIFFERENCE, a, b, payload_a, payload_b, descending, return_index, False)


# -- joins on torch tensors -------------------------------------------------------------------------------------------------------------
_JOIN_OPS = {"inner": JOIN_INNER, "left": JOIN_LEFT, "semi": JOIN_SEMI, "anti": JOIN_ANTI}


def _join_code(what: str, how) -> int:
    if isinstance(how, str) and how in _JOIN_OPS:
        return _JOIN_OPS[how]
    if isinstance(how, int) and not isinstance(how, bool) and 0 <= how <= 3:
        return how
    raise ValueError(f"{what}: unknown kind {how!r} (one of {', '.join(_JOIN_OPS)}, or JOIN_INNER .. JOIN_ANTI)")


def _join_call(what: str, a, a_offsets, b, b_offsets, how, descending: bool, want_keys: bool, capacity):
    """One or two rsx_segmented_join calls on 1-D device tensors (both offsets None: one segment).  Returns (ia, ib, out_offsets, keys) with
    int64 indices, -1 for "none"; ib is None for the anti join, keys None unless asked for.  capacity None: a count-only call, ONE read-back
    of the total, then the writing call into buffers of exactly that size.  capacity an int: one call, no synchronisation, buffers of that
    length holding -1 (keys: 0) behind min(total, capacity)."""
    import torch
    name = _args.pair_key_name(what, a, b, "a join compares keys of one type")
    code = _join_code(what, how)
    nseg = _args.check_pair(what, a, b, a_offsets, b_offsets)
    if capacity is not None and (not isinstance(capacity, int) or isinstance(capacity, bool) or capacity < 0 or capacity > (1 << 34)):
        raise ValueError(f"{what}: capacity must be None or an int in [0, 2^34]")
    na, nb = a.numel(), b.numel()
    _args.check_count(what, "rsx_segmented_join", "keys in a and in b", na, nb)
    dev = a.device
    ooff = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
    want_b = code != JOIN_ANTI
    eng = None
    ptr = _args.ptr_nonempty
    if nseg > 0:
        a_in, b_in, ao, bo = _aligned_copy(a), _aligned_copy(b), _args.as_offsets(a_offsets), _args.as_offsets(b_offsets)      # (alive until the calls are enqueued)
        eng = _search_engine(*_args.device_and_stream(a), name, bool(descending))
        sides = (ptr(a_in), na, ptr(ao), ptr(b_in), nb, ptr(bo))
    if capacity is None:
        cap = 0
        if eng is not None:
            eng.segmented_join(*sides, nseg, code, 0, ooff.data_ptr())
            cap = int(ooff[-1].item())          # the one read-back (a host synchronisation): how many rows there are
            eng.check_status()
            if cap > (1 << 34):
                raise ValueError(f"{what}: {cap} rows are more than one call writes (2^34); join in pieces, or pass capacity")
    else:
        cap = capacity
    # (uint32 results in int32 storage: "none" is -1 as it stands, and the buffers of capacity=int start out as -1)
    ia = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    ib = torch.full((cap,), -1, dtype=torch.int32, device=dev) if want_b else None
    keys = torch.zeros(cap, dtype=a.dtype, device=dev) if want_keys else None
    if eng is not None and cap > 0:
        eng.segmented_join(*sides, nseg, code, cap, ooff.data_ptr(), d_a_index_out=ptr(ia), d_b_index_out=ptr(ib), d_keys_out=ptr(keys))
        eng.check_status()      # reports bad offsets of calls that have already finished; no synchronisation
    return _args.widen_keeping_none(ia), _args.widen_keeping_none(ib), ooff, keys


def segmented_join(a, a_offsets, b, b_offsets, how="inner", descending: bool = False, return_keys: bool = False, capacity=None):
    """The equi-join of sorted segment a[a_offsets[s] : a_offsets[s+1]] with sorted segment b[b_offsets[s] : b_offsets[s+1]], for every s, in
    rsx_segmented_join: returns (ia, ib, out_offsets[, keys]).  how: "inner" (every a element with every equal b element: a key that occurs
    m times in a's segment and n times in b's gives m x n rows), "left" (the same, and one row with ib = -1 for an a element without a
    partner), "semi" (one row per a element that has a partner, ib its first), "anti" (one row per a element that has none; ib is None), or
    the JOIN_* constants.  ia and ib (int64) are positions relative to the segments' starts; rows out_offsets[s] : out_offsets[s+1] belong
    to segment s, ordered by ia, then ib.  keys (return_keys): a's key of every row.  Keys are equal iff their bits are (-0.0 and +0.0 do
    not join; NaNs with equal bits do).  The segments must be sorted as this library sorts them (segmented_sort / sort_rows with the same
    `descending`); inputs that are not sorted give unspecified rows.  capacity=None counts first, reads the total back (ONE host
    synchronisation) and returns exactly the rows.  capacity=int never synchronises: the buffers have that length, hold -1 (keys: 0) behind
    min(out_offsets[-1], capacity), and the caller compares out_offsets[-1] with capacity.  Bad offsets raise RadixSortError."""
    ia, ib, oo, k = _join_call("segmented_join", a, a_offsets, b, b_offsets, how, descending, return_keys, capacity)
    return (ia, ib, oo) + ((k,) if return_keys else ())


def join_sorted(a, b, how="inner", descending: bool = False, capacity=None):
    """The equi-join of two sorted device tensors along their last dimension.  1-D inputs are one segment: (ia, ib) comes back, the
    positions in a and in b of every pair of equal keys (a[ia] == b[ib] bit for bit), ordered by ia, then ib.  N-D inputs with equal
    leading shape are joined row by row, the rows being the segments of one rsx_segmented_join, and (ia, ib, row_offsets) comes back:
    ia and ib are columns, and row r's pairs are [row_offsets[r] : row_offsets[r+1]).  how, capacity, order and errors as
    segmented_join."""
    fa, ao, fb, bo = _pair_rows("join_sorted", a, b)[:4]
    ia, ib, oo, _ = _join_call("join_sorted", fa, ao, fb, bo, how, descending, False, capacity)
    return (ia, ib) + ((oo,) if a.dim() > 1 else ())


def isin_sorted(a, b, invert: bool = False, descending: bool = False):
    """torch.isin(a, b) for sorted device tensors, by bits: a bool tensor shaped like a, True where the element has an equal element in b
    (in b's row of the same index for N-D inputs); invert=True: where it has none.  The semi (anti) join scattered to a mask; never
    synchronises with the host."""
    import torch
    fa, ao, fb, bo = _pair_rows("isin_sorted", a, b)[:4]
    na = fa.numel() if torch.is_tensor(fa) else 0
    ia, _, oo, _ = _join_call("isin_sorted", fa, ao, fb, bo, JOIN_ANTI if invert else JOIN_SEMI, descending, False, na)
    mask = torch.zeros(na + 1, dtype=torch.bool, device=fa.device)
    if ao is not None and na:
        # columns -> flat positions: row r's rows are [oo[r], oo[r+1]); rows behind the total hold -1 and land in the spare slot
        row = torch.searchsorted(oo[1:].contiguous(), torch.arange(na, device=fa.device), right=True).clamp_(max=ao.numel() - 2)
        ia = torch.where(ia >= 0, ia + ao[row], ia)
    mask.index_fill_(0, torch.where(ia < 0, na, ia), True)          # (rows behind the total go to the spare last slot; no host value, no synchronisation)
    return mask[:na].reshape(a.shape)
