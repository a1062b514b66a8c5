"""CPU checks of the segmented top-k: header, exports and binding agree on rsx_segmented_topk; the numpy oracle of
tests/test_gpu_topk.py gives the stable-sort prefix of every segment on hand-made cases (ties across the k boundary, segments shorter
than k, empty and invalid segments); and the call and the torch helpers fail loudly instead of selecting on the CPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from test_gpu_topk import topk_oracle
from test_segmented import HEADER


def test_symbol_in_header_exports_and_binding(rsx):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_topk\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_topk is not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "uint64_t n", "const uint64_t* d_offsets", "uint64_t num_segments", "uint32_t k",
                      "void* d_keys_out", "uint32_t* d_index_out"]
    assert "rsx_segmented_topk" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_topk
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_topk\b", out)
    assert callable(rsx.Engine.segmented_topk) and callable(rsx.segmented_topk) and callable(rsx.topk)
    assert rsx.TOPK_MAX_K == 4096


def test_oracle_hand_made_cases():
    x = np.array([5, 3, 9, 3, 1, 8, 8, 2, 7, 0, 4, 6], dtype=np.uint32)
    # segments [1, 4) [4, 4) [4, 5) [5, 11) [11, 12)
    off = np.array([1, 4, 4, 5, 11, 12], dtype=np.uint64)
    keys, pos, written = topk_oracle(x, off, 2)
    assert keys.tolist() == [[3, 3], [0, 0], [1, 0], [0, 2], [6, 0]]
    assert pos.tolist() == [[0, 2], [0, 0], [0, 0], [4, 2], [0, 0]]
    assert written.tolist() == [[True, True], [False, False], [True, False], [True, True], [True, False]]
    # descending: the largest first, ties lowest index first (segment [5, 11) holds 8, 8, 2, 7, 0, 4)
    keys, pos, written = topk_oracle(x, off, 2, descending=True)
    assert keys[3].tolist() == [8, 8] and pos[3].tolist() == [0, 1]
    keys, pos, _ = topk_oracle(x, np.array([4, 11], dtype=np.uint64), 3, descending=True)
    assert keys.tolist() == [[8, 8, 7]] and pos.tolist() == [[1, 2, 4]]
    # a tie run across the k boundary: only its first members (by index) are taken
    y = np.array([2, 1, 2, 2, 0, 2], dtype=np.int32)
    keys, pos, _ = topk_oracle(y, np.array([0, 6], dtype=np.uint64), 4)
    assert keys.view(np.int32).tolist() == [[0, 1, 2, 2]] and pos.tolist() == [[4, 1, 0, 2]]
    # float keys in totalOrder: +NaN above +inf, -0.0 below +0.0
    z = np.array([0.0, np.nan, -0.0, np.inf, 1.0], dtype=np.float32)
    keys, pos, _ = topk_oracle(z, np.array([0, 5], dtype=np.uint64), 3, descending=True)
    assert pos.tolist() == [[1, 3, 4]]
    keys, pos, _ = topk_oracle(z, np.array([0, 5], dtype=np.uint64), 2)
    assert pos.tolist() == [[2, 0]]


def test_oracle_leaves_bad_segments_alone():
    x = np.arange(10, dtype=np.uint64)[::-1].copy()
    # [0, 3) fine, [3, 2) decreasing, [2, 11) past n = 10
    keys, pos, written = topk_oracle(x, np.array([0, 3, 2, 11], dtype=np.uint64), 2)
    assert written.tolist() == [[True, True], [False, False], [False, False]]
    assert keys[0].tolist() == [7, 8] and pos[0].tolist() == [2, 1]


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    # a null engine is refused, nothing is selected
    assert lib.rsx_segmented_topk(None, None, 16, None, 1, 4, None, None) == 4
    torch = pytest.importorskip("torch")
    keys = torch.arange(10, dtype=torch.int32)
    offsets = torch.tensor([0, 10], dtype=torch.int64)
    with pytest.raises(ValueError):              # host tensors: no CPU fallback
        rsx.segmented_topk(keys, offsets, 3)
    with pytest.raises(ValueError):
        rsx.topk(torch.ones(3, 4, dtype=torch.int32), 2)
    if not torch.cuda.is_available():
        with pytest.raises(rsx.RadixSortError) as ei:
            rsx.Engine(np.uint32, 16).segmented_topk(0, 16, 0, 1, 4, 0, 0)
        assert ei.value.status == 2              # INITIALIZATION_FAILED: no device
