"""CPU checks of the segmented select: header, exports and binding agree on rsx_segmented_select; the two forms of the host referee
agree with each other and with hand-made cases; the rank arithmetic of kthvalue / median / quantile reproduces torch's results bit for
bit when applied to torch.sort output; and the call and the torch helpers fail loudly instead of selecting on the CPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import _topk_ref
from _select_ref import NONE, fast_select, random_ranks, select_oracle
from test_gpu_float_keys import random_bits, special
from test_gpu_segmented import DTYPES, offsets_from
from test_segmented import HEADER


def test_symbol_in_header_exports_and_binding(rsx):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_select\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_select is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "uint64_t n", "const uint64_t* d_offsets", "uint64_t num_segments",
                      "const uint32_t* d_ranks", "uint32_t ranks_per_segment", "void* d_keys_out", "uint32_t* d_index_out"]
    assert "rsx_segmented_select" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_select
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_select\b", out)
    for name in ("segmented_select", "kthvalue", "median", "quantile", "select_ranks"):
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_select)
    assert rsx.SELECT_MAX_RANKS == 8


def test_oracle_hand_made_cases():
    x = np.array([5, 3, 9, 3, 1, 8, 8, 2, 7, 0, 4, 6], dtype=np.uint32)
    # segments [1, 4) = 3 9 3, [4, 4), [4, 5) = 1, [5, 11) = 8 8 2 7 0 4, [11, 12) = 6
    off = np.array([1, 4, 4, 5, 11, 12], dtype=np.uint64)
    ranks = np.array([[1, 0, 3], [0, NONE, 0], [0, 1, 0], [5, 4, 4], [NONE, 0, 7]], dtype=np.uint32)
    for form in (select_oracle, fast_select):
        keys, pos, written = form(x, off, ranks)
        assert keys.tolist() == [[3, 3, 0], [0, 0, 0], [1, 0, 1], [8, 8, 8], [0, 6, 0]]
        assert pos.tolist() == [[2, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]]
        assert written.tolist() == [[True, True, False], [False] * 3, [True, False, True], [True] * 3, [False, True, False]]
        # descending: rank 0 is the largest, equal keys still lowest index first
        keys, pos, _ = form(x, off, ranks, descending=True)
        assert keys[3].tolist() == [0, 2, 2] and pos[3].tolist() == [4, 2, 2]
        keys, pos, _ = form(x, np.array([5, 11], dtype=np.uint64), np.array([[0, 1]], dtype=np.uint32), descending=True)
        assert keys.tolist() == [[8, 8]] and pos.tolist() == [[0, 1]]
        # the second and the last of a run of ties, not the first
        y = np.array([2, 1, 2, 2, 0, 2], dtype=np.int32)
        keys, pos, _ = form(y, np.array([0, 6], dtype=np.uint64), np.array([[3, 5, 2]], dtype=np.uint32))
        assert keys.view(np.int32).tolist() == [[2, 2, 2]] and pos.tolist() == [[2, 5, 0]]
        # totalOrder: -0.0 below +0.0, +NaN above +inf
        z = np.array([0.0, np.nan, -0.0, np.inf, 1.0], dtype=np.float32)
        _, pos, _ = form(z, np.array([0, 5], dtype=np.uint64), np.array([[0, 1, 4, 3]], dtype=np.uint32))
        assert pos.tolist() == [[2, 0, 1, 3]]
        # invalid segments are left alone: [3, 2) decreasing, [2, 11) past n
        w = np.arange(10, dtype=np.uint64)[::-1].copy()
        _, _, written = form(w, np.array([0, 3, 2, 11], dtype=np.uint64), np.zeros((3, 1), dtype=np.uint32))
        assert written.tolist() == [[True], [False], [False]]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_oracle_forms_agree_on_ragged_cases(dtype, descending):
    rng = np.random.default_rng(DTYPES.index(dtype) * 2 + descending)
    lens = [0, 1, 2, 255, 256, 257, 1024, 1025, 4096, 4097, 9000, 0, 3, 20011]
    off = offsets_from(lens, start=3)
    n = int(off[-1]) + 5
    for maker in ("bits", "few", "special"):
        if maker == "bits":
            x = random_bits(dtype, n, rng)
        elif maker == "few":
            x = rng.integers(0, 3, n).astype(dtype)
        elif np.dtype(dtype).kind == "f":
            x = special(dtype, n, rng)
        else:
            continue
        ranks = random_ranks(off, 8, rng)
        a = select_oracle(x, off, ranks, descending)
        b = fast_select(x, off, ranks, descending)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    # the layouts of the big GPU shapes, cut down: fast_select against the argsort form on the ragged rows
    off = _topk_ref.ragged_offsets()[:40]
    x = random_bits(dtype, _topk_ref.shape_n(off), rng)
    ranks = random_ranks(off, 3, rng)
    for u, v in zip(select_oracle(x, off, ranks, descending), fast_select(x, off, ranks, descending)):
        assert np.array_equal(u, v)


def test_rank_arithmetic_kthvalue_and_median(rsx):
    torch = pytest.importorskip("torch")
    g = torch.Generator().manual_seed(3)
    for size in (1, 2, 5, 6, 1001):
        x = torch.randperm(size * 4, generator=g).reshape(4, size).to(torch.int32)          # distinct: torch's indices are defined
        sv, si = torch.sort(x, dim=-1, stable=True)
        lo, hi, w = rsx.select_ranks(size)
        assert lo == hi == (size - 1) // 2 and w is None
        wv, wi = torch.median(x, dim=-1)
        assert torch.equal(sv[:, lo], wv) and torch.equal(si[:, lo], wi)
        for k in {1, (size + 1) // 2, size}:
            lo, hi, w = rsx.select_ranks(size, k=k)
            assert lo == hi == k - 1 and w is None
            wv, wi = torch.kthvalue(x, k, dim=-1)
            assert torch.equal(sv[:, lo], wv) and torch.equal(si[:, lo], wi)
        for k in (0, size + 1):
            with pytest.raises(ValueError):
                rsx.select_ranks(size, k=k)
    with pytest.raises(ValueError):
        rsx.select_ranks(0)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("mode", ["linear", "lower", "higher", "midpoint", "nearest"])
def test_rank_arithmetic_quantile_bitwise(rsx, dtype, mode):
    """lerp(sorted[lo], sorted[hi], weight) with select_ranks' (lo, hi, weight) equals torch.quantile bit for bit, every mode, both dtypes."""
    torch = pytest.importorskip("torch")
    dt = getattr(torch, dtype)
    g = torch.Generator().manual_seed(11)
    q = torch.tensor([0.0, 0.1, 0.25, 1 / 3, 0.5, 0.77, 0.999, 1.0], dtype=dt)
    for size in (1, 2, 6, 1001, 50257):
        x = torch.randn(3, size, generator=g, dtype=dt)
        sv = torch.sort(x, dim=-1).values
        lo, hi, w = rsx.select_ranks(size, q=q, interpolation=mode)
        assert lo.dtype == torch.int64 and int(lo.min()) >= 0 and int(hi.max()) <= size - 1
        got = sv[:, lo] if w is None else torch.lerp(sv[:, lo], sv[:, hi], w)
        want = torch.quantile(x, q, dim=-1, interpolation=mode)
        assert torch.equal(got.movedim(-1, 0), want), (size, mode)
    with pytest.raises(ValueError):
        rsx.select_ranks(5, q=q, interpolation="cubic")


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    # a null engine is refused, nothing is selected
    assert lib.rsx_segmented_select(None, None, 16, None, 1, None, 1, None, None) == 4
    torch = pytest.importorskip("torch")
    keys = torch.arange(10, dtype=torch.int32)
    offsets = torch.tensor([0, 10], dtype=torch.int64)
    with pytest.raises(ValueError):              # host tensors: no CPU fallback
        rsx.segmented_select(keys, offsets, torch.tensor([[3]]))
    with pytest.raises(ValueError):
        rsx.kthvalue(torch.ones(3, 4, dtype=torch.int32), 2)
    with pytest.raises(ValueError):
        rsx.median(torch.ones(3, 4, dtype=torch.int32))
    with pytest.raises(ValueError):
        rsx.quantile(torch.ones(3, 4), 0.5)
    if not torch.cuda.is_available():
        with pytest.raises(rsx.RadixSortError) as ei:
            rsx.Engine(np.uint32, 16).segmented_select(0, 16, 0, 1, 0, 1, 0, 0)
        assert ei.value.status == 2              # INITIALIZATION_FAILED: no device, no silent CPU path
