"""CPU checks of the segmented unique: header, exports, binding and the Python callables agree on rsx_segmented_unique; the two forms of the
host referee agree with each other and with hand-made cases; and the call and the torch helpers fail loudly instead of working on the
CPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import _unique_ref as U
from _unique_ref import flat_unique, same, slow_unique, unique_oracle
from test_gpu_float_keys import random_bits, special
from test_gpu_segmented import DTYPES, offsets_from
from test_segmented import HEADER


def test_symbol_in_header_exports_and_binding(rsx):
    raw = open(HEADER).read()
    assert re.search(r"#define\s+RSX_UNIQUE_CONSECUTIVE\s+1\b", raw)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_unique\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_unique is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "uint64_t n", "const uint64_t* d_offsets", "uint64_t num_segments", "uint32_t flags",
                      "void* d_keys_out", "uint64_t* d_run_offsets_out", "uint32_t* d_counts_out", "uint32_t* d_first_out",
                      "uint32_t* d_inverse_out"]
    assert "rsx_segmented_unique" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_unique
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32] + [C.c_void_p] * 5
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_unique\b", out)
    for name in ("segmented_unique", "unique", "unique_consecutive"):
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_unique)
    assert rsx.UNIQUE_CONSECUTIVE == 1


def test_oracle_hand_made_cases():
    x = np.array([9, 5, 3, 5, 3, 3, 7, 7, 7, 2, 2, 8, 1, 9], dtype=np.uint32)
    # off[0] > 0; segments [1, 6) = 5 3 5 3 3, [6, 6), [6, 9) = 7 7 7, [9, 9), [9, 13) = 2 2 8 1, [13, 13): empty ones in the middle and last
    off = np.array([1, 6, 6, 9, 9, 13, 13], dtype=np.uint64)
    for form in (unique_oracle, slow_unique):
        r = form(x, off)
        assert r["keys"].tolist() == [3, 5, 7, 1, 2, 8]
        assert r["run_offsets"].tolist() == [0, 2, 2, 3, 3, 6, 6]
        assert r["counts"].tolist() == [3, 2, 3, 1, 2, 1]
        assert r["first"].tolist() == [1, 0, 0, 3, 0, 2]                  # the FIRST occurrence, relative to the segment start
        assert r["inverse"].tolist() == [0, 1, 0, 1, 0, 0, 0, 0, 0, 1, 1, 2, 0, 0]
        assert r["written"].tolist() == [False] + [True] * 12 + [False]
        d = form(x, off, descending=True)
        assert d["keys"].tolist() == [5, 3, 7, 8, 2, 1] and d["counts"].tolist() == [2, 3, 3, 1, 2, 1] and d["first"].tolist() == [0, 1, 0, 2, 0, 3]
        assert d["inverse"][1:13].tolist() == [0, 1, 0, 1, 1, 0, 0, 0, 1, 1, 0, 2]
        c = form(x, off, consecutive=True)
        assert c["keys"].tolist() == [5, 3, 5, 3, 7, 2, 8, 1] and c["run_offsets"].tolist() == [0, 4, 4, 5, 5, 8, 8]
        assert c["counts"].tolist() == [1, 1, 1, 2, 3, 2, 1, 1] and c["first"].tolist() == [0, 1, 2, 3, 0, 0, 2, 3]
        assert c["inverse"][1:13].tolist() == [0, 1, 2, 3, 3, 0, 0, 0, 0, 0, 1, 2]
        # equal keys on the two sides of a segment boundary stay two runs, in both modes; an empty first segment
        y = np.array([4, 4, 4, 4, 6], dtype=np.int64)
        for cons in (False, True):
            b = form(y, np.array([0, 0, 2, 5], dtype=np.uint64), consecutive=cons)
            assert b["keys"].tolist() == [4, 4, 6] and b["run_offsets"].tolist() == [0, 0, 1, 3] and b["counts"].tolist() == [2, 2, 1]
            assert b["first"].tolist() == [0, 0, 2] and b["inverse"].tolist() == [0, 0, 0, 0, 1]
        # one segment (no offsets): all equal, all distinct
        e = form(np.full(7, 5, dtype=np.int32))
        assert e["keys"].tolist() == [5] and e["counts"].tolist() == [7] and e["run_offsets"].tolist() == [0, 1] and not e["inverse"].any()
        p = np.array([3, 0, 2, 1], dtype=np.uint64)
        a = form(p)
        assert a["keys"].tolist() == [0, 1, 2, 3] and a["first"].tolist() == [1, 3, 2, 0] and a["inverse"].tolist() == [3, 0, 2, 1]
        # signed order, and totalOrder: -0.0 and +0.0 are two values, two NaN payloads are two values, equal NaN bits are one
        g = form(np.array([1, -1, 0, -1], dtype=np.int32))
        assert g["keys"].view(np.int32).tolist() == [-1, 0, 1] and g["counts"].tolist() == [2, 1, 1]
        nan_a, nan_b = 0x7FC00000, 0x7FC00001
        z = np.array([0x00000000, nan_a, 0x80000000, nan_b, 0x00000000, nan_a, 0x7F800000], dtype=np.uint32).view(np.float32)
        f = form(z)
        assert f["keys"].tolist() == [0x80000000, 0x00000000, 0x7F800000, nan_a, nan_b]           # -0.0 < +0.0 < +inf < NaNs by payload
        assert f["counts"].tolist() == [1, 2, 1, 2, 1] and f["first"].tolist() == [2, 0, 6, 1, 3]
        f = form(z, descending=True)
        assert f["keys"].tolist() == [nan_b, nan_a, 0x7F800000, 0x00000000, 0x80000000]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_oracle_forms_agree_on_ragged_cases(dtype, descending):
    rng = np.random.default_rng(DTYPES.index(dtype) * 2 + descending)
    lens = [0, 1, 2, 255, 256, 257, 1024, 1025, 4096, 4097, 9000, 0, 3, 20011]
    off = offsets_from(lens, start=3)
    n = int(off[-1]) + 5
    for maker in ("bits", "few", "one", "sorted", "special"):
        if maker == "bits":
            x = random_bits(dtype, n, rng)
        elif maker == "few":
            x = rng.integers(0, 3, n).astype(dtype)
        elif maker == "one":
            x = np.full(n, 7, dtype=dtype)
        elif maker == "sorted":
            x = np.sort(rng.integers(0, 500, n)).astype(dtype)
        elif np.dtype(dtype).kind == "f":
            x = special(dtype, n, rng)
        else:
            continue
        for cons in (False, True):
            a = unique_oracle(x, off, descending, cons)
            assert same(a, slow_unique(x, off, descending, cons)), (maker, cons)
            # what every answer satisfies: the inverse reconstructs the input, the counts add up to the segment lengths
            xu = x.view(a["keys"].dtype)
            for s in range(len(lens)):
                lo, hi = int(off[s]), int(off[s + 1])
                u0, u1 = int(a["run_offsets"][s]), int(a["run_offsets"][s + 1])
                assert np.array_equal(a["keys"][u0:u1][a["inverse"][lo:hi]], xu[lo:hi])
                assert int(a["counts"][u0:u1].sum()) == hi - lo
        assert same(unique_oracle(x[:5000]), slow_unique(x[:5000]))
        for cons in (False, True):                     # the one-sort form: the same dict
            assert same(flat_unique(x, off, descending, cons), unique_oracle(x, off, descending, cons)), (maker, cons)
        assert same(flat_unique(x[:5000]), slow_unique(x[:5000]))


def small_layouts():
    """scaled-down copies (tiles of 16 or 64 keys, 4 CUs) of every layout of tests/test_gpu_unique_reduce_paths.py: name -> (n, off, keys)"""
    out = {}
    for chunk in (2, 3):
        out[f"ragged{chunk}"] = U.ragged_layout(chunk, tile=64, cus=4, wg=3, long_tiles=5)[:3]
    for kind in ("ragged", "aligned", "chunk2"):
        out[f"dense_{kind}"] = U.dense_layout(kind, tile=16, cus=4)
    for kind in ("mid", "edge", "none", "none_edge"):
        out[f"deep_{kind}"] = U.deep_layout(kind, tile=64)
    return out


@pytest.mark.parametrize("name", list(small_layouts()))
def test_flat_unique_equals_both_forms_on_the_new_layouts(name):
    n, off, keys = small_layouts()[name]
    assert keys.size == n and int(off[-1]) <= n and (np.diff(off.astype(np.int64)) >= 0).all()
    for x in (keys, keys.astype(np.int64) - 2):
        for descending in (False, True):
            for cons in (False, True):
                a = flat_unique(x, off, descending, cons)
                assert same(a, unique_oracle(x, off, descending, cons)), (descending, cons)
                assert same(a, slow_unique(x, off, descending, cons)), (descending, cons)
                assert a["order"].size == int(off[-1]) - int(off[0]) and a["heads"].size == int(a["run_offsets"][-1])


def test_tile_grid_mirror():
    """chunk = ceil(npad / (16 * CUs)): 1 up to 4095 * 4096 keys, 2 up to 8191 * 4096, then 3"""
    T = U.TILE
    assert U.tile_grid(1) == {"ntiles": 1, "npad": 16, "chunk": 1, "tgrid": 16}
    assert U.tile_grid(4095 * T)["chunk"] == 1 and U.tile_grid(4095 * T + 1)["chunk"] == 2
    assert U.tile_grid(8191 * T)["chunk"] == 2 and U.tile_grid(8191 * T + 1)["chunk"] == 3
    assert U.tile_grid(1 << 24) == {"ntiles": 4096, "npad": 4112, "chunk": 2, "tgrid": 2056}


def test_layouts_reach_their_paths():
    """Each layout of tests/test_gpu_unique_reduce_paths.py still reaches what it is there for on 256 CUs; if the formulas of
    unique_groups_enqueue change, this fails first."""
    T = U.TILE
    for chunk in (2, 3):
        n, off, keys, (start, length) = U.ragged_layout(chunk)
        o = off.astype(np.int64)
        lens = np.diff(o)
        assert U.tile_grid(n)["chunk"] == chunk and keys.size == n and o[-1] <= n and (lens >= 0).all()
        assert (lens == 0).any() and (lens > 3 * T).any() and ((lens > 0) & (lens < 4)).any()
        assert (o % T == 0).any() and (o % T == 1).any() and (o % T == T - 1).any() and o[0] % T != 0 and o[-1] % T != 0
        # the long run: longer than 65 tiles, begins mid-tile in the last tile of a workgroup's range, ends in another workgroup's,
        # no segment border inside it, other keys on both sides
        assert length > 65 * T and start % T != 0 and (start // T) % chunk == chunk - 1 and (start + length) // T // chunk > start // T // chunk + 20
        assert (keys[start:start + length] == keys[start]).all() and keys[start - 1] != keys[start] and keys[start + length] != keys[start]
        s = int(np.searchsorted(o, start, side="right"))
        assert o[s - 1] < start and o[s] >= start + length and o[s - 1] // T == start // T
        same_both_sides = keys[o[1:-1] - 1] == keys[o[1:-1]]                  # equal keys on both sides of a segment border
        assert same_both_sides[lens[:-1] > 0].any()
    for kind in ("ragged", "aligned", "chunk2"):
        n, off, keys = U.dense_layout(kind)
        o = off.astype(np.int64)
        per = U.offsets_per_tile(o, n)
        assert n >= 1 << 22 and keys.size == n and per.size == U.tile_grid(n)["ntiles"] + 1
        assert (per > 256).any() and (per > 512).any() and U.tile_grid(n)["chunk"] == (2 if kind == "chunk2" else 1)
        lens = np.diff(o)
        assert lens.max() <= 5 and np.median(lens) <= 3
        pos, cnt = np.unique(o, return_counts=True)
        blocks = pos[cnt > 1000]                                              # the three blocks of 1000 empty segments
        assert blocks.size == 3 and blocks[0] % T not in (0, T - 1) and blocks[1] % T == 0 and blocks[2] == o[-1]
        assert (o[-1] == n and n % T == 0) if kind == "aligned" else (o[-1] < n and o[-1] % T != 0)
    for kind in ("mid", "edge", "none", "none_edge"):
        n, off, keys = U.deep_layout(kind)
        o = off.astype(np.int64)
        assert o[0] >= 3 * T and o[-1] <= n - 3 * T and keys.size == n
        assert (o[0] % T == 0) == (kind in ("edge", "none_edge")) and (o[0] == o[-1]) == kind.startswith("none")


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    # a null engine is refused, nothing is computed
    assert lib.rsx_segmented_unique(None, None, 16, None, 1, 0, None, None, None, None, None) == 4
    torch = pytest.importorskip("torch")
    keys = torch.arange(10, dtype=torch.int32)
    offsets = torch.tensor([0, 10], dtype=torch.int64)
    with pytest.raises(ValueError):              # host tensors: no CPU fallback
        rsx.segmented_unique(keys, offsets)
    with pytest.raises(ValueError):
        rsx.unique(keys, return_inverse=True, return_counts=True)
    with pytest.raises(ValueError):
        rsx.unique_consecutive(keys)
    with pytest.raises(NotImplementedError):
        rsx.unique(keys, dim=0)
    with pytest.raises(NotImplementedError):
        rsx.unique_consecutive(keys.reshape(2, 5), dim=1)
    if not torch.cuda.is_available():
        with pytest.raises(rsx.RadixSortError) as ei:
            rsx.Engine(np.uint32, 16).segmented_unique(0, 16, None, 1, 0, 0)
        assert ei.value.status == 2              # INITIALIZATION_FAILED: no device, no silent CPU path
