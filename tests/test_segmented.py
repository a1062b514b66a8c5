"""CPU checks of the segmented sort: header, exports and binding agree on rsx_segmented_sort; the numpy oracle of
tests/test_gpu_segmented.py gives the stable per-segment order on hand-made cases (bad segments and positions outside the
segments untouched); the call and the torch helpers fail loudly instead of sorting on the CPU; and the mirror of the launch
geometry in tests/_segmented_ref.py is right on a hand-made case and says that every layout of tests/test_gpu_segmented_paths.py
reaches the path it is named for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _segmented_ref as S
from test_gpu_float_keys import enc
from test_gpu_segmented import covered, offsets_from, seg_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "radixsort_hip.h")


def test_symbol_in_header_exports_and_binding(rsx):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_sort\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_sort is not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "const uint32_t* d_payload", "uint64_t n", "const uint64_t* d_offsets",
                      "uint64_t num_segments", "void* d_keys_out", "uint32_t* d_payload_out"]
    assert "rsx_segmented_sort" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_sort
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_sort\b", out)
    assert callable(rsx.Engine.segmented_sort) and callable(rsx.segmented_sort) and callable(rsx.sort_rows)


def test_oracle_hand_made_cases():
    x = np.array([5, 3, 9, 3, 1, 8, 8, 2, 7, 0, 4], dtype=np.uint32)
    # segments [1, 4) [4, 4) [4, 5) [5, 9); positions 0, 9, 10 outside
    off = np.array([1, 4, 4, 5, 9], dtype=np.uint64)
    want = seg_oracle(x, off, x.size)
    assert want.tolist() == [0, 1, 3, 2, 4, 7, 8, 5, 6, 9, 10]
    assert x[want].tolist() == [5, 3, 3, 9, 1, 2, 7, 8, 8, 0, 4]
    # descending, stable: equal keys keep their input order
    want = seg_oracle(x, off, x.size, descending=True)
    assert want.tolist() == [0, 2, 1, 3, 4, 5, 6, 8, 7, 9, 10]
    # signed and float keys go through the engine's encoding
    y = np.array([-1, 2, -3, 0], dtype=np.int32)
    assert y[seg_oracle(y, np.array([0, 4], dtype=np.uint64), 4)].tolist() == [-3, -1, 0, 2]
    z = np.array([1.5, -0.0, 0.0, -2.0, np.inf], dtype=np.float32)
    assert z[seg_oracle(z, np.array([0, 5], dtype=np.uint64), 5)].view(np.uint32).tolist() == \
        np.array([-2.0, -0.0, 0.0, 1.5, np.inf], dtype=np.float32).view(np.uint32).tolist()


def test_oracle_leaves_bad_segments_alone():
    x = np.array([4, 3, 2, 1, 0, 9, 8], dtype=np.uint32)
    # [0, 2) sorted, [2, 1) decreasing: untouched
    assert seg_oracle(x, np.array([0, 2, 1], dtype=np.uint64), x.size).tolist() == [1, 0, 2, 3, 4, 5, 6]
    # [0, 2) and [2, 5) sorted, [5, 9) ends past n = 7: untouched
    assert seg_oracle(x, np.array([0, 2, 5, 9], dtype=np.uint64), x.size).tolist() == [1, 0, 4, 3, 2, 5, 6]


def test_offsets_cover_every_residue():
    off = offsets_from([0, 1, 2, 31, 32, 33, 255, 256, 257], start=3)
    assert {int(v) % 4 for v in off} == {0, 1, 2, 3}


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    # a null engine is refused, nothing is sorted
    assert lib.rsx_segmented_sort(None, None, None, 16, None, 1, None, None) == 4
    torch = pytest.importorskip("torch")
    keys = torch.arange(10, dtype=torch.int32)
    offsets = torch.tensor([0, 10], dtype=torch.int64)
    with pytest.raises(ValueError):              # host tensors: no CPU fallback
        rsx.segmented_sort(keys, offsets)
    with pytest.raises(ValueError):
        rsx.sort_rows(torch.ones(3, 4, dtype=torch.int32).reshape(-1))
    if not torch.cuda.is_available():
        with pytest.raises(rsx.RadixSortError) as ei:
            rsx.Engine(np.uint32, 16).segmented_sort(0, 16, 0, 1, 0)
        assert ei.value.status == 2              # INITIALIZATION_FAILED: no device


# -- the launch geometry and the layouts of tests/test_gpu_segmented_paths.py ---------------------------------------------------------------


def test_geometry_hand_made_case():
    """Twelve segments over n = 20000, two of them large, three bad; every figure below is worked out by hand from the offsets."""
    #      0  1  2   3    4     5     6     7      8      9      10     11
    off = [2, 2, 3, 10, 300, 1000, 5100, 5100, 14000, 13000, 15000, 21000, 16000]
    # 0 empty, 1 one key, 2 [3, 10) class 0, 3 [10, 300) and 4 [300, 1000) class 1, 5 [1000, 5100) large, 6 empty, 7 [5100, 14000) large,
    # 8 [14000, 13000) decreasing, 9 [13000, 15000) class 2, 10 [15000, 21000) past n, 11 [21000, 16000) decreasing
    g = S.seg_geometry(off, 20000)
    assert g["valid"].tolist() == [True] * 8 + [False, True, False, False]
    assert g["bad"].tolist() == [8, 10, 11] and g["first_bad"] == 8
    assert g["ones"] == 1 and g["count"] == [1, 2, 1] and g["large"].tolist() == [5, 7]
    assert [l.tolist() for l in g["lists"]] == [[2], [3, 4], [9]]
    assert (g["nblocks"], g["per"], g["large_blocks"], g["last_large_block"]) == (1, 1, 1, 0)
    # min(nseg, n / min_len, cus * per_cu) = min(12, 10000, 8192), min(12, 77, 4096), min(12, 19, 1024)
    assert g["grid"] == [12, 12, 12] and g["trips"] == [1, 1, 1]
    # 20000 / 4097 = 4 large segments at most; ceil(20000 / 4096) = 5 grid tiles and one partial tile per large segment
    assert (g["max_large"], g["max_tiles"], g["chain_grid"]) == (4, 9, 9)
    # [1000, 5100): grid tiles 0 and 1 -> 3096 + 1004 keys; [5100, 14000): grid tiles 1, 2, 3 -> 3092 + 4096 + 1712
    assert (g["tot_large"], g["tot_tiles"], g["tot_keys"]) == (2, 5, 4100 + 8900)
    assert (g["chain_ok"], g["nlarge"], g["tiles"]) == (1, 2, 5)
    assert g["first_tile"] == [3096, 3092] and g["last_tile"] == [1004, 1712]
    # one CU: class 2 has min(12, 19, 4) workgroups, still one trip for its one segment; 40 segments of class 2 on one CU make 10 trips
    assert S.seg_geometry(off, 20000, cus=1)["grid"] == [12, 12, 4]
    many = S.seg_geometry(S.offsets_from([2000] * 40), 80000, cus=1)
    assert many["count"] == [0, 0, 40] and many["grid"][2] == 4 and many["trips"] == [0, 0, 10]
    # no segment can be large: no chain at all
    none = S.seg_geometry([0, 4096], 4096)
    assert (none["max_large"], none["max_tiles"], none["chain_grid"], none["count"]) == (0, 0, 0, [0, 0, 1])


def test_fast_covered_matches_the_loop():
    rng = np.random.default_rng(1)
    cases = [([1, 4, 4, 5, 9], 11), ([0, 2, 1], 7), ([0, 2, 5, 9], 7), ([3, 3], 5), S.FOLD_SMALL[::-1], S.FOLD_LARGE[::-1]]
    cases += [(np.sort(rng.integers(0, 5000, 300)), 4000), (rng.integers(0, 600, 200), 500)]
    n, off = S.sparse_large_bad()
    cases.append((off[540000:], n))
    for off, n in cases:
        assert np.array_equal(S.covered(off, n), covered(np.asarray(off), n))


def test_layout_sparse_large_reaches_block_prefixes():
    """sparse_large: per == 2, large segments in >= 30 classify blocks, the last block among them, at the edge of blocks 0 / 1"""
    n, off = S.sparse_large()
    g = S.seg_geometry(off, n)
    print(n, S.summary(g))
    assert len(off) - 1 == 600000 and int(off[0]) == 3 and int(off[-1]) == n and 1000000 < n < 1400000
    assert g["per"] == 2 and g["nblocks"] == 293
    assert g["large_blocks"] >= 30 and g["last_large_block"] == g["nblocks"] - 1
    assert set(S.SPARSE_FORCED) <= set(g["large"].tolist()) and 40 <= g["tot_large"] <= 43
    assert g["chain_ok"] == 1 and g["first_bad"] is None
    assert g["count"][0] > 250000 and g["count"][1] == 10 and g["count"][2] == 10 and g["ones"] > 100000
    # large segments beyond block 256 get their prefix from the second block of a scan thread
    assert np.count_nonzero(g["large"] // S.SEG_PER_BLOCK >= S.SCAN_THREADS) >= 3
    lens = np.diff(off.astype(np.int64))
    assert lens[g["large"]].min() >= 4097 and lens[g["large"]].max() <= 9000


def test_layout_sparse_large_bad_spikes_deep_in_the_list():
    """sparse_large_bad: four bad segments beyond 524288, first 550001; the valid ones are disjoint; large ones follow the spikes"""
    n, off = S.sparse_large_bad()
    g = S.seg_geometry(off, n)
    print(n, S.summary(g))
    assert g["bad"].tolist() == [550001, 550002, 580000, 580001] and g["first_bad"] == 550001
    assert g["first_bad"] // S.SEG_PER_BLOCK >= S.SCAN_THREADS and g["per"] == 2
    assert g["chain_ok"] == 1 and g["large"].max() == 599999 and g["large_blocks"] >= 30
    o = off.astype(np.int64)
    lens = np.where(g["valid"], o[1:] - o[:-1], 0)
    cov = S.covered(off, n)
    assert int(lens.sum()) == int(cov.sum())                        # no valid segment overlaps another
    for s in (550001, 580000):
        lo, hi = int(S.sparse_large()[1][s]), int(S.sparse_large()[1][s + 2])
        assert not cov[lo:hi].any() and cov[lo - 1] and cov[hi]      # the bad ranges, and nothing else around them


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("cus", [256, 304, 64])
def test_layout_stride_second_item_is_shorter(cls, cus):
    """stride_layout: trips[cls] >= 2, and the item a workgroup takes after its first (i + grid) is the shorter one"""
    n, off = S.stride_layout(cls, cus)
    g = S.seg_geometry(off, n, cus)
    print(n, S.summary(g))
    extra = 400 if cls == 1 else 200
    grid = cus * S.PER_CU[cls]
    assert g["grid"][cls] == grid and g["count"][cls] == grid + extra == len(off) - 1 and g["trips"][cls] == 2
    assert g["count"][3 - cls] == 0 and g["count"][0] == 0 and g["tot_large"] == 0 and g["first_bad"] is None
    lens = np.diff(off.astype(np.int64))
    order = g["lists"][cls]
    i = np.arange(extra)
    assert np.all(lens[order[i + grid]] < lens[order[i]])
    lo, hi = (257, 1024) if cls == 1 else (1025, 4096)
    assert lens.min() >= lo and lens.max() <= hi
    if cus == 256:
        assert 2500000 < n < 3500000
    x = S.few_distinct(np.float32, off, n, np.random.default_rng(0))
    a, b = int(off[0]), int(off[1])
    assert set(np.unique(x[a:b]).tolist()) <= set(range(7)) and np.unique(x[int(off[1]):int(off[2])]).size > 100


def nibbles(e):
    bits = e.dtype.itemsize * 8
    return np.stack([(e >> e.dtype.type(4 * j)) & e.dtype.type(15) for j in range(bits // 4)])


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype", [np.uint32, np.int64, np.float64], ids=lambda d: np.dtype(d).name)
def test_layout_digit_keys_hold_in_the_call_order(dtype, descending):
    """digit_keys: the digits named are those of the order-mapped key (enc, complemented when descending), in either direction"""
    off = S.offsets_from(S.DIGIT_LENGTHS)
    n = int(off[-1])
    g = S.seg_geometry(off, n)
    assert g["count"] == [3, 2, 2] and g["tot_large"] == 3 and g["chain_ok"] == 1
    rng = np.random.default_rng(3)
    image = lambda x: ~enc(x) if descending else enc(x)
    ones = image(np.zeros(1, dtype=dtype)).dtype.type(~np.uint64(0))
    e = image(S.digit_keys("equal", dtype, off, n, rng, descending))
    assert np.unique(e).size == 1
    d = nibbles(image(S.digit_keys("digits_7_8", dtype, off, n, rng, descending)))
    assert set(np.unique(d).tolist()) == {7, 8} and all(np.unique(row).size == 2 for row in d)
    d = nibbles(image(S.digit_keys("digits_0_15", dtype, off, n, rng, descending)))
    assert set(np.unique(d).tolist()) == {0, 15} and all(np.unique(row).size == 2 for row in d)
    e = image(S.digit_keys("window", dtype, off, n, rng, descending))
    a, b = int(off[7]), int(off[8])                                 # the 30000-key segment: one byte varies
    assert bin(int(np.bitwise_or.reduce(e[a:b] ^ e[a]))).count("1") <= 8 and np.unique(e[a:b]).size > 200
    e = image(S.digit_keys("pad_heavy", dtype, off, n, rng, descending))
    assert np.count_nonzero(e == ones) > 0.9 * n and np.count_nonzero(e == ones - 1) > 100
    for kind, sign in (("sorted", 1), ("reversed", -1)):
        e = image(S.digit_keys(kind, dtype, off, n, rng, descending))
        for s in range(len(off) - 1):
            seg = e[int(off[s]):int(off[s + 1])]
            assert np.all(seg[:-1] <= seg[1:]) if sign > 0 else np.all(seg[:-1] >= seg[1:])
        assert np.unique(e[a:b]).size < b - a                       # ties: the payload shows the stable order


def test_layout_grid_tiles():
    """grid_layout: first and last tiles of 1 / 1, 4096 / 4096, 4096 / 1, two segments meeting mid-tile, a last tile of one key at n"""
    n, off = S.grid_layout()
    g = S.seg_geometry(off, n)
    print(n, S.summary(g))
    assert list(zip(g["first_tile"], g["last_tile"])) == S.GRID_TILES
    o = off.astype(np.int64)
    la, lb = o[g["large"]], o[g["large"] + 1]
    assert la[0] % 4096 == 4095 and lb[0] - la[0] == 4098 and (lb[0] + 4095) // 4096 - la[0] // 4096 == 3
    assert la[1] % 4096 == 0 and lb[1] % 4096 == 0 and lb[1] - la[1] == 8192
    assert la[2] % 4096 == 0 and lb[2] - la[2] == 4097
    assert lb[3] == la[4] and lb[3] % 4096 not in (0, 1, 4095) and g["large"][4] == g["large"][3] + 1
    assert lb[5] == n == int(off[-1]) and n % 4096 == 1
    assert g["chain_ok"] == 1 and g["count"] == [1, 1, 2] and g["ones"] == 1 and int(np.count_nonzero(np.diff(o) == 0)) == 2


def test_layout_full_house():
    """full_house_layout: nlarge == max_large exactly"""
    n, off = S.full_house_layout()
    g = S.seg_geometry(off, n)
    print(n, S.summary(g))
    assert g["nlarge"] == g["max_large"] == 37 and g["chain_ok"] == 1 and g["tiles"] == 74 <= g["max_tiles"] == 75
    assert n == int(off[-1]) == 37 * 4097 and int(off[0]) == 0


def test_layout_engine_sequence_shrinks():
    """engine_sequence: every call fits the engine; after the larger calls the chain's rows shrink to 2, 0, 1, 0 large segments"""
    shapes = []
    for lens, start in S.engine_sequence():
        off = S.offsets_from(lens, start)
        n = int(off[-1])
        assert n <= S.ENGINE_CAPACITY
        g = S.seg_geometry(off, n)
        assert g["chain_ok"] == 1 and g["first_bad"] is None
        shapes.append((g["nlarge"], g["tiles"], g["count"]))
    assert shapes[0][:2] == (1, 1024) and shapes[1][:2] == (200, 400)
    assert [s[0] for s in shapes[2:]] == [2, 0, 1, 0]
    assert shapes[2][2] == [1, 0, 0] and shapes[3][2] == [0, 3000, 0] and shapes[4][2] == [1, 0, 0] and shapes[5][2] == [1, 0, 0]


def test_layout_folded_offsets():
    """FOLD_LARGE: chain_ok == 0 (three valid large segments where n keys hold one); FOLD_SMALL: the chain's bounds hold, four identical
    class 1 segments walked by ONE workgroup"""
    n, off = S.FOLD_LARGE
    g = S.seg_geometry(off, n)
    print(n, S.summary(g))
    assert (g["tot_large"], g["max_large"], g["tot_keys"]) == (3, 1, 15000) and g["max_tiles"] == 3
    assert (g["chain_ok"], g["nlarge"], g["tiles"]) == (0, 0, 0) and g["first_bad"] == 1 and g["bad"].tolist() == [1, 3]
    assert g["count"] == [0, 0, 0] and g["ones"] == 0
    n, off = S.FOLD_SMALL
    g = S.seg_geometry(off, n)
    print(n, S.summary(g))
    assert (g["max_large"], g["max_tiles"], g["tot_large"], g["chain_ok"]) == (0, 0, 0, 1)
    assert g["count"] == [0, 4, 0] and g["grid"][1] == 1 and g["trips"][1] == 4 and g["grid"][2] == 0
    assert g["first_bad"] == 1 and g["bad"].tolist() == [1, 3, 5]
    assert np.array_equal(S.covered(off, n), np.ones(n, dtype=bool))
