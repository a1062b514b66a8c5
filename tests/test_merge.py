"""CPU checks of the merge of sorted segments: header, exports, binding and the Python callables agree on rsx_segmented_merge; the two
forms of the host referee (tests/_merge_ref.py) agree with each other and with a hand-made case; the split rule reproduces the oracle's
prefix on every diagonal; the layouts of tests/test_gpu_merge.py reach the paths they are named for; and the call and the torch helpers
fail loudly instead of working on the CPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _merge_ref as M
from _merge_ref import diagonal_split, merge_oracle, merge_two_pointer, sorted_segments, thread_paths, tile_sources
from _search_ref import order_map
from test_search import HEADER_DTYPES as DTYPES
from test_search import header_text, random_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ragged_inputs(dt, rng, descending=False):
    """the ragged layout with sorted segments: every other segment from a narrow range (ties across the two sides), random spare keys
    outside the segments"""
    na, aoff, nb, boff = M.ragged_layout()
    a, b = random_keys(dt, na, rng), random_keys(dt, nb, rng)
    for s in range(len(M.A_LENGTHS)):
        if s % 2 == 1:
            a[aoff[s]:aoff[s + 1]] = random_keys(dt, M.A_LENGTHS[s], rng, narrow=True)
            b[boff[s]:boff[s + 1]] = random_keys(dt, M.B_LENGTHS[s], rng, narrow=True)
    return sorted_segments(a, aoff, descending), aoff, sorted_segments(b, boff, descending), boff


def test_symbol_in_header_exports_and_binding(rsx):
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_merge\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_merge is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_a", "const uint32_t* d_a_payload", "uint64_t na", "const uint64_t* d_a_offsets",
                      "const void* d_b", "const uint32_t* d_b_payload", "uint64_t nb", "const uint64_t* d_b_offsets", "uint64_t num_segments",
                      "uint32_t flags", "void* d_keys_out", "uint32_t* d_payload_out", "uint32_t* d_index_out", "uint64_t* d_out_offsets"]
    assert "rsx_segmented_merge" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_merge
    P, U = C.c_void_p, C.c_uint64
    assert fn.argtypes == [P, P, P, U, P, P, P, U, P, U, C.c_uint32, P, P, P, P]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_merge\b", out)
    for name in ("segmented_merge", "merge"):
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_merge)


def test_grid_constants_match_the_kernel_header():
    """tests/_merge_ref.py states the kernels' grid; the numbers are those of rsx_merge.hpp (which takes the family's tile)"""
    csrc = os.path.join(ROOT, "radix-sort_amd", "csrc")
    text = open(os.path.join(csrc, "rsx_merge.hpp")).read()
    assert re.search(r"kMergeThreads = kUniqThreads, kMergeKpt = kUniqKpt;", text)
    assert re.search(r"kMergeTileKeys = kUniqTileKeys;", text) and re.search(r"kMergeTileShift = kUniqTileShift;", text)
    uniq = open(os.path.join(csrc, "rsx_unique.hpp")).read()
    m = re.search(r"kUniqThreads = (\d+), kUniqKpt = (\d+);", uniq)
    assert (int(m.group(1)), int(m.group(2))) == (M.THREADS, M.KPT)
    seg = open(os.path.join(csrc, "rsx_segmented.hpp")).read()
    assert 1 << int(re.search(r"kSegTileShift = (\d+);", seg).group(1)) == M.TILE == M.THREADS * M.KPT
    assert "kUniqTileKeys = kSegTileKeys" in uniq and "kUniqTileShift = kSegTileShift" in uniq
    # the split rule and the tie rule as the referee has them
    assert "if (a(mid) <= b(d - 1u - mid))" in text and "uint32_t lo = d > nb ? d - nb : 0u, hi = min(d, na);" in text
    assert "const bool take_a = j >= nb || (i < na && xa <= xb);" in text
    # rsx_capi.hip includes the family after the compaction
    capi = open(os.path.join(csrc, "rsx_capi.hip")).read()
    assert capi.index('#include "capi_compact.inc"') < capi.index('#include "capi_merge.inc"')


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_referee_forms_agree(dt, descending):
    rng = np.random.default_rng(10 + DTYPES.index(dt) * 2 + descending)
    a, aoff, b, boff = ragged_inputs(dt, rng, descending)
    k1, i1, o1 = merge_oracle(a, aoff, b, boff, descending)
    k2, i2, o2 = merge_two_pointer(a, aoff, b, boff, descending)
    u = k1.dtype.str.replace("f", "u").replace("i", "u")
    assert np.array_equal(k1.view(u), k2.view(u)) and np.array_equal(i1, i2) and np.array_equal(o1, o2)
    assert o1[0] == 0 and o1[-1] == sum(M.A_LENGTHS) + sum(M.B_LENGTHS) == k1.size
    # ties across the two sides occur: some B key equals an A key of its segment
    ties = sum(np.intersect1d(order_map(a[aoff[s]:aoff[s + 1]]), order_map(b[boff[s]:boff[s + 1]])).size for s in range(len(M.A_LENGTHS)))
    assert ties > 50


def test_diagonal_split_reproduces_the_oracle_prefix():
    rng = np.random.default_rng(3)
    cases = [(np.sort(rng.integers(0, 30, 57).astype(np.uint32)), np.sort(rng.integers(0, 30, 41).astype(np.uint32))),
             (np.full(33, 7, dtype=np.uint32), np.full(20, 7, dtype=np.uint32)),                 # the tie rule at every diagonal
             (np.arange(0, 40, 2, dtype=np.uint32), np.arange(1, 41, 2, dtype=np.uint32)),
             (np.arange(10, dtype=np.uint32), np.array([], dtype=np.uint32)),
             (np.array([], dtype=np.uint32), np.arange(10, dtype=np.uint32)),
             (np.arange(100, 120, dtype=np.uint32), np.arange(20, dtype=np.uint32))]
    for a, b in cases:
        _, index, _ = merge_oracle(a, None, b, None)
        from_a = index < a.size
        for d in range(a.size + b.size + 1):
            i = diagonal_split(a, b, d)
            assert i == int(from_a[:d].sum()), (a.size, b.size, d)
            # the d outputs before the diagonal are exactly A[0, i) and B[0, d - i)
            assert sorted(index[:d].tolist()) == list(range(i)) + list(range(a.size, a.size + d - i))
    a, b = cases[1]
    assert [diagonal_split(a, b, d) for d in range(54)] == [min(d, 33) for d in range(54)]           # all of A before any equal B


def test_hand_made_example():
    a = np.array([9, 9, 1, 4, 4, 7, 5], dtype=np.int32)             # aoff = [2, 6, 6, 7]: [1 4 4 7] [] [5]
    b = np.array([8, 2, 4, 4, 9, 3, 6, 8], dtype=np.int32)          # boff = [1, 5, 7, 7]: [2 4 4 9] [3 6] []
    aoff, boff = [2, 6, 6, 7], [1, 5, 7, 7]
    for fn in (merge_oracle, merge_two_pointer):
        keys, index, ooff = fn(a, aoff, b, boff)
        assert ooff.tolist() == [0, 8, 10, 11]
        assert keys.tolist() == [1, 2, 4, 4, 4, 4, 7, 9, 3, 6, 5]
        assert index.tolist() == [0, 4, 1, 2, 5, 6, 3, 7, 0, 1, 0]          # the 4s of A (1, 2) before the 4s of B (5, 6)
    keys, index, _ = merge_oracle(np.array([-0.0, 0.0, np.nan], dtype=np.float32), None, np.array([-np.inf, -0.0, 0.0], dtype=np.float32), None)
    assert index.tolist() == [3, 0, 4, 1, 5, 2] and np.signbit(keys[:3]).all() and not np.signbit(keys[3:]).any()
    keys, index, _ = merge_oracle(np.array([5, 3, 3], dtype=np.uint32), None, np.array([7, 3, 0], dtype=np.uint32), None, descending=True)
    assert keys.tolist() == [7, 5, 3, 3, 3, 0] and index.tolist() == [3, 0, 1, 2, 4, 5]


def test_tile_sources_cover_the_inputs_in_order():
    rng = np.random.default_rng(5)
    a, aoff, b, boff = ragged_inputs(np.uint32, rng)
    keys, index, ooff = merge_oracle(a, aoff, b, boff)
    src = tile_sources(a, aoff, b, boff)
    assert len(src) == -(-keys.size // M.TILE)
    assert src[0][0] == aoff[0] and src[0][2] == boff[0] and src[-1][1] == aoff[-1] and src[-1][3] == boff[-1]
    for t, (a0, a1, b0, b1) in enumerate(src):
        assert a0 <= a1 and b0 <= b1 and (a1 - a0) + (b1 - b0) == min(M.TILE, keys.size - t * M.TILE)
        if t:
            assert (a0, b0) == (src[t - 1][1], src[t - 1][3])                   # contiguous from tile to tile
        got = np.sort(np.concatenate([a[a0:a1], b[b0:b1]]))
        assert np.array_equal(got, np.sort(keys[t * M.TILE:(t + 1) * M.TILE]))   # the tile's outputs are the merge of its sources


def test_gpu_layouts_reach_their_paths():
    kinds = lambda tiles: {p for _, paths in tiles for p in paths}
    na, aoff, nb, boff = M.ragged_layout()
    tiles = thread_paths(aoff, boff)
    assert {s for s, _ in tiles} == {True, False} and kinds(tiles) == {"serial", "runs", None}
    # 5000 segments of (0 .. 7) + (0 .. 7): every tile spans hundreds of segments and every live thread meets a boundary among its 16
    rng = np.random.default_rng(400)
    na, aoff, nb, boff = M.small_segments_layout(rng)
    tiles = thread_paths(aoff, boff)
    assert len(tiles) >= 8 and not any(s for s, _ in tiles)
    live = [p for _, paths in tiles for p in paths if p is not None]
    assert live.count("runs") >= 0.97 * len(live)
    # 300 segments of about 100 + 100: a mix
    na, aoff, nb, boff = M.medium_segments_layout(np.random.default_rng(401))
    live = [p for _, paths in thread_paths(aoff, boff) for p in paths if p is not None]
    assert min(live.count("runs"), live.count("serial")) >= 200
    # one segment: every tile is single, every thread serial; the last tile is ragged
    tiles = thread_paths(None, None, 4097, 100)
    assert all(s for s, _ in tiles) and kinds(tiles[:-1]) == {"serial"} and kinds(tiles[-1:]) == {"serial", None}
    # the staged ranges start at every residue of 16 bytes when the first offsets are shifted
    for width, dt in ((4, np.uint32), (2, np.uint64)):
        seen = set()
        for sa in range(width):
            for sb in range(width):
                a = np.arange(sa + 5000, dtype=dt)
                b = np.arange(sb + 5000, dtype=dt)
                src = tile_sources(a, [sa, sa + 5000], b, [sb, sb + 5000])
                seen |= {(x[0] % width, x[2] % width) for x in src}
        assert len(seen) == width * width


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    assert lib.rsx_segmented_merge(None, None, None, 16, None, None, None, 16, None, 1, 0, None, None, None, None) == 4       # a null engine is refused
    assert b"rsx_segmented_merge" in lib.rsx_last_error()
    torch = pytest.importorskip("torch")
    a = torch.arange(10, dtype=torch.int32)
    b = torch.arange(5, dtype=torch.int32)
    off = torch.tensor([0, 10], dtype=torch.int64)
    with pytest.raises(ValueError):              # host tensors: no CPU fallback
        rsx.merge(a, b)
    with pytest.raises(ValueError):
        rsx.merge(a.reshape(2, 5), b.reshape(1, 5).expand(2, 5))
    with pytest.raises(ValueError):
        rsx.segmented_merge(a, off, b, torch.tensor([0, 5], dtype=torch.int64))
    with pytest.raises(TypeError):               # the key type is looked at first
        rsx.merge(a, b.to(torch.int64))
    for bad in (torch.float16, torch.bfloat16, torch.bool):
        with pytest.raises(TypeError):
            rsx.merge(a.to(bad), b.to(bad))
    if not torch.cuda.is_available():
        with pytest.raises(rsx.RadixSortError) as ei:          # no device: the engine cannot be created, nothing is merged on the host
            rsx.Engine(np.uint32, 4096)
        assert ei.value.status == 2
