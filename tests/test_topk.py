"""CPU checks of the segmented top-k: header, exports and binding agree on rsx_segmented_topk; the numpy oracle of
tests/test_gpu_topk.py gives the stable-sort prefix of every segment on hand-made cases (ties across the k boundary, segments shorter
than k, empty and invalid segments); and the call and the torch helpers fail loudly instead of selecting on the CPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import _topk_ref
from test_gpu_float_keys import UINT, enc
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


# -- the linear-time reference of the production-shape tests (tests/_topk_ref.py) ---------------------------------------------------

def _ragged_case(rng, dtype, kind):
    from test_gpu_float_keys import random_bits, special
    from test_gpu_segmented import offsets_from
    lens = [0, 1, 2, 5, 40, 255, 256, 257, 300, 1000, 1025, 3000, 4097, 9000, 0, 17]
    off = offsets_from(list(rng.permutation(lens)), start=int(rng.integers(0, 4)))
    n = int(off[-1]) + 3
    if kind == "random":
        x = random_bits(dtype, n, rng)
        x[rng.integers(0, n, n // 3)] = x[rng.integers(0, n, n // 3)]                    # ties
    elif kind == "few":
        x = rng.integers(0, 3, n).astype(UINT[np.dtype(dtype)]).view(dtype)          # ties across every k boundary
    elif kind == "equal":
        x = np.full(n, 7, dtype=UINT[np.dtype(dtype)]).view(dtype)
    elif kind == "special":
        x = special(dtype, n, rng)                                                       # ±0, ±inf, NaNs of both signs with payloads
    else:
        x = _topk_ref.digit_local(dtype, off, n, rng, kind, bool(rng.integers(0, 2)), k=300)
    return x, off


KEY_TYPES = [np.uint32, np.int32, np.float32, np.uint64, np.int64, np.float64]
REF_CASES = [(d, kind) for d in KEY_TYPES for kind in ["random", "few", "equal", "special", "window", "low", "straddle"]
             if kind != "special" or np.dtype(d).kind == "f"]


@pytest.mark.parametrize("dtype,kind", REF_CASES, ids=[f"{np.dtype(d).name}-{kind}" for d, kind in REF_CASES])
def test_fast_reference_equals_oracle(dtype, kind):
    rng = np.random.default_rng(REF_CASES.index((dtype, kind)))
    x, off = _ragged_case(rng, dtype, kind)
    bad = np.concatenate([off, [off[-1] - 3, off[-1] + 10]]).astype(np.uint64)      # a decreasing and a past-n segment at the end
    for o in (off, bad):
        for desc in (False, True):
            ref = _topk_ref.fast_topk(x, o, 1100, desc)
            for k in (1, 2, 300, 1024, 1100):
                wk, wi, written = topk_oracle(x, o, k, desc)
                gk, gi, gw = ref.at(k)
                assert np.array_equal(gw, written)
                assert np.array_equal(np.where(written, gk, 0), wk) and np.array_equal(np.where(written, gi, 0), wi), (k, desc)


@pytest.mark.parametrize("dtype", KEY_TYPES, ids=lambda d: np.dtype(d).name)
def test_order_words_decode(dtype):
    """dec inverts the engine's encoding, and the builders' order words land where they should: the pad-heavy keys are the pad key
    (encoded all ones in the call's order), digit-local keys differ from their segment's first key in one round's byte only."""
    rng = np.random.default_rng(3)
    u = UINT[np.dtype(dtype)]
    e = rng.integers(0, np.iinfo(u).max, 5000, dtype=u, endpoint=True)
    e[:4] = [0, 1, np.iinfo(u).max, np.iinfo(u).max >> 1]
    assert np.array_equal(enc(_topk_ref.dec(e, dtype)), e)
    ones = np.iinfo(u).max
    pad_asc = {"uint32": ones, "uint64": ones, "int32": 0x7FFFFFFF, "int64": 0x7FFFFFFFFFFFFFFF, "float32": 0x7FFFFFFF,
               "float64": 0x7FFFFFFFFFFFFFFF}[np.dtype(dtype).name]
    pad_desc = {"uint32": 0, "uint64": 0, "int32": 0x80000000, "int64": 0x8000000000000000, "float32": 0xFFFFFFFF,
                "float64": 0xFFFFFFFFFFFFFFFF}[np.dtype(dtype).name]
    off = np.array([0, 300, 5000], dtype=np.uint64)
    for desc, pad in ((False, pad_asc), (True, pad_desc)):
        x = _topk_ref.pad_heavy(dtype, off, 5000, rng, desc).view(u)
        assert np.count_nonzero(x == u(pad)) > 0.9 * 5000
        for variant in ("window", "low"):
            x = _topk_ref.digit_local(dtype, off, 5000, rng, variant, desc)
            o = enc(x)
            o = ~o if desc else o
            diff = int(np.bitwise_or.reduce(o[300:5000] ^ o[300]))       # the one large segment: round 0, or the lowest byte
            bits = np.dtype(u).itemsize * 8
            assert diff == (0xFF << (bits - 8) if variant == "window" else 0xFF)


def test_shapes_reach_their_paths():
    """Each production-shape layout of tests/test_gpu_topk_shapes.py still reaches what it is there for on 256 CUs (the mirror of
    seg_shape and topk_group_tiles in tests/_topk_ref.py; if those formulas change, this fails first)."""
    geo = {}
    for name, (_, make) in _topk_ref.SHAPES.items():
        off = make()
        geo[name] = _topk_ref.select_geometry(off, _topk_ref.shape_n(off))
    for name, g in geo.items():          # every shape: groups of several tiles, segments that begin inside a group
        assert g["gtiles"] >= 2 and g["switches"] > 0, (name, g)
    assert geo["1024x50257_f32"]["gtiles"] == 7 and geo["1024x50257_f32"]["switches"] == 879
    assert geo["1024x50257_f32"]["nlarge"] > 512                        # the pick kernel strides over segments
    g = geo["2048x5000_u64"]
    assert g["nlarge"] > 1024 and g["switches"] == 1365                 # ... and the final sort at k > 1024 (k = 4096 runs)
    assert g["tiles"] / g["nlarge"] < g["gtiles"]                       # groups hold two segment starts
    assert max(_topk_ref.SHAPE_KS) > 1024
    g = geo["64x151936_i64"]
    assert (151936 % _topk_ref.TILE) != 0 and g["tiles"] > 64 * 37 and g["switches"] > 0            # unaligned rows over 37 / 38 tiles
    off = _topk_ref.SHAPES["ragged_i32"][1]()
    lens = np.diff(off.astype(np.int64))
    assert off[0] % 2 == 1 and lens.max() <= 40000 and (lens[lens > 4096] >= 4097).all() and (lens <= 4096).any()
    # the vocabulary shapes of the torch-helper test
    g = _topk_ref.select_geometry(_topk_ref.rows(4096, 32000), 4096 * 32000)
    assert g["gtiles"] == 18 and g["switches"] == 3812
    g = _topk_ref.select_geometry(_topk_ref.rows(512, 50257), 512 * 50257)
    assert g["gtiles"] >= 2 and g["switches"] > 0
    # and the old top-k tests never did: the widest, 64 x 2^17, has no segment start inside a group
    assert _topk_ref.select_geometry(_topk_ref.rows(64, 1 << 17), 64 << 17)["switches"] == 0
