"""CPU checks of the set operations on sorted segments: header, exports, binding and the Python callables agree on rsx_segmented_set_op;
the two forms of the host referee (tests/_setop_ref.py) agree with each other, with numpy's set routines on inputs without duplicates,
with the per-key counts of std::set_* and with a hand-made case; and the call and the torch helpers fail loudly instead of working on the
CPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _merge_ref as M
import _setop_ref as R
from _search_ref import order_map, sort_engine_order
from _setop_ref import OPS, expected_count, key_counts, setop_oracle, setop_two_pointer
from test_merge import ragged_inputs
from test_search import HEADER_DTYPES as DTYPES
from test_search import header_text, random_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.ascontiguousarray(x).view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def test_symbol_in_header_exports_and_binding(rsx):
    raw = header_text()
    for name, value in (("INTERSECTION", 0), ("DIFFERENCE", 1), ("UNION", 2), ("SYMMETRIC_DIFFERENCE", 3)):
        assert re.search(rf"#define\s+RSX_SET_{name}\s+{value}\b", raw), name
        assert getattr(rsx, "SET_" + name) == value == getattr(R, name)          # the op constants: header, binding, referee
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_set_op\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_set_op is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_a", "const uint32_t* d_a_payload", "uint64_t na", "const uint64_t* d_a_offsets",
                      "const void* d_b", "const uint32_t* d_b_payload", "uint64_t nb", "const uint64_t* d_b_offsets", "uint64_t num_segments",
                      "uint32_t op", "uint32_t flags", "void* d_keys_out", "uint32_t* d_payload_out", "uint32_t* d_index_out",
                      "uint32_t* d_match_out", "uint64_t* d_out_offsets"]
    assert "rsx_segmented_set_op" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_set_op
    P, U = C.c_void_p, C.c_uint64
    assert fn.argtypes == [P, P, P, U, P, P, P, U, P, U, C.c_uint32, C.c_uint32, P, P, P, P, P]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_set_op\b", out)
    for name in ("segmented_set_op", "intersect_sorted", "difference_sorted", "union_sorted", "symmetric_difference_sorted"):
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_set_op)


def test_grid_constants_match_the_kernel_headers():
    """the set operations run on the merge's grid and with the merge's split and tie rule: rsx_setop.hpp takes them from rsx_merge.hpp"""
    csrc = os.path.join(ROOT, "radix-sort_amd", "csrc")
    merge = open(os.path.join(csrc, "rsx_merge.hpp")).read()
    assert re.search(r"kMergeThreads = kUniqThreads, kMergeKpt = kUniqKpt;", merge) and re.search(r"kMergeTileKeys = kUniqTileKeys;", merge)
    uniq = open(os.path.join(csrc, "rsx_unique.hpp")).read()
    m = re.search(r"kUniqThreads = (\d+), kUniqKpt = (\d+);", uniq)
    assert (int(m.group(1)), int(m.group(2))) == (M.THREADS, M.KPT) and M.TILE == M.THREADS * M.KPT
    text = open(os.path.join(csrc, "rsx_setop.hpp")).read()
    assert '#include "rsx_merge.hpp"' in text
    for name in ("kMergeThreads", "kMergeKpt", "kMergeTileKeys", "kMergeTileShift", "merge_diagonal(", "merge_stage(", "merge_segment_of("):
        assert name in text, name
    assert "const bool take_a = j >= nb || (i < na && xa <= xb);" in text           # the merge's tie rule
    assert re.search(r"kSetIntersection = 0u, kSetDifference = 1u, kSetUnion = 2u, kSetSymmetricDifference = 3u;", text)
    # one function evaluates the predicate for the count pass and for the write pass
    assert text.count("setop_tile_bits(sh, g, t, p0,") == 2 and text.count("__device__ __forceinline__ uint32_t setop_tile_bits(") == 1
    capi = open(os.path.join(csrc, "rsx_capi.hip")).read()
    assert capi.index('#include "capi_merge.inc"') < capi.index('#include "capi_setop.inc"')
    inc = open(os.path.join(csrc, "capi_setop.inc")).read()
    assert "merge_split_kernel<Key>" in inc and "kStatusCallSetop" in inc and "kStatusCallSetop" in capi


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_referee_forms_agree(dt, descending):
    rng = np.random.default_rng(20 + DTYPES.index(dt) * 2 + descending)
    a, aoff, b, boff = ragged_inputs(dt, rng, descending)
    # every other segment is drawn from a narrow range: keys with more copies in A than in B, and the other way round, both occur
    more_a = more_b = 0
    for s in range(len(M.A_LENGTHS)):
        ca, cb = key_counts(order_map(a[aoff[s]:aoff[s + 1]])), key_counts(order_map(b[boff[s]:boff[s + 1]]))
        more_a += sum(1 for k, m in ca.items() if 0 < cb.get(k, 0) < m)
        more_b += sum(1 for k, n in cb.items() if 0 < ca.get(k, 0) < n)
    assert more_a >= 5 and more_b >= 5                 # (of at most 40 distinct narrow keys a segment)
    for op in OPS:
        k1, i1, m1, o1 = setop_oracle(a, aoff, b, boff, op, descending)
        k2, i2, m2, o2 = setop_two_pointer(a, aoff, b, boff, op, descending)
        assert np.array_equal(bits(k1), bits(k2)) and np.array_equal(i1, i2) and np.array_equal(o1, o2), op
        assert (m1 is None) == (m2 is None) == (op != R.INTERSECTION) and (m1 is None or np.array_equal(m1, m2))
        assert o1[0] == 0 and o1[-1] == k1.size <= R.capacity(op, sum(M.A_LENGTHS), sum(M.B_LENGTHS)) and np.all(np.diff(o1) >= 0)


def test_equals_numpy_on_inputs_without_duplicates():
    rng = np.random.default_rng(31)
    for dt in (np.uint32, np.int64, np.float32):
        a = np.unique(rng.integers(0, 3000, 2000)).astype(dt)
        b = np.unique(rng.integers(1000, 4000, 1500)).astype(dt)
        for op, fn in ((R.INTERSECTION, np.intersect1d), (R.DIFFERENCE, np.setdiff1d), (R.UNION, np.union1d), (R.SYMMETRIC_DIFFERENCE, np.setxor1d)):
            for form in (setop_oracle, setop_two_pointer):
                keys, _, _, koff = form(a, None, b, None, op)
                assert np.array_equal(keys, fn(a, b)) and koff.tolist() == [0, keys.size], (op, form.__name__)


@pytest.mark.parametrize("descending", [False, True])
def test_per_key_counts_payload_index_and_match(descending):
    rng = np.random.default_rng(40 + descending)
    a, aoff, b, boff = ragged_inputs(np.int32, rng, descending)
    for op in OPS:
        keys, index, match, koff = setop_oracle(a, aoff, b, boff, op, descending)
        for s in range(len(M.A_LENGTHS)):
            sa, sb = a[aoff[s]:aoff[s + 1]], b[boff[s]:boff[s + 1]]
            ca, cb, got = key_counts(sa), key_counts(sb), key_counts(keys[koff[s]:koff[s + 1]])
            want = {k: expected_count(op, ca.get(k, 0), cb.get(k, 0)) for k in set(ca) | set(cb)}
            assert got == {k: c for k, c in want.items() if c}, (op, s)
            idx, seg = index[koff[s]:koff[s + 1]], keys[koff[s]:koff[s + 1]]
            from_a = idx < sa.size
            assert np.array_equal(sa[idx[from_a]], seg[from_a]) and np.array_equal(sb[idx[~from_a] - sa.size], seg[~from_a])
            e = order_map(seg, descending)
            assert np.all(e[1:] >= e[:-1])                                        # the merge's order
            assert np.all(np.diff(idx[from_a]) > 0) and np.all(np.diff(idx[~from_a]) > 0)          # each side in its own order
            if op in (R.INTERSECTION, R.DIFFERENCE):
                assert from_a.all()
            if match is not None:
                mt = match[koff[s]:koff[s + 1]]
                assert np.array_equal(sb[mt], seg) and np.all(np.diff(mt) > 0)


def test_hand_made_example():
    a = np.array([9, 1, 4, 4, 4, 7, 7, 5, 5], dtype=np.int32)       # aoff = [1, 7, 7, 9]: [1 4 4 4 7 7] [] [5 5]
    b = np.array([2, 4, 4, 7, 7, 7, 9, 3, 6, 5, 8], dtype=np.int32)     # boff = [0, 7, 9, 10]: [2 4 4 7 7 7 9] [3 6] [5]
    aoff, boff = [1, 7, 7, 9], [0, 7, 9, 10]
    want = {
        R.INTERSECTION: ([4, 4, 7, 7, 5], [1, 2, 4, 5, 0], [0, 4, 4, 5], [1, 2, 3, 4, 0]),
        R.DIFFERENCE: ([1, 4, 5], [0, 3, 1], [0, 2, 2, 3], None),
        R.UNION: ([1, 2, 4, 4, 4, 7, 7, 7, 9, 3, 6, 5, 5], [0, 6, 1, 2, 3, 4, 5, 11, 12, 0, 1, 0, 1], [0, 9, 11, 13], None),
        R.SYMMETRIC_DIFFERENCE: ([1, 2, 4, 7, 9, 3, 6, 5], [0, 6, 3, 11, 12, 0, 1, 1], [0, 5, 7, 8], None),
    }
    for op, (keys, index, koff, match) in want.items():
        for form in (setop_oracle, setop_two_pointer):
            k, i, m, o = form(a, aoff, b, boff, op)
            assert k.tolist() == keys and i.tolist() == index and o.tolist() == koff, (op, form.__name__)
            assert (m is None and match is None) or m.tolist() == match
    # bits decide: -0.0 and +0.0 are two keys, a NaN equals itself
    fa, fb = np.array([-0.0, 0.0, np.nan], dtype=np.float32), np.array([-np.inf, 0.0, np.nan], dtype=np.float32)
    k, i, m, _ = setop_oracle(fa, None, fb, None, R.INTERSECTION)
    assert i.tolist() == [1, 2] and m.tolist() == [1, 2] and not np.signbit(k[0]) and np.isnan(k[1])
    k, i, _, _ = setop_oracle(sort_engine_order(np.array([5, 3, 3], dtype=np.uint32), True), None, np.array([7, 3, 0], dtype=np.uint32), None,
                              R.SYMMETRIC_DIFFERENCE, descending=True)
    assert k.tolist() == [7, 5, 3, 0] and i.tolist() == [3, 0, 2, 5]


def test_empty_sides():
    a = np.arange(5, dtype=np.uint32)
    e = a[:0]
    for form in (setop_oracle, setop_two_pointer):
        for op in OPS:
            k, i, _, o = form(a, None, e, None, op)                      # B empty: union, difference, symmetric difference give A back
            assert k.tolist() == ([] if op == R.INTERSECTION else a.tolist()) and o.tolist() == [0, k.size]
            k, i, _, o = form(e, None, a, None, op)
            assert k.tolist() == (a.tolist() if op in (R.UNION, R.SYMMETRIC_DIFFERENCE) else []) and i.tolist() == list(range(k.size))
            assert form(e, None, e, None, op)[3].tolist() == [0, 0]


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    assert lib.rsx_segmented_set_op(None, None, None, 16, None, None, None, 16, None, 1, 0, 0, None, None, None, None, None) == 4    # a null engine is refused
    assert b"rsx_segmented_set_op" in lib.rsx_last_error()
    torch = pytest.importorskip("torch")
    a = torch.arange(10, dtype=torch.int32)
    b = torch.arange(5, dtype=torch.int32)
    off = torch.tensor([0, 10], dtype=torch.int64)
    helpers = (rsx.intersect_sorted, rsx.difference_sorted, rsx.union_sorted, rsx.symmetric_difference_sorted)
    for fn in helpers:
        with pytest.raises(ValueError):              # host tensors: no CPU fallback
            fn(a, b)
        with pytest.raises(ValueError):
            fn(a.reshape(2, 5), b)
        with pytest.raises(TypeError):               # the key type is looked at first
            fn(a, b.to(torch.int64))
        for bad in (torch.float16, torch.bfloat16, torch.bool):
            with pytest.raises(TypeError):
                fn(a.to(bad), b.to(bad))
    with pytest.raises(ValueError):
        rsx.segmented_set_op(a, off, b, torch.tensor([0, 5], dtype=torch.int64), "union")
    with pytest.raises(ValueError):                  # an unknown op, a match with another op, one payload without the other
        rsx.segmented_set_op(a, None, b, None, "minus")
    with pytest.raises(ValueError):
        rsx.segmented_set_op(a, None, b, None, 4)
    with pytest.raises(ValueError):
        rsx.segmented_set_op(a, None, b, None, "union", return_match=True)
    with pytest.raises(ValueError):
        rsx.intersect_sorted(a, b, payload_a=a)
    if not torch.cuda.is_available():
        with pytest.raises(rsx.RadixSortError) as ei:          # no device: the engine cannot be created, nothing is computed on the host
            rsx.Engine(np.uint32, 4096)
        assert ei.value.status == 2
