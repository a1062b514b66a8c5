"""CPU checks of the reduce by key: header, exports, binding and the Python callables agree on rsx_segmented_reduce_by_key; the two forms of
the host referee agree with each other and with hand-made cases; and the call and the torch helpers fail loudly instead of working on the
CPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import _unique_ref as U
from _reduce_ref import OPS, model_sum, reduce_oracle, same_values, slow_reduce
from _unique_ref import FIELDS, flat_unique, unique_oracle
from test_gpu_float_keys import random_bits
from test_gpu_segmented import DTYPES, offsets_from
from test_segmented import HEADER

DEFINES = {"RSX_REDUCE_SUM": 0, "RSX_REDUCE_MIN": 1, "RSX_REDUCE_MAX": 2, "RSX_VALUE_INT32": 0, "RSX_VALUE_INT64": 1, "RSX_VALUE_FLOAT32": 2,
           "RSX_VALUE_FLOAT64": 3}


def test_symbol_in_header_exports_and_binding(rsx):
    raw = open(HEADER).read()
    for name, value in DEFINES.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), raw), name
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_reduce_by_key\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_reduce_by_key is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "const void* d_values", "uint64_t n", "const uint64_t* d_offsets",
                      "uint64_t num_segments", "uint32_t flags", "uint32_t op", "uint32_t value_kind", "void* d_keys_out",
                      "uint64_t* d_run_offsets_out", "void* d_values_out", "uint32_t* d_counts_out"]
    assert "rsx_segmented_reduce_by_key" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_reduce_by_key
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_reduce_by_key\b", out)
    for name in ("segmented_reduce_by_key", "reduce_by_key"):
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_reduce_by_key)
    assert (rsx.REDUCE_SUM, rsx.REDUCE_MIN, rsx.REDUCE_MAX) == (0, 1, 2)
    assert (rsx.VALUE_INT32, rsx.VALUE_INT64, rsx.VALUE_FLOAT32, rsx.VALUE_FLOAT64) == (0, 1, 2, 3)


def test_oracle_hand_made_cases():
    x = np.array([9, 5, 3, 5, 3, 3, 7, 7, 7, 2, 2, 8, 1, 9], dtype=np.uint32)
    # off[0] > 0; segments [1, 6) = 5 3 5 3 3, [6, 6), [6, 9) = 7 7 7, [9, 9), [9, 13) = 2 2 8 1, [13, 13): empty ones in the middle and last
    off = np.array([1, 6, 6, 9, 9, 13, 13], dtype=np.uint64)
    for form in (reduce_oracle, slow_reduce):
        for vt in (np.int32, np.int64, np.float32, np.float64):
            v = np.arange(1, 15).astype(vt)                  # positions 0 and 13 (values 1 and 14) lie outside every segment
            r = form(x, v, off, "sum")
            assert r["keys"].tolist() == [3, 5, 7, 1, 2, 8] and r["run_offsets"].tolist() == [0, 2, 2, 3, 3, 6, 6]
            assert r["counts"].tolist() == [3, 2, 3, 1, 2, 1]
            assert r["values"].tolist() == [3 + 5 + 6, 2 + 4, 7 + 8 + 9, 13, 10 + 11, 12]
            assert form(x, v, off, "min")["values"].tolist() == [3, 2, 7, 13, 10, 12]
            assert form(x, v, off, "max")["values"].tolist() == [6, 4, 9, 13, 11, 12]
            d = form(x, v, off, "sum", descending=True)
            assert d["keys"].tolist() == [5, 3, 7, 8, 2, 1] and d["values"].tolist() == [6, 14, 24, 12, 21, 13]
            c = form(x, v, off, "sum", consecutive=True)
            assert c["keys"].tolist() == [5, 3, 5, 3, 7, 2, 8, 1] and c["run_offsets"].tolist() == [0, 4, 4, 5, 5, 8, 8]
            assert c["values"].tolist() == [2, 3, 4, 5 + 6, 7 + 8 + 9, 10 + 11, 12, 13]
            assert form(x, v, off, "max", consecutive=True)["values"].tolist() == [2, 3, 4, 6, 9, 11, 12, 13]
            # equal keys on the two sides of a segment boundary stay two runs, in both modes; an empty first segment
            y = np.array([4, 4, 4, 4, 6], dtype=np.int64)
            w = np.array([1, 2, 4, 8, 16]).astype(vt)
            for cons in (False, True):
                b = form(y, w, np.array([0, 0, 2, 5], dtype=np.uint64), "sum", consecutive=cons)
                assert b["keys"].tolist() == [4, 4, 6] and b["run_offsets"].tolist() == [0, 0, 1, 3] and b["values"].tolist() == [3, 12, 16]
            # one segment (no offsets)
            e = form(np.full(7, 5, dtype=np.int32), np.arange(7).astype(vt), None, "sum")
            assert e["keys"].tolist() == [5] and e["values"].tolist() == [21] and e["counts"].tolist() == [7]
        # integer sums wrap in the value's own width
        big = form(np.zeros(3, dtype=np.uint32), np.array([2**31 - 1, 1, 5], dtype=np.int32), None, "sum")
        assert big["values"].tolist() == [-(2**31) + 5]
        big = form(np.zeros(2, dtype=np.uint32), np.array([-2**63, -1], dtype=np.int64), None, "sum")
        assert big["values"].tolist() == [2**63 - 1]
        # min / max return NaN if the run holds one; infinities are ordinary numbers
        z = np.array([1, 1, 1, 2, 2, 3], dtype=np.int32)
        f = np.array([1.0, np.nan, -2.0, np.inf, 5.0, -np.inf], dtype=np.float32)
        lo, hi = form(z, f, None, "min")["values"], form(z, f, None, "max")["values"]
        assert np.isnan(lo[0]) and np.isnan(hi[0]) and lo[1:].tolist() == [5.0, -np.inf] and hi[1:].tolist() == [np.inf, -np.inf]
        s = form(z, f.astype(np.float64), None, "sum")
        assert np.isnan(s["values"][0]) and s["values"][1] == np.inf and s["values"][2] == -np.inf


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_oracle_forms_agree_on_ragged_cases(dtype, descending):
    rng = np.random.default_rng(DTYPES.index(dtype) * 2 + descending)
    lens = [0, 1, 2, 255, 256, 257, 1024, 1025, 4096, 4097, 9000, 0, 3, 20011]
    off = offsets_from(lens, start=3)
    n = int(off[-1]) + 5
    makers = {"bits": lambda: random_bits(dtype, n, rng), "few": lambda: rng.integers(0, 3, n).astype(dtype), "one": lambda: np.full(n, 7, dtype=dtype),
              "sorted": lambda: np.sort(rng.integers(0, 500, n)).astype(dtype)}
    for vt in (np.int32, np.int64, np.float32, np.float64):
        if np.dtype(vt).kind == "i":
            info = np.iinfo(vt)
            v = rng.integers(info.min, info.max, n, dtype=vt, endpoint=True)          # sums that wrap
        else:
            v = rng.integers(-1024, 1025, n).astype(vt)                               # integer-valued: every order of a sum is exact
        maker = list(makers)[(DTYPES.index(dtype) + [np.int32, np.int64, np.float32, np.float64].index(vt)) % len(makers)]
        x = makers[maker]()
        for cons in (False, True):
            for op in OPS:
                a, b = reduce_oracle(x, v, off, op, descending, cons), slow_reduce(x, v, off, op, descending, cons)
                assert all(np.array_equal(a[f], b[f]) for f in FIELDS), (maker, cons, op)
                assert same_values(a["values"], b["values"]), (maker, cons, op)
                if "abs" in a:
                    assert np.array_equal(a["abs"], b["abs"])
        # what every sum satisfies: the runs of a segment add up to the segment (exact here)
        a = reduce_oracle(x, v, off, "sum", descending, False)
        for s in range(len(lens)):
            lo, hi = int(off[s]), int(off[s + 1])
            u0, u1 = int(a["run_offsets"][s]), int(a["run_offsets"][s + 1])
            if np.dtype(vt).kind == "f":
                assert float(a["values"][u0:u1].sum()) == float(v[lo:hi].astype(np.float64).sum())
            else:
                assert int(a["values"][u0:u1].astype(object).sum() - v[lo:hi].astype(object).sum()) % (1 << (8 * np.dtype(vt).itemsize)) == 0
    assert same_values(reduce_oracle(x[:5000], v[:5000])["values"], slow_reduce(x[:5000], v[:5000])["values"])


UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
EXACT_CAPS = {np.dtype(np.float32): (1024, 1 << 13), np.dtype(np.float64): (1 << 20, 1 << 20)}     # (|v|, run length): tests/test_gpu_reduce.py


def model_cases():
    """(keys, offsets, consecutive) on real 4096-key tiles: runs within float32's exact cap that cross tiles, begin and end on tile
    edges, segments with off[0] deep in the grid and off[S] before n, one segment, no segment"""
    rng = np.random.default_rng(41)
    T = U.TILE
    n, off, _ = U.deep_layout("mid")
    yield rng.integers(0, 50, n).astype(np.uint32), off, False
    runs = rng.choice([1, 2, 17, 300, T - 1, T, T + 1, 6000], size=400)
    runs = runs[:int(np.searchsorted(np.cumsum(runs), n)) + 1]
    assert runs.sum() >= n
    cons = np.repeat(np.arange(runs.size) % 7, runs)[:n].astype(np.uint32)
    yield cons, off, True
    n, off, _ = U.deep_layout("edge")
    yield cons[:n].astype(np.int64), off, True
    yield rng.integers(0, 9, 3 * T).astype(np.uint32), None, False
    yield cons[:2 * T + 5], None, True
    yield rng.integers(0, 30, 5000).astype(np.uint32), np.array([7, 7, 4096, 4096, 4990], dtype=np.uint64), False


def test_model_sum_equals_the_oracle_where_every_order_is_exact():
    """integer-valued inputs within EXACT_CAPS: every association gives the same bits, the written one included"""
    rng = np.random.default_rng(42)
    for x, off, cons in model_cases():
        g = flat_unique(x, off, False, cons)
        assert all(np.array_equal(g[f], unique_oracle(x, off, False, cons)[f]) for f in FIELDS)
        for vt in (np.float32, np.float64):
            vmax, rmax = EXACT_CAPS[np.dtype(vt)]
            v = rng.integers(-vmax, vmax + 1, x.size).astype(vt)
            assert int(g["counts"].max()) <= rmax
            want = reduce_oracle(x, v, off, "sum", False, cons)["values"]
            assert np.array_equal(reduce_oracle(x, v, off, "sum", False, cons, groups=g)["values"], want)
            got = model_sum(v, g["order"], g["heads"])
            assert got.dtype == np.dtype(vt) and np.array_equal(got, want.astype(vt)), (cons, vt)


def test_model_sum_within_the_any_order_bound_on_general_inputs():
    rng = np.random.default_rng(43)
    for x, off, cons in model_cases():
        g = flat_unique(x, off, False, cons)
        for vt in (np.float32, np.float64):
            v = (rng.standard_normal(x.size) * 10.0 ** rng.integers(-6, 7, x.size)).astype(vt)
            ref = reduce_oracle(x, v, off, "sum", False, cons, groups=g)
            got = model_sum(v, g["order"], g["heads"])
            wide = ref["values"].dtype.type
            err = np.abs(got.astype(wide) - ref["values"])
            assert np.all(err <= (ref["counts"].astype(wide) - 1) * wide(UNIT[np.dtype(vt)]) * ref["abs"]), (cons, vt)
            # and the association matters on such inputs: a plain left-to-right sum of a long run gives other bits somewhere
            if vt is np.float32 and int(ref["counts"].max()) > 1000:
                starts = np.concatenate([[0], np.cumsum(ref["counts"].astype(np.int64))])
                vs = v[g["order"]]
                plain = np.array([np.add.accumulate(vs[a:b], dtype=vt)[-1] for a, b in zip(starts[:-1], starts[1:])], dtype=vt)
                assert not np.array_equal(plain, got)


def test_model_sum_carry_over_70_tiles():
    """one run of 70 tiles and a bit that begins mid-tile: the second trip of the carry's lane fold (more than 64 leads) and every level of
    its tree.  Exact where every order is (integer-valued float64), within the any-order bound on general values."""
    rng = np.random.default_rng(45)
    T = U.TILE
    n = 75 * T + 11
    x = np.full(n, 2, dtype=np.uint32)
    x[:2000] = 0
    x[2000:2000 + 70 * T + 1000] = 1
    for off in (None, np.array([3, 1000, n - 5], dtype=np.uint64)):
        g = flat_unique(x, off, False, True)
        assert int(g["counts"].max()) == 70 * T + 1000 and g["heads"][g["counts"].argmax()] % T == 2000
        v = rng.integers(-(1 << 20), (1 << 20) + 1, n).astype(np.float64)
        want = reduce_oracle(x, v, off, "sum", False, True, groups=g)["values"]
        assert np.array_equal(model_sum(v, g["order"], g["heads"]), want.astype(np.float64))
        for vt in (np.float32, np.float64):
            v = (rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)).astype(vt)
            ref = reduce_oracle(x, v, off, "sum", False, True, groups=g)
            wide = ref["values"].dtype.type
            err = np.abs(model_sum(v, g["order"], g["heads"]).astype(wide) - ref["values"])
            assert np.all(err <= (ref["counts"].astype(wide) - 1) * wide(UNIT[np.dtype(vt)]) * ref["abs"]), vt
            # one dropped lead (a whole tile of the long run) would show: the bound is far below a tile's sum of magnitudes here
            lost = np.abs(v[2000 + 64 * T:2000 + 65 * T].astype(wide).sum())
            assert lost > 0


def test_model_sum_hand_built_tile():
    """one tile, heads at 0, 20 and 1000, written out by hand from the header comment of rsx_reduce.hpp"""
    rng = np.random.default_rng(44)
    for vt in (np.float32, np.float64):
        f = np.dtype(vt).type
        v = (rng.standard_normal(4096) * 10.0 ** rng.integers(-3, 4, 4096)).astype(vt)

        def fold(a):                                  # left to right
            r = a[0]
            for t in a[1:]:
                r = f(r + t)
            return r

        thread = [fold(v[16 * t:16 * t + 16]) for t in range(256)]          # a thread without a head: all 16

        def scan(p, l, s, k=5):
            """lane l of the Hillis-Steele scan after distances 1 .. 2^k over the lane partials p, begun afresh at lane s"""
            if k < 0:
                return p[l]
            d = 1 << k
            if l - d < s:                             # the lanes l-d+1 .. l reach back to s already: nothing is added
                return scan(p, l, s, k - 1)
            return f(scan(p, l - d, s, k - 1) + scan(p, l, s, k - 1))

        # run 0 = [0, 20): thread 0 whole, then the four elements of thread 1 before its head
        run0 = f(thread[0] + fold(v[16:20]))
        # run 1 = [20, 1000): thread 1 from its head on, the threads 2 .. 61 (lanes of wave 0, scanned from lane 1), thread 62 before its head
        p0 = [thread[0], fold(v[20:32])] + thread[2:62]
        run1 = f(scan(p0, 61, 1) + fold(v[992:1000]))
        # run 2 = [1000, 4096): it leaves the tile, so it is the tile's tail.  Wave 0 ends with lanes 62 (from its head on) and 63; the
        # totals of waves 1 and 2 follow left to right; then wave 3's lanes 0 .. 62 scanned, and thread 255 itself last
        p0 = thread[:62] + [fold(v[1000:1008]), thread[63]]
        before = f(f(scan(p0, 63, 62) + scan(thread[64:128], 63, 0)) + scan(thread[128:192], 63, 0))
        run2 = f(f(before + scan(thread[192:256], 62, 0)) + thread[255])
        got = model_sum(v, np.arange(4096), np.array([0, 20, 1000]))
        assert got.tolist() == [run0, run1, run2]
        # two more tiles of the same run: their leads joined by the carry's tree (lane 0 + lane 1), the tail on the left
        w = np.concatenate([v, v[::-1], v[5:] * f(3)])
        lead1, lead2 = model_sum(w[4096:8192], np.arange(4096), np.array([0]))[0], model_sum(np.concatenate([w[8192:], np.zeros(5, vt)]), np.arange(4096), np.array([0]))[0]
        got = model_sum(w, np.arange(w.size), np.array([0, 20, 1000]))
        assert got.tolist()[:2] == [run0, run1] and got[2] == f(run2 + f(lead1 + lead2))


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    # a null engine is refused, nothing is computed
    assert lib.rsx_segmented_reduce_by_key(None, None, None, 16, None, 1, 0, 0, 0, None, None, None, None) == 4
    torch = pytest.importorskip("torch")
    keys = torch.arange(10, dtype=torch.int32)
    vals = torch.ones(10, dtype=torch.float32)
    offsets = torch.tensor([0, 10], dtype=torch.int64)
    with pytest.raises(ValueError):              # host tensors: no CPU fallback
        rsx.segmented_reduce_by_key(keys, vals, offsets)
    with pytest.raises(ValueError):
        rsx.reduce_by_key(keys, vals, return_counts=True)
    with pytest.raises(ValueError):
        rsx.reduce_by_key(keys, vals, consecutive=True)
    with pytest.raises(ValueError):              # an unknown op
        rsx.reduce_by_key(keys, vals, op="prod")
    with pytest.raises(ValueError):              # shapes differ
        rsx.reduce_by_key(keys, vals[:9])
    with pytest.raises(TypeError):               # the mean of integers
        rsx.reduce_by_key(keys, keys, op="mean")
    with pytest.raises(TypeError):
        rsx.segmented_reduce_by_key(keys, keys.to(torch.int64), offsets, op="mean")
    with pytest.raises(TypeError):               # value and key types outside the supported ones
        rsx.reduce_by_key(keys, vals.to(torch.float16))
    with pytest.raises(TypeError):
        rsx.reduce_by_key(keys.to(torch.int16), vals)
    if not torch.cuda.is_available():
        with pytest.raises(rsx.RadixSortError) as ei:
            rsx.Engine(np.uint32, 16, payload=True).segmented_reduce_by_key(0, 0, 16, None, 1, rsx.REDUCE_SUM, rsx.VALUE_FLOAT32, 0, 0, 0)
        assert ei.value.status == 2              # INITIALIZATION_FAILED: no device, no silent CPU path
