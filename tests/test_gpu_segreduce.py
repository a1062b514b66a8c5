"""Segmented reduction (rsx_segmented_reduce, radix_sort_amd.segmented_reduce / reduce_rows / amax / argmax ...) on the GPU.

The referee is tests/_segreduce_ref.py.  Integers, float min / max (NaN on both sides counts as equal) and every index are compared exactly
with reduce_oracle.  Float sums are held to model_sum, the order written at the top of rsx_segreduce.hpp, BIT FOR BIT, and independently
to the bound of any summation order: |out - exact| <= ((1 + u)^(m-1) - 1) * sum|v| (<= gamma_(m-1) * sum|v|, gamma_k = k u / (1 - k u),
which is what it simplifies to while k u < 1), u = 2^-24 / 2^-53, m = the segment's length; the referee's own rounding (m * eps_wide * sum|v|, wide = float64 / numpy's extended precision) is added, nothing
measured is.  The outputs start out holding a sentinel and lie between guard bands; values outside [off[0], off[S]) are NaN (floats) or
huge (integers) so that reading one shows.  Every engine here has capacity 4096 unless a test says otherwise: the call is not bound by it.
"""
import ctypes as C

import numpy as np
import pytest

import _segreduce_ref as R
from _segreduce_ref import OPCODE, OPS, TILE, UNIT, model_sum, offsets_from, reduce_oracle, reduce_terms
from test_gpu_float_keys import UINT
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, GUARD

pytestmark = pytest.mark.gpu

VTYPES = [np.int32, np.int64, np.float32, np.float64]
KIND = {np.dtype(np.int32): 0, np.dtype(np.int64): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}
CAP = 4096
ids_of = lambda d: np.dtype(d).name


def engine(rsx, stream=None, capacity=CAP):
    eng = rsx.Engine(np.uint32, capacity)
    if stream is not None:
        eng.set_stream(stream)
    return eng


def banded(t, nbytes, shift_bytes):
    """a device buffer: guard | shift | nbytes of sentinel | guard; returns (tensor, byte offset of the payload)"""
    pre = GUARD + shift_bytes
    return dev(t, np.concatenate([np.full(pre, 0x5A, dtype=np.uint8), np.full(nbytes, FILL, dtype=np.uint8), np.full(GUARD, 0xA5, dtype=np.uint8)])), pre


def unband(buf, pre, nbytes):
    b = buf.cpu().numpy().view(np.uint8)
    assert np.all(b[:pre] == 0x5A), "bytes before the output written"
    assert np.all(b[pre + nbytes:] == 0xA5), "guard band written"
    return b[pre:pre + nbytes].copy()


def run(rsx, v, off=None, op="sum", eng=None, in_shift=0, out_shift=0, want_values=True, nseg=None):
    """One rsx_segmented_reduce through the Engine API.  in_shift / out_shift: the pointers lie that many ELEMENTS past a 16-byte aligned
    address.  Returns (value bits or None, index words or None, engine)."""
    t = _torch()
    n = v.size
    vb = v.dtype.itemsize
    nseg = (1 if off is None else len(off) - 1) if nseg is None else nseg
    arg = op in ("argmin", "argmax")
    v_in = dev(t, np.concatenate([np.full(in_shift * vb, 0x5A, dtype=np.uint8), v.view(np.uint8), np.full(GUARD, 0xA5, dtype=np.uint8)]))
    o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
    assert GUARD % 16 == 0 and v_in.data_ptr() % 16 == 0
    vout, vpre = banded(t, nseg * vb, out_shift * vb) if want_values or not arg else (None, 0)
    iout, ipre = banded(t, nseg * 4, out_shift * 4) if arg else (None, 0)
    if eng is None:
        eng = engine(rsx)
    eng.segmented_reduce(v_in.data_ptr() + in_shift * vb if n else None, n, None if o is None else o.data_ptr(), nseg, OPCODE[op], KIND[v.dtype],
                         None if vout is None else vout.data_ptr() + vpre, None if iout is None else iout.data_ptr() + ipre)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    vals = None if vout is None else unband(vout, vpre, nseg * vb).view(UINT[v.dtype])
    idx = None if iout is None else unband(iout, ipre, nseg * 4).view(np.uint32)
    return vals, idx, eng


def same(have, want):
    if have.dtype.kind == "f":
        return (have.view(UINT[have.dtype]) == want.view(UINT[want.dtype])) | (np.isnan(have) & np.isnan(want))
    return have == want


def check_exact(vals, idx, v, off, op):
    """integers, float min / max, arg values and indices against the referee; an arg op's value keeps its bits"""
    want, widx = reduce_oracle(v, off, op)
    if vals is not None:
        have = vals.view(v.dtype)
        bad = np.flatnonzero(~same(have, want.astype(v.dtype)))
        assert bad.size == 0, f"{op} {v.dtype.name}: segments {bad[:8].tolist()} (of {bad.size}): {have[bad[:8]].tolist()} != {want[bad[:8]].tolist()}"
    if widx is not None:
        have = idx.view(np.int32).astype(np.int64)                 # 0xFFFFFFFF reads as -1, the referee's mark of an empty segment
        bad = np.flatnonzero(have != widx)
        assert bad.size == 0, f"{op} {v.dtype.name}: indices of segments {bad[:8].tolist()} (of {bad.size}): {have[bad[:8]].tolist()} != {widx[bad[:8]].tolist()}"
    else:
        assert idx is None


def check_float_sum(vals, v, off=None, what=""):
    """bit for bit model_sum; and every output inside the any-order bound around the exact sum"""
    model = model_sum(v, off).view(UINT[v.dtype])
    bad = np.flatnonzero(vals != model)
    assert bad.size == 0, f"{what}: bits differ from the written order in segments {bad[:8].tolist()} (of {bad.size})"
    ref = reduce_oracle(v, off, "sum")[0]
    wide = ref.dtype.type
    m, mag = reduce_terms(v, off)
    k = np.maximum(m - 1, 0).astype(wide)
    u = wide(UNIT[v.dtype])
    # (1 + u)^k - 1 <= gamma_k: the bound before its last simplification, because gamma_k is undefined once k u >= 1, as it is for the
    # 2^24 + 4097 float32 elements of one segment; below that it asks no less than gamma_k does
    bound = np.expm1(k * np.log1p(u)) * mag + m.astype(wide) * wide(np.finfo(wide).eps) * mag
    err = np.abs(vals.view(v.dtype).astype(wide) - ref)
    worst = float(np.max(err / np.maximum(bound, np.finfo(wide).tiny)))
    print(f"float sum {v.dtype.name} {what}: {len(m)} segments, longest {int(m.max())}, worst error / bound = {worst:.3g}")
    assert np.all(err <= bound), f"{what}: beyond the any-order bound"


def make_values(vt, n, rng, op="sum", off=None, ties=False):
    """wrapping integers; general floats for sums; for the other ops floats with NaN and infinities, or (ties) a handful of distinct
    values so that every extreme is attained many times; NaN / huge outside [off[0], off[S])"""
    vt = np.dtype(vt)
    if ties:
        v = rng.integers(-3, 4, n).astype(vt)
    elif vt.kind == "i":
        info = np.iinfo(vt)
        v = rng.integers(info.min, info.max, n, dtype=vt, endpoint=True)
    elif op == "sum":
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(vt)
    else:
        v = rng.standard_normal(n).astype(vt)
        pick = rng.integers(0, 3000, n)
        v[pick == 0] = np.nan
        v[pick == 1] = np.inf
        v[pick == 2] = -np.inf
    if off is not None:
        outside = np.nan if vt.kind == "f" else (np.iinfo(vt).max if op != "min" and op != "argmin" else np.iinfo(vt).min)
        v[:int(off[0])] = outside
        v[int(off[-1]):] = outside
    return v


def check_any(rsx, v, off, op, eng=None, what="", **kw):
    vals, idx, eng = run(rsx, v, off, op, eng=eng, **kw)
    if op == "sum" and v.dtype.kind == "f":
        check_float_sum(vals, v, off, what or "sum")
    else:
        check_exact(vals, idx, v, off, op)
    return eng


# -- all value kinds and ops on ragged segments -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("vt", VTYPES, ids=ids_of)
def test_ragged(rsx, vt, op):
    rng = np.random.default_rng(VTYPES.index(vt) * 10 + OPS.index(op))
    n, off = R.layout_ragged()
    assert off[0] > 0 and off[-1] < n
    eng = check_any(rsx, make_values(vt, n, rng, op, off), off, op)
    if op != "sum":
        check_any(rsx, make_values(vt, n, rng, op, off, ties=True), off, op, eng=eng)
    eng.sync()


# -- layouts ----------------------------------------------------------------------------------------------------------------------------

LAYOUTS = {
    "inside": R.layout_inside, "ends on edge": R.layout_ends_on_edge, "first and last": R.layout_first_last,
    "64 leads": lambda: R.layout_long(64, start=TILE - 1), "65 leads": lambda: R.layout_long(65, start=TILE - 1),
    "70 tiles": lambda: R.layout_long(70), "258 tiles": lambda: R.layout_long(258),
    "5000 empty": R.layout_many_empty, "empty at the end": R.layout_empty_at_end, "all empty": R.layout_all_empty,
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layouts(rsx, name):
    rng = np.random.default_rng(len(name))
    n, off = LAYOUTS[name]()
    eng = engine(rsx)
    check_any(rsx, make_values(np.float32, n, rng, "sum", off), off, "sum", eng=eng, what=name)
    check_any(rsx, make_values(np.float64, n, rng, "sum", off), off, "sum", eng=eng, what=name)
    check_any(rsx, make_values(np.int32, n, rng, "sum", off), off, "sum", eng=eng)
    check_any(rsx, make_values(np.float32, n, rng, "max", off), off, "max", eng=eng)
    check_any(rsx, make_values(np.int64, n, rng, "argmin", off, ties=True), off, "argmin", eng=eng)
    check_any(rsx, make_values(np.float64, n, rng, "argmax", off, ties=True), off, "argmax", eng=eng)
    eng.sync()


@pytest.mark.parametrize("rows", [False, True], ids=["one segment", "rows"])
def test_two_tiles_per_workgroup(rsx, rows):
    """n = 2^24 + 4097: 4098 tiles, two per workgroup on 256 CUs"""
    rng = np.random.default_rng(3 + rows)
    n, off = R.layout_two_tiles(rows)
    assert "two tiles per workgroup" in R.paths(n, off)
    v = make_values(np.float32, n, rng, "sum")
    eng = engine(rsx)
    vals, _, _ = run(rsx, v, off, "sum", eng=eng)
    check_float_sum(vals, v, off, "two tiles per workgroup")
    w = rng.integers(-1000, 1001, n).astype(np.int32)
    vals, idx, _ = run(rsx, w, off, "argmax", eng=eng)
    check_exact(vals, idx, w, off, "argmax")
    if not rows:                                                   # no offsets at all is the same segment
        vals2, idx2, _ = run(rsx, w, None, "argmax", eng=eng)
        assert np.array_equal(vals, vals2) and np.array_equal(idx, idx2)
    eng.sync()


@pytest.mark.parametrize("vt", VTYPES, ids=ids_of)
def test_nothing_to_read(rsx, vt):
    """n == 0 with three segments, and NULL offsets with n == 0: the identities are still written"""
    v = np.zeros(0, dtype=vt)
    eng = engine(rsx)
    for op in OPS:
        for off in (np.zeros(4, dtype=np.uint64), None):
            vals, idx, _ = run(rsx, v, off, op, eng=eng)
            check_exact(vals, idx, v, off, op)
            if idx is not None:
                assert np.all(idx == 0xFFFFFFFF)
    eng.sync()


# -- the arg ops ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vt", [np.float32, np.int64], ids=ids_of)
def test_arg_ties_across_thread_wave_and_tile_edges(rsx, vt):
    """the extreme sits at both sides of a thread edge, a wave edge and a tile edge, and in two tiles 69 apart: the first wins"""
    n = 72 * TILE
    off = np.array([5, n - 3], dtype=np.uint64)
    eng = engine(rsx)
    for pair in ((15, 16), (31, 32), (1023, 1024), (TILE - 1, TILE), (TILE + 5, 70 * TILE + 5), (6, n - 4), (2 * TILE, 2 * TILE + 1)):
        for op, ext in (("argmax", 9), ("argmin", -9)):
            v = np.zeros(n, dtype=vt)
            v[list(pair)] = ext
            v[:5] = 2 * ext                                        # outside the range: must not be seen
            v[n - 3:] = 2 * ext
            vals, idx, _ = run(rsx, v, off, op, eng=eng)
            assert int(idx[0]) == pair[0] - 5 and vals.view(v.dtype)[0] == ext, (pair, op, int(idx[0]))
    v = np.full(n, 4, dtype=vt)                                    # all equal: index 0 of every segment
    rows = offsets_from([1, 17, 4096, 4097, 69 * TILE, 100])
    assert rows[-1] <= n
    for op in ("argmax", "argmin"):
        vals, idx, _ = run(rsx, v, rows, op, eng=eng)
        assert np.all(idx == 0) and np.all(vals.view(v.dtype) == 4)
    eng.sync()


@pytest.mark.parametrize("vt", [np.float32, np.float64], ids=ids_of)
def test_arg_nan_and_signed_zero(rsx, vt):
    n = 3 * TILE
    eng = engine(rsx)
    for op, ext in (("argmax", 7.0), ("argmin", -7.0)):
        for nan_at in (10, 2 * TILE + 9):                          # a NaN before and after the extreme, which lies in the middle tile
            v = np.zeros(n, dtype=vt)
            v[TILE + 100] = ext
            v[nan_at] = np.nan
            v[nan_at + 33] = np.nan                                # among NaNs the first wins
            vals, idx, _ = run(rsx, v, None, op, eng=eng)
            assert int(idx[0]) == nan_at and np.isnan(vals.view(v.dtype)[0]), (op, nan_at)
        fill = vt(-1.0 if op == "argmax" else 1.0)                # zero is the extreme
        off = np.array([70, 2 * TILE], dtype=np.uint64)
        for first_negative in (True, False):
            y = np.full(n, fill, dtype=vt)
            y[77], y[78] = (-0.0, 0.0) if first_negative else (0.0, -0.0)
            y[TILE + 1] = 0.0
            vals, idx, _ = run(rsx, y, off, op, eng=eng)
            assert int(idx[0]) == 7, op                            # -0.0 and +0.0 tie: the first, with its own sign bit
            assert bool(np.signbit(vals.view(vt)[0])) == first_negative and vals.view(vt)[0] == 0
    eng.sync()


# -- min and max: identities and NaN ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vt", VTYPES, ids=ids_of)
def test_min_of_positives_max_of_negatives_later_tile(rsx, vt):
    """off[0] in a later tile, ragged ends: a dead lane's 0 would beat every value here"""
    rng = np.random.default_rng(77)
    off = offsets_from([3, 4096, 1, 5000, 0, 17], start=2 * TILE + 37)
    n = int(off[-1]) + 50
    pos = rng.integers(5, 1000, n).astype(vt)
    eng = engine(rsx)
    for op, v in (("min", pos), ("argmin", pos), ("max", -pos), ("argmax", -pos)):
        v = v.copy()
        v[:int(off[0])] = 0
        v[int(off[-1]):] = 0
        check_any(rsx, v, off, op, eng=eng)
    eng.sync()


def test_nan_carried_across_69_tiles(rsx):
    n = 70 * TILE
    off = np.array([9, n - 9], dtype=np.uint64)
    v = np.random.default_rng(8).standard_normal(n).astype(np.float32)
    v[100] = np.nan                                                # in the first tile: the join must carry it to the end
    eng = engine(rsx)
    for op in ("min", "max"):
        vals, _, _ = run(rsx, v, off, op, eng=eng)
        assert np.isnan(vals.view(np.float32)[0]), op
    v[100] = 0
    v[40 * TILE + 1] = np.nan                                      # in a whole tile in between
    for op in ("min", "max", "sum"):
        vals, _, _ = run(rsx, v, off, op, eng=eng)
        assert np.isnan(vals.view(np.float32)[0]), op
    eng.sync()


# -- pointers off 16-byte alignment -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vt", [np.float32, np.float64], ids=ids_of)
def test_misaligned_pointers(rsx, vt):
    rng = np.random.default_rng(12)
    n, off = R.layout_ragged()
    v = make_values(vt, n, rng, "sum", off)
    eng = engine(rsx)
    ref, _, _ = run(rsx, v, off, "sum", eng=eng)
    for in_shift, out_shift in ((1, 0), (0, 1), (1, 1), (3 if vt == np.float32 else 1, 2 if vt == np.float32 else 1)):
        vals, _, _ = run(rsx, v, off, "sum", eng=eng, in_shift=in_shift, out_shift=out_shift)
        assert np.array_equal(vals, ref), (in_shift, out_shift)    # the bits do not depend on the alignment
        w = make_values(vt, n, rng, "argmax", off)
        vals, idx, _ = run(rsx, w, off, "argmax", eng=eng, in_shift=in_shift, out_shift=out_shift)
        check_exact(vals, idx, w, off, "argmax")
    check_float_sum(ref, v, off, "aligned")
    eng.sync()


# -- reproducibility --------------------------------------------------------------------------------------------------------------------

def test_float_sums_reproducible_and_sort_state_untouched(rsx):
    """equal input, equal bits: twice on one engine, an engine of capacity 2^20, a side stream; and the sort result of the engine stays"""
    t = _torch()
    rng = np.random.default_rng(99)
    n, off = R.layout_long(70)
    off = np.concatenate([off, offsets_from(R.LENGTHS, start=int(off[-1]))[1:]])
    n = int(off[-1]) + 7
    v = make_values(np.float32, n, rng, "sum", off)
    eng = engine(rsx)
    x = rng.integers(0, 1 << 32, CAP, dtype=np.uint32)
    eng.upload(x)
    eng.sort()
    a, _, _ = run(rsx, v, off, eng=eng)
    b, _, _ = run(rsx, v, off, eng=eng)
    c, _, _ = run(rsx, v, off, eng=engine(rsx, capacity=1 << 20))
    side = t.cuda.Stream()
    d, _, eng2 = run(rsx, v, off, eng=engine(rsx, stream=side.cuda_stream))
    eng2.sync()
    assert np.array_equal(a, b), "second call"
    assert np.array_equal(a, c), "engine of another capacity"
    assert np.array_equal(a, d), "side stream"
    check_float_sum(a, v, off, "reproducible")
    assert n > CAP and eng.geometry().num_keys == CAP
    assert np.array_equal(eng.download(), np.sort(x))


def test_capture_and_replay(rsx):
    """one captured call is replayed after values and offsets were changed in place; the bits are those of an eager call"""
    t = _torch()
    rng = np.random.default_rng(70)
    n, off = R.layout_ragged()
    nseg = len(off) - 1
    side = t.cuda.Stream()
    eng = engine(rsx, stream=side.cuda_stream)
    v = make_values(np.float32, n, rng, "sum", off)
    vd, od = dev(t, v), dev(t, off)
    out = dev(t, np.full(nseg * 4, FILL, dtype=np.uint8))

    def call():
        eng.segmented_reduce(vd.data_ptr(), n, od.data_ptr(), nseg, OPCODE["sum"], KIND[v.dtype], out.data_ptr())

    call()                                                         # eager: sizes the scratch of this n
    eng.sync()
    check_float_sum(out.cpu().numpy().view(np.uint32), v, off, "eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for rep in range(2):
        off = offsets_from(list(rng.permutation(R.LENGTHS)), start=rep)      # same segment count, ends within n
        v = make_values(np.float32, n, rng, "sum", off)
        vd.copy_(t.from_numpy(v.view(np.int32)))
        od.copy_(t.from_numpy(off.view(np.int64)))
        out.fill_(FILL - 256)
        graph.replay()
        t.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        eager, _, _ = run(rsx, v, off)
        assert np.array_equal(got, eager), f"replay {rep} differs from the eager call"
        check_float_sum(got, v, off, f"replay {rep}")
    del graph
    eng.sync()


# -- errors -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ["sum", "argmax"])
@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_write_nothing_and_are_reported_once(rsx, bad, op):
    rng = np.random.default_rng(23)
    n = 40000
    v = make_values(np.float32, n, rng, op)
    off = np.array([0, 100, 5000, 4000 if bad == "decreasing" else n + 1, n, n], dtype=np.uint64)       # segment 2 is the first bad one
    eng = engine(rsx)
    vals, idx, _ = run(rsx, v, off, op, eng=eng)
    fill32 = np.uint32(int.from_bytes(bytes([FILL]) * 4, "little"))
    assert np.all(vals == fill32) and (idx is None or np.all(idx == fill32)), "a call with bad offsets wrote something"
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "rsx_segmented_reduce" in str(ei.value) and "segment 2 " in str(ei.value)
    eng.sync()                                                     # reported once
    good = np.array([0, 3, 5000, 5001, 30000, n], dtype=np.uint64)
    check_any(rsx, v, good, op, eng=eng, what="after bad offsets")  # the engine stays usable
    eng.sync()


def test_refusals(rsx):
    t = _torch()
    n = 3 * TILE
    eng = rsx.Engine(np.uint32, n, payload=True)
    vals = t.ones(2 * n + 4, dtype=t.float32, device="cuda")
    out = t.full((64,), -7.0, dtype=t.float32, device="cuda")
    iout = t.full((64,), -7, dtype=t.int32, device="cuda")
    off = t.tensor([0, n, n, n], dtype=t.int64, device="cuda")
    lib = rsx.load_library()
    base = dict(d_values=vals.data_ptr(), n=n, d_offsets=off.data_ptr(), num_segments=3, op=rsx.REDUCE_SUM, value_kind=rsx.VALUE_FLOAT32,
                d_values_out=out.data_ptr(), d_index_out=None)
    ok = lambda **kw: eng.segmented_reduce(**{**base, **kw})
    arg = dict(op=rsx.REDUCE_ARGMAX, d_index_out=iout.data_ptr())
    for kw in (dict(d_values=vals.data_ptr() + 2),                               # misaligned values,
               dict(d_values=vals.data_ptr() + 4, value_kind=rsx.VALUE_FLOAT64),
               dict(d_values_out=out.data_ptr() + 2),                            # output,
               dict(d_values_out=out.data_ptr() + 4, value_kind=rsx.VALUE_INT64),
               dict(d_offsets=off.data_ptr() + 4),                               # offsets,
               {**arg, "d_index_out": iout.data_ptr() + 2},                      # indices
               dict(d_values=None), dict(d_values_out=None),                     # what is required
               dict(op=rsx.REDUCE_ARGMAX), dict(op=rsx.REDUCE_ARGMIN),           # ... the indices of the arg ops
               dict(d_index_out=iout.data_ptr()), dict(op=rsx.REDUCE_MAX, d_index_out=iout.data_ptr()),      # and refused for the others
               dict(d_values_out=vals.data_ptr() + 4 * (n - 1)),                 # the output on the values,
               dict(d_values_out=off.data_ptr() + 8),                            # on the offsets,
               {**arg, "d_index_out": vals.data_ptr()},                          # the indices on the values,
               {**arg, "d_index_out": out.data_ptr() + 8},                       # on the other output
               dict(d_values_out=eng.result_device()[0]),                        # anything on the engine's own buffers
               dict(d_values=eng.result_device()[0]),
               dict(d_values=eng.result_device()[1]),
               {**arg, "d_values_out": None, "d_index_out": eng.result_device()[1]}):
        with pytest.raises(rsx.RadixSortError) as ei:
            ok(**kw)
        assert ei.value.status == 1 and "rsx_segmented_reduce" in str(ei.value), kw
    P = C.c_void_p
    call = lambda n_, off_, nseg, flags, op, kind: lib.rsx_segmented_reduce(eng._h, P(vals.data_ptr()), n_, off_, nseg, flags, op, kind, P(out.data_ptr()), None)
    o = P(off.data_ptr())
    for args in ((n, o, 3, 1, 0, 2), (n, o, 3, 2, 0, 2), (n, o, 3, 1 << 31, 0, 2),      # flags
                 (n, o, 3, 0, 5, 2), (n, o, 3, 0, 0xFFFFFFFF, 2), (n, o, 3, 0, 0, 4),       # op, value kind
                 (n, None, 0, 0, 0, 2), (n, None, 2, 0, 0, 2),                              # NULL offsets with S != 1
                 ((1 << 31) + 1, o, 3, 0, 0, 2), (n, o, 0xFFFFFFFF, 0, 0, 2)):              # n and S over the limits
        assert call(*args) == 4, args
        assert b"rsx_segmented_reduce" in lib.rsx_last_error()
    ok(num_segments=0)                                                           # no segments: nothing is launched
    eng.sync()
    assert bool((out == -7.0).all()) and bool((iout == -7).all()), "a refused call wrote something"
    ok()                                                                         # and the call these were variations of works,
    ok(**arg, d_values_out=None)                                                 # the arg form without values too
    eng.sync()
    assert out[:3].tolist() == [float(n), 0.0, 0.0] and bool((out[3:] == -7.0).all())
    assert iout[:3].tolist() == [0, -1, -1] and bool((iout[3:] == -7).all())


# -- the torch helpers ------------------------------------------------------------------------------------------------------------------

def gamma_close(t, got, x, dim):
    """|got - exact| <= gamma_(m-1) * sum|x| along dim, the exact sum taken in float64 (its own rounding, m * 2^-53 * sum|x|, added)"""
    m = x.shape[dim]
    u = UNIT[np.dtype(str(x.dtype).replace("torch.", ""))]
    mag = x.abs().double().sum(dim)
    bound = (m - 1) * u / (1 - (m - 1) * u) * mag + m * 2.0 ** -53 * mag
    return bool(((got.double() - x.double().sum(dim)).abs() <= bound).all())


@pytest.mark.parametrize("shape,dim", [((64, 1000), -1), ((3, 5, 257), 1)], ids=["64x1000", "3x5x257 dim 1"])
def test_row_helpers_match_torch(rsx, shape, dim):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(5)
    for dt in (t.int32, t.int64, t.float32):
        if dt.is_floating_point:
            x = t.randn(shape, device="cuda", generator=g, dtype=dt)          # (no ties, almost surely: torch's indices are then defined)
        else:
            total = int(np.prod(shape))
            x = (t.randperm(total, device="cuda", generator=g) - total // 2).to(dt).reshape(shape)
        assert t.equal(rsx.amax(x, dim), t.amax(x, dim)) and t.equal(rsx.amin(x, dim), t.amin(x, dim))
        assert t.equal(rsx.argmax(x, dim), t.argmax(x, dim)) and t.equal(rsx.argmin(x, dim), t.argmin(x, dim))
        assert t.equal(rsx.argmax(x, dim, keepdim=True), t.argmax(x, dim, keepdim=True))
        for mine, theirs in ((rsx.max_rows, t.max), (rsx.min_rows, t.min)):
            vals, idx = mine(x, dim)
            want = theirs(x, dim)
            assert t.equal(vals, want.values) and t.equal(idx, want.indices)
        for op in ("min", "max", "argmin", "argmax"):
            want = {"min": t.amin, "max": t.amax, "argmin": t.argmin, "argmax": t.argmax}[op](x, dim)
            assert t.equal(rsx.reduce_rows(x, op, dim), want)
        s = rsx.reduce_rows(x, "sum", dim)
        assert s.dtype == x.dtype and s.shape == t.sum(x, dim).shape
        if dt.is_floating_point:
            assert gamma_close(t, s, x, dim)
            mean = rsx.reduce_rows(x, "mean", dim, keepdim=True)
            assert mean.shape == t.mean(x, dim, keepdim=True).shape and t.equal(mean.squeeze(dim), s / x.shape[dim])
        else:
            assert t.equal(s, t.sum(x, dim, dtype=dt))             # int32 stays int32
    big = t.full((2, 3), 2 ** 31 - 1, dtype=t.int32, device="cuda")
    assert rsx.reduce_rows(big, "sum").tolist() == [2 ** 31 - 3, 2 ** 31 - 3]      # 3 * (2^31 - 1) wraps


def test_segmented_reduce_helper(rsx):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(6)
    lengths = [0, 5, 1, 0, 4097, 300, 0]
    off_h = np.concatenate([[2], 2 + np.cumsum(lengths)])
    off = t.tensor(off_h, dtype=t.int64, device="cuda")
    n = int(off_h[-1]) + 3
    for dt in (t.int64, t.float64):
        x = t.randn(n, device="cuda", generator=g, dtype=t.float64)
        x = (x * 1000).to(dt) if not dt.is_floating_point else x
        segs = [x[a:b] for a, b in zip(off_h[:-1], off_h[1:])]
        live = [i for i, s in enumerate(segs) if s.numel()]
        dead = [i for i, s in enumerate(segs) if not s.numel()]
        for op, fn in (("min", t.amin), ("max", t.amax)):
            got = rsx.segmented_reduce(x, off, op)
            assert got.shape == (len(lengths),) and got.dtype == dt
            assert all(got[i] == fn(segs[i]) for i in live)
            vals, idx = rsx.segmented_reduce(x, off, op, return_index=True)
            assert t.equal(vals, got) and idx.dtype == t.int64
            assert all(int(idx[i]) == -1 for i in dead) and all(segs[i][int(idx[i])] == got[i] for i in live)
            assert t.equal(rsx.segmented_reduce(x, off, "arg" + op), idx)
        s = rsx.segmented_reduce(x, off, "sum")
        assert all(float(s[i]) == 0 for i in dead)
        if dt.is_floating_point:
            assert all(gamma_close(t, s[i], segs[i], 0) for i in live)
            mean = rsx.segmented_reduce(x, off, "mean")
            assert all(bool(t.isnan(mean[i])) for i in dead)       # 0 / 0
            assert all(mean[i] == s[i] / segs[i].numel() for i in live)
            assert bool(t.isinf(rsx.segmented_reduce(x, off, "min")[0])) and float(rsx.segmented_reduce(x, off, "max")[0]) == -np.inf
        else:
            assert all(int(s[i]) == int(segs[i].sum()) for i in live)
    with pytest.raises(ValueError):
        rsx.segmented_reduce(x, off, "sum", return_index=True)
    with pytest.raises(ValueError):
        rsx.segmented_reduce(x.reshape(1, -1), off)
    with pytest.raises(ValueError):
        rsx.segmented_reduce(x, off.to(t.int32))
    for dtb in (t.float16, t.bfloat16, t.bool):
        with pytest.raises(TypeError):
            rsx.segmented_reduce(x.to(dtb), off)
        with pytest.raises(TypeError):
            rsx.amax(x.to(dtb).reshape(1, -1))
    with pytest.raises(TypeError):
        rsx.reduce_rows(x.to(t.int32), "mean")
    nc = t.randn(40, 60, device="cuda", generator=g)[:, ::2]       # a non-contiguous input is copied
    assert t.equal(rsx.argmax(nc, 0), t.argmax(nc, 0)) and t.equal(rsx.amax(nc, 1), t.amax(nc, 1))
