"""Scan by key (rsx_segmented_scan, radix_sort_amd.segmented_scan / scan_by_key / cumsum) on the GPU.

The referee is tests/_scan_ref.py.  Integers, and float min / max, are compared exactly with scan_oracle (NaN on both sides counts as equal).
Float sums are held to model_scan, the order written at the top of rsx_scan_by_key.hpp, BIT FOR BIT, and independently to the bound of
any summation order: |out - exact| <= gamma_(m-1) * sum|v|, gamma_k = k u / (1 - k u), u = 2^-24 / 2^-53, m = the elements folded;
the referee's own rounding (m * eps_wide * sum|v|, wide = float64 / numpy's extended precision) is added, nothing measured is.  The output
starts out holding a sentinel that must survive outside [off[0], off[S]) and ends in a guard band; values outside that range are NaN
(floats) or huge (integers) so that reading one shows.  Every engine here has capacity 4096: the scan is not bound by it.
"""
import ctypes as C

import numpy as np
import pytest

from _scan_ref import OPS, TILE, UNIT, model_scan, restarts, scan_oracle, scan_terms
from test_gpu_float_keys import UINT
from test_gpu_segmented import _torch, dev, offsets_from
from test_gpu_unique import FILL, FILL64, GUARD
from test_scan import LENGTHS, RUNS, keys_of_runs

pytestmark = pytest.mark.gpu

VTYPES = [np.int32, np.int64, np.float32, np.float64]
KIND = {np.dtype(np.int32): 0, np.dtype(np.int64): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}
OPCODE = {"sum": 0, "min": 1, "max": 2}
CAP = 4096


def engine(rsx, keys=None, stream=None, capacity=CAP):
    eng = rsx.Engine(np.uint32 if keys is None else UINT[keys.dtype], capacity)
    if stream is not None:
        eng.set_stream(stream)
    return eng


def run(rsx, v, off=None, keys=None, op="sum", excl=False, eng=None, in_place=False, in_shift=0, out_shift=0):
    """One rsx_segmented_scan through the Engine API.  Out of place: the output is pre-filled with the sentinel and followed by a guard
    band.  In place: the values' own buffer.  in_shift / out_shift: the pointer handed over lies that many ELEMENTS past a 16-byte
    aligned one (in place: in_shift for both); the bytes before the output must survive like the guard after it.  Returns (the output's
    bits, engine)."""
    t = _torch()
    n = v.size
    nbytes = n * v.dtype.itemsize
    nseg = 1 if off is None else len(off) - 1
    pre_in = in_shift * v.dtype.itemsize
    pre_out = pre_in if in_place else out_shift * v.dtype.itemsize
    v_in = dev(t, np.concatenate([np.full(pre_in, 0x5A, dtype=np.uint8), v.view(np.uint8), np.full(GUARD, 0xA5, dtype=np.uint8)]))
    k_in = None if keys is None else dev(t, keys)
    o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
    out = v_in if in_place else dev(t, np.concatenate([np.full(pre_out, 0x5A, dtype=np.uint8), np.full(nbytes, FILL, dtype=np.uint8),
                                                       np.full(GUARD, 0xA5, dtype=np.uint8)]))
    assert v_in.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    if eng is None:
        eng = engine(rsx, keys)
    eng.segmented_scan(None if k_in is None else k_in.data_ptr(), v_in.data_ptr() + pre_in, n, None if o is None else o.data_ptr(), nseg, OPCODE[op],
                       KIND[v.dtype], out.data_ptr() + pre_out, exclusive=excl)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    b = out.cpu().numpy().view(np.uint8)
    assert np.all(b[:pre_out] == 0x5A), "bytes before the output written"
    assert np.all(b[pre_out + nbytes:] == 0xA5), "guard band written"
    return b[pre_out:pre_out + nbytes].copy().view(UINT[v.dtype]), eng


def sentinel(dt):
    return UINT[np.dtype(dt)](FILL64 & ((1 << (8 * np.dtype(dt).itemsize)) - 1))


def check(got, v, off=None, keys=None, op="sum", excl=False, ref=None, in_place=False):
    """exact comparison with the referee inside [off[0], off[S]); outside, the sentinel (in place: the input)"""
    n = v.size
    lo, hi = (0, n) if off is None else (int(off[0]), int(off[-1]))
    ref = scan_oracle(v, off, keys, op, excl) if ref is None else ref
    outside = np.concatenate([got[:lo], got[hi:]])
    keep = np.concatenate([v[:lo], v[hi:]]).view(UINT[v.dtype]) if in_place else sentinel(v.dtype)
    assert np.all(outside == keep), "written outside [off[0], off[S])"
    have, want = got[lo:hi].view(v.dtype), ref[lo:hi].astype(v.dtype)
    if v.dtype.kind == "f":
        bad = np.flatnonzero(~((have == want) | (np.isnan(have) & np.isnan(want))))
    else:
        bad = np.flatnonzero(have != want)
    assert bad.size == 0, f"{op} excl={excl}: differ at {(bad[:8] + lo).tolist()} (of {bad.size}): {have[bad[:8]].tolist()} != {want[bad[:8]].tolist()}"


def check_float_sum(got, v, off=None, keys=None, excl=False, what=""):
    """bit for bit model_scan; and every output inside the any-order bound around the exact prefix"""
    n = v.size
    lo, hi = (0, n) if off is None else (int(off[0]), int(off[-1]))
    assert np.all(np.concatenate([got[:lo], got[hi:]]) == sentinel(v.dtype)), "written outside [off[0], off[S])"
    model = model_scan(v, off, keys, excl).view(UINT[v.dtype])
    bad = np.flatnonzero(got[lo:hi] != model[lo:hi])
    assert bad.size == 0, f"{what}: bits differ from the written order at {(bad[:8] + lo).tolist()} (of {bad.size})"
    ref = scan_oracle(v, off, keys, "sum", excl)
    wide = ref.dtype.type
    m, mag = scan_terms(v, off, keys, excl)
    k = np.maximum(m - 1, 0).astype(wide)
    u = wide(UNIT[v.dtype])
    bound = k * u / (1 - k * u) * mag + m.astype(wide) * wide(np.finfo(wide).eps) * mag
    err = np.abs(got.view(v.dtype).astype(wide) - ref)[lo:hi]
    worst = float(np.max(err / np.maximum(bound[lo:hi], np.finfo(wide).tiny)))
    print(f"float sum {v.dtype.name} {what}: {hi - lo} outputs, longest fold {int(m.max())}, worst error / bound = {worst:.3g}")
    assert np.all(err <= bound[lo:hi]), f"{what}: beyond the any-order bound"


def make_values(vt, n, rng, op="sum", off=None, general=True):
    """wrapping integers; general floats for sums (or integer-valued ones); floats with NaN and infinities for min / max; NaN / huge
    outside [off[0], off[S])"""
    vt = np.dtype(vt)
    if vt.kind == "i":
        info = np.iinfo(vt)
        v = rng.integers(info.min, info.max, n, dtype=vt, endpoint=True)
    elif op == "sum" and general:
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(vt)
    elif op == "sum":
        v = rng.integers(-256, 257, n).astype(vt)
    else:
        v = rng.standard_normal(n).astype(vt)
        pick = rng.integers(0, 3000, n)
        v[pick == 0] = np.nan
        v[pick == 1] = np.inf
        v[pick == 2] = -np.inf
    if off is not None:
        outside = np.nan if vt.kind == "f" else np.iinfo(vt).max
        v[:int(off[0])] = outside
        v[int(off[-1]):] = outside
    return v


def ragged(rng, kdtype=None):
    """the issue's segment lengths with off[0] = 3 and a tail, and key runs whose restarts fall on, before and after tile and wave edges"""
    off = offsets_from(LENGTHS, start=3)
    n = int(off[-1]) + 5
    return n, off, None if kdtype is None else keys_of_runs(n, rng, kdtype, RUNS)


# -- exactness on integers --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kdtype", [None, np.uint32, np.uint64], ids=["nokeys", "u32keys", "u64keys"])
@pytest.mark.parametrize("vt", [np.int32, np.int64], ids=lambda d: np.dtype(d).name)
def test_integers_exact(rsx, vt, kdtype):
    rng = np.random.default_rng(VTYPES.index(vt) * 3 + [None, np.uint32, np.uint64].index(kdtype))
    n, off, keys = ragged(rng, kdtype)
    eng = engine(rsx, keys)
    for o in (off, None):
        v = make_values(vt, n, rng, off=o)
        for op in OPS:
            for excl in (False, True):
                got, _ = run(rsx, v, o, keys, op, excl, eng=eng)
                check(got, v, o, keys, op, excl)
    eng.sync()


# -- the carry across tiles -------------------------------------------------------------------------------------------------------------

def carry_layouts():
    """(name, n, offsets, keys)"""
    T = TILE
    n = 75 * T + 11
    k = np.full(n, 2, dtype=np.uint32)
    k[:2000] = 0
    k[2000:2000 + 70 * T + 1000] = 1
    yield "one run of 70 tiles and a bit, begun mid-tile: the carry's second block of 64", n, np.array([3, 1000, n - 5], dtype=np.uint64), k
    yield "one segment of exactly 70 tiles", 70 * T, None, None
    # tile 1 has no restart between tiles 0 and 2 that do; the run from tile 2 ends exactly at the last element of tile 3; off[S] inside tile 5
    off = np.array([5, 100, 2 * T + 7, 4 * T, 5 * T + 99], dtype=np.uint64)
    yield "a tile without a restart between two with one", 6 * T, off, None
    k = np.zeros(6 * T, dtype=np.uint64)
    k[T - 1:] = 1                                                # a run that starts in the last element of a tile
    k[3 * T:] = 2                                                # and one that ends exactly at a tile's last element
    yield "runs against tile edges, off[S] inside a tile", 6 * T, np.array([0, 5 * T + 1], dtype=np.uint64), k


@pytest.mark.parametrize("case", range(4))
def test_carry(rsx, case):
    name, n, off, keys = list(carry_layouts())[case]
    rng = np.random.default_rng(100 + case)
    eng = engine(rsx, keys)
    v = make_values(np.int64, n, rng, off=off)
    for op, excl in (("sum", False), ("sum", True), ("max", False)):
        got, _ = run(rsx, v, off, keys, op, excl, eng=eng)
        check(got, v, off, keys, op, excl)
    for vt in (np.float32, np.float64):
        v = make_values(vt, n, rng, off=off)
        for excl in (False, True):
            got, _ = run(rsx, v, off, keys, "sum", excl, eng=eng)
            check_float_sum(got, v, off, keys, excl, what=name)
    eng.sync()


def test_several_tiles_per_workgroup(rsx):
    """The launch rule (capi_scan.inc): tiles per workgroup = ceil(tiles / (16 * CUs)), so a workgroup walks two tiles from
    16 * CUs + 1 tiles on: n = 4096 * 16 * CUs + 1 is the smallest such n (2^24 + 1 on 256 CUs).  Segments and runs cross from one
    workgroup's tiles into the next's; the float32 sum must still be model_scan's, which knows no workgroups."""
    t = _torch()
    cus = t.cuda.get_device_properties(0).multi_processor_count
    n = TILE * 16 * cus + 1
    rng = np.random.default_rng(7)
    lens = rng.integers(1, 3 * TILE, size=n // TILE)                           # segments of up to three tiles ...
    lens = lens[:int(np.searchsorted(np.cumsum(lens), n - 10))]
    off = offsets_from(list(lens) + [n - 10 - int(lens.sum())], start=3)       # ... and off[S] = n - 7, inside the last but one tile
    v = make_values(np.int32, n, rng, off=off)
    eng = engine(rsx)
    got, _ = run(rsx, v, off, None, "sum", eng=eng)
    check(got, v, off)
    v = make_values(np.float32, n, rng, off=off)
    got, _ = run(rsx, v, off, None, "sum", eng=eng)
    check_float_sum(got, v, off, what=f"{n} elements, two tiles per workgroup")
    eng.sync()


# -- floats -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kdtype", [None, np.uint32, np.uint64], ids=["nokeys", "u32keys", "u64keys"])
@pytest.mark.parametrize("vt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_float_sums_bits_and_bound(rsx, vt, kdtype):
    rng = np.random.default_rng(VTYPES.index(vt) * 3 + [None, np.uint32, np.uint64].index(kdtype) + 20)
    n, off, keys = ragged(rng, kdtype)
    eng = engine(rsx, keys)
    for o in (off, None):
        v = make_values(vt, n, rng, off=o)
        assert not np.any((v != 0) & (np.abs(v) < np.finfo(vt).tiny)), "no subnormals"
        for excl in (False, True):
            got, _ = run(rsx, v, o, keys, "sum", excl, eng=eng)
            check_float_sum(got, v, o, keys, excl, what="ragged")
    v = make_values(vt, n, rng, off=off, general=False)                          # integer-valued: every order is exact
    got, _ = run(rsx, v, off, keys, "sum", eng=eng)
    check(got, v, off, keys, "sum")
    eng.sync()


@pytest.mark.parametrize("vt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_float_min_max_and_nan(rsx, vt):
    """min / max compare exactly; a NaN poisons the rest of its run only"""
    rng = np.random.default_rng(31)
    n, off, keys = ragged(rng, np.uint32)
    eng = engine(rsx, keys)
    for op in ("min", "max"):
        v = make_values(vt, n, rng, op, off)
        ref = scan_oracle(v, off, keys, op)
        mask, lo, hi = restarts(n, off, keys)
        nan = np.isnan(ref[lo:hi])
        assert nan.any() and not nan.all() and not np.isnan(ref[lo:hi][mask[lo:hi] & ~np.isnan(v[lo:hi])]).any()      # a run starts clean
        for excl in (False, True):
            got, _ = run(rsx, v, off, keys, op, excl, eng=eng)
            check(got, v, off, keys, op, excl)
    eng.sync()


def test_float_keys_are_compared_by_bits(rsx):
    """-0.0 and +0.0 keys are two runs; NaN keys of equal bits are one run, of different bits two"""
    k = np.array([0.0, 0.0, -0.0, -0.0, np.nan, np.nan, 1.0, 1.0], dtype=np.float32)
    kb = k.view(np.uint32).copy()
    kb[5] ^= 1                                                  # another NaN
    kb = np.concatenate([kb, kb[:4], np.full(4, kb[4])])        # 0 0 | -0 -0 | nan | nan' | 1 1 | 0 0 | -0 -0 | nan nan nan nan
    v = np.arange(1, kb.size + 1, dtype=np.int64)
    got, _ = run(rsx, v, None, kb)
    assert got.view(np.int64).tolist() == [1, 3, 3, 7, 5, 6, 7, 15, 9, 19, 11, 23, 13, 27, 42, 58]
    k64 = np.array([0.0, -0.0, -0.0, np.nan, np.nan], dtype=np.float64)
    got, _ = run(rsx, np.arange(1, 6, dtype=np.int32), None, k64.view(np.uint64))
    assert got.view(np.int32).tolist() == [1, 2, 5, 4, 9]


# -- reproducibility --------------------------------------------------------------------------------------------------------------------

def test_float_sums_reproducible(rsx):
    """equal input, equal bits: twice on one engine, an engine of another capacity, a side stream, in place, and the exclusive result
    against the inclusive one shifted"""
    t = _torch()
    rng = np.random.default_rng(99)
    n, off, keys = ragged(rng, np.uint32)
    v = make_values(np.float32, n, rng, off=off)
    a, eng = run(rsx, v, off, keys)
    b, _ = run(rsx, v, off, keys, eng=eng)
    c, _ = run(rsx, v, off, keys, eng=engine(rsx, keys, capacity=3 * n + 4099))
    side = t.cuda.Stream()
    d, eng2 = run(rsx, v, off, keys, eng=engine(rsx, keys, stream=side.cuda_stream))
    eng2.sync()
    e, _ = run(rsx, v, off, keys, eng=eng, in_place=True)
    x, _ = run(rsx, v, off, keys, excl=True, eng=eng)
    assert np.array_equal(a, b), "second call"
    assert np.array_equal(a, c), "engine of another capacity"
    assert np.array_equal(a, d), "side stream"
    lo, hi = int(off[0]), int(off[-1])
    assert np.array_equal(a[lo:hi], e[lo:hi]), "in place"
    mask = restarts(n, off, keys)[0]
    inside = np.flatnonzero(~mask[lo + 1:hi]) + lo + 1
    assert np.array_equal(x[inside], a[inside - 1]), "excl[i + 1] == incl[i] inside a run"
    assert np.all(x[mask] == 0)
    eng.sync()


# -- in place; the engine's sort state --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vt", VTYPES, ids=lambda d: np.dtype(d).name)
def test_in_place(rsx, vt):
    rng = np.random.default_rng(VTYPES.index(vt) + 50)
    n, off, keys = ragged(rng, np.uint64)
    v = make_values(vt, n, rng, off=off)
    for o, k in ((off, keys), (None, None)):
        for excl in (False, True):
            out, eng = run(rsx, v, o, k, "sum", excl)
            inp, _ = run(rsx, v, o, k, "sum", excl, eng=eng, in_place=True)
            lo, hi = (0, n) if o is None else (int(o[0]), int(o[-1]))
            assert np.array_equal(out[lo:hi], inp[lo:hi])
            assert np.array_equal(inp[:lo], v[:lo].view(UINT[v.dtype])) and np.array_equal(inp[hi:], v[hi:].view(UINT[v.dtype]))


def test_sort_state_is_untouched_and_n_exceeds_capacity(rsx):
    t = _torch()
    rng = np.random.default_rng(61)
    eng = rsx.Engine(np.uint32, CAP)
    x = rng.integers(0, 1 << 32, CAP, dtype=np.uint32)
    eng.upload(x)
    eng.sort()
    n, off, _ = ragged(rng)
    assert n > CAP
    v = make_values(np.int64, n, rng, off=off)
    got, _ = run(rsx, v, off, None, "sum", eng=eng)
    check(got, v, off)
    assert eng.geometry().num_keys == CAP
    out = t.zeros(CAP, dtype=t.int32, device="cuda")
    eng.copy_result(out.data_ptr())
    eng.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.sort(x))
    assert np.array_equal(eng.download(), np.sort(x))


# -- capture and replay -----------------------------------------------------------------------------------------------------------------

def test_capture_and_replay(rsx):
    """the chain is linear and every launch is sized from n and the segment count: one captured call is replayed on new keys, values and
    offsets; the bits are those of an eager call"""
    t = _torch()
    rng = np.random.default_rng(70)
    n, off, keys = ragged(rng, np.uint32)
    nseg = len(off) - 1
    side = t.cuda.Stream()
    eng = engine(rsx, keys, stream=side.cuda_stream)
    v = make_values(np.float32, n, rng, off=off)
    kd, vd, od = dev(t, keys), dev(t, v), dev(t, off)
    out = dev(t, np.full(n * 4, FILL, dtype=np.uint8))

    def call():
        eng.segmented_scan(kd.data_ptr(), vd.data_ptr(), n, od.data_ptr(), nseg, OPCODE["sum"], KIND[v.dtype], out.data_ptr())

    call()                                                                   # eager: sizes the scratch of this n
    eng.sync()
    check_float_sum(out.cpu().numpy().view(np.uint32), v, off, keys, what="eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for rep in range(2):
        keys = keys_of_runs(n, rng, np.uint32, RUNS)
        lens = list(rng.permutation(LENGTHS))
        off = offsets_from(lens, start=rep)                                   # same segment count, ends within n
        v = make_values(np.float32, n, rng, off=off)
        kd.copy_(t.from_numpy(keys.view(np.int32)))
        vd.copy_(t.from_numpy(v.view(np.int32)))
        od.copy_(t.from_numpy(off.view(np.int64)))
        out.fill_(FILL - 256)
        graph.replay()
        t.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        eager, _ = run(rsx, v, off, keys)
        assert np.array_equal(got, eager), f"replay {rep} differs from the eager call"
        check_float_sum(got, v, off, keys, what=f"replay {rep}")
    del graph
    eng.sync()


# -- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals(rsx):
    t = _torch()
    n = 3 * TILE
    eng = rsx.Engine(np.uint32, n, payload=True)
    keys = t.zeros(n + 4, dtype=t.int32, device="cuda")
    vals = t.ones(2 * n + 4, dtype=t.float32, device="cuda")
    out = t.full((2 * n,), -7.0, dtype=t.float32, device="cuda")
    off = t.tensor([0, n, n, n], dtype=t.int64, device="cuda")
    lib = rsx.load_library()
    ok = lambda **kw: eng.segmented_scan(**{**dict(d_keys=keys.data_ptr(), d_values=vals.data_ptr(), n=n, d_offsets=off.data_ptr(), num_segments=1,
                                                   op=rsx.REDUCE_SUM, value_kind=rsx.VALUE_FLOAT32, d_values_out=out.data_ptr()), **kw})
    for kw in (dict(d_keys=keys.data_ptr() + 4),                                 # misaligned keys,
               dict(d_values=vals.data_ptr() + 2),                               # values,
               dict(d_values=vals.data_ptr() + 4, value_kind=rsx.VALUE_FLOAT64),
               dict(d_values_out=out.data_ptr() + 2),                            # output,
               dict(d_values_out=out.data_ptr() + 4, value_kind=rsx.VALUE_INT64),
               dict(d_offsets=off.data_ptr() + 4),                               # offsets
               dict(d_values_out=keys.data_ptr()),                               # the output on the keys,
               dict(d_values_out=off.data_ptr() - 8),                            # on the offsets,
               dict(d_values_out=off.data_ptr() + 8),
               dict(d_values_out=vals.data_ptr() + 4),                           # on the values without being them,
               dict(d_values_out=vals.data_ptr() + 4 * (n - 1)),
               dict(d_values=out.data_ptr() + 4 * (n - 1)),
               dict(d_values_out=eng.result_device()[0]),                        # anything on the engine's own buffers
               dict(d_values=eng.result_device()[0]),
               dict(d_values=eng.result_device()[1]),
               dict(d_keys=eng.result_device()[0]),
               dict(d_values=eng.result_device()[0], d_values_out=eng.result_device()[0]),
               dict(d_values=None), dict(d_values_out=None)):                    # what is required
        with pytest.raises(rsx.RadixSortError) as ei:
            ok(**kw)
        assert ei.value.status == 1 and "rsx_segmented_scan" in str(ei.value), kw
    P = C.c_void_p
    call = lambda flags, op, kind: lib.rsx_segmented_scan(eng._h, P(keys.data_ptr()), P(vals.data_ptr()), n, P(off.data_ptr()), 1, flags, op, kind, P(out.data_ptr()))
    for flags, op, kind in ((1, 0, 2), (3, 0, 2), (4, 0, 2), (1 << 31, 0, 2), (0, 3, 2), (0, 0xFFFFFFFF, 2), (0, 0, 4), (2, 2, 17)):
        assert call(flags, op, kind) == 4                                        # unknown flag bits (bit 0 included), op, value kind
        assert b"rsx_segmented_scan" in lib.rsx_last_error()
    # n == 0 and no segments: nothing is launched either
    ok(n=0)
    ok(num_segments=0)
    ok(n=0, d_offsets=None, d_keys=None)
    eng.sync()
    assert bool((out == -7.0).all()), "a refused call wrote something"
    ok()                                                                         # and the call these were variations of works,
    ok(d_values=out.data_ptr() + 4 * n, d_values_out=out.data_ptr() + 4 * n, d_keys=None, d_offsets=None)      # in place too
    eng.sync()
    assert out[:n].tolist() == list(range(1, n + 1)) and out[n:].tolist() == [-7.0 * i for i in range(1, n + 1)]


@pytest.mark.parametrize("keyed", [False, True], ids=["nokeys", "keys"])
@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_write_nothing_and_are_reported_once(rsx, bad, keyed):
    rng = np.random.default_rng(23)
    n = 40000
    keys = keys_of_runs(n, rng) if keyed else None
    v = make_values(np.float32, n, rng)
    off = np.array([0, 100, 5000, 4000 if bad == "decreasing" else n + 1, n], dtype=np.uint64)       # segment 2 is the first bad one
    eng = engine(rsx, keys)
    got, _ = run(rsx, v, off, keys, eng=eng)
    assert np.all(got == sentinel(np.float32)), "a call with bad offsets wrote something"
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "segment 2 " in str(ei.value)
    eng.sync()                                                                   # reported once
    good = np.array([0, 3, 5000, 5001, 30000, n], dtype=np.uint64)
    got, _ = run(rsx, v, good, keys, eng=eng)                                    # the engine stays usable
    eng.sync()
    check_float_sum(got, v, good, keys, what="after bad offsets")


# -- the torch helpers ------------------------------------------------------------------------------------------------------------------

def test_cumsum_matches_torch(rsx):
    t = _torch()
    g = t.Generator().manual_seed(5)
    for shape in [(1,), (5000,), (37, 211), (3, 4100), (4, 5, 1000), (2, 4097, 3)]:
        x = t.randint(-2**62, 2**62, shape, generator=g).cuda()
        for dim in range(-len(shape), len(shape)):
            got = rsx.cumsum(x, dim)
            assert got.dtype == t.int64 and t.equal(got, t.cumsum(x, dim)), (shape, dim)
    base = t.randint(-1000, 1000, (300, 64), generator=g).cuda()
    for view in (base.t(), base[:, 1::3], base.reshape(-1)[1:], base[5]):        # non-contiguous and misaligned views
        before = view.clone()
        for dim in range(view.dim()):
            assert t.equal(rsx.cumsum(view, dim), t.cumsum(view, dim))
        assert t.equal(view, before)                                             # the input is left alone
    x32 = t.full((3, 5), 2**30, dtype=t.int32, device="cuda")                    # int32 stays int32 and wraps; torch promotes to int64
    got = rsx.cumsum(x32, 1)
    assert got.dtype == t.int32 and t.equal(got, t.cumsum(x32, 1).to(t.int32))
    xf = t.randint(-100, 100, (64, 5000), generator=g).to(t.float32).cuda()      # integer-valued floats: exact in every order
    assert t.equal(rsx.cumsum(xf, -1), t.cumsum(xf.double(), -1).float())
    assert rsx.cumsum(t.zeros((0, 4), device="cuda"), 1).shape == (0, 4) and float(rsx.cumsum(t.tensor(3.0, device="cuda"), 0)) == 3.0
    assert all(k[2] in (4, 8) for k in rsx._SCAN_ENGINES) and all(e.capacity <= 4096 for e in rsx._SCAN_ENGINES.values())


def test_segmented_scan_and_scan_by_key_helpers(rsx):
    t = _torch()
    rng = np.random.default_rng(8)
    n, off, keys = ragged(rng, np.uint32)
    ot = dev(t, off)
    kt = dev(t, keys)
    for vt in (np.int64, np.float64):
        v = make_values(vt, n, rng, general=False)
        vtensor = t.from_numpy(v).cuda()
        for op in OPS:
            for excl in (False, True):
                got = rsx.segmented_scan(vtensor, ot, op=op, exclusive=excl)
                assert got.dtype == vtensor.dtype and np.array_equal(got.cpu().numpy(), scan_oracle(v, off, None, op, excl).astype(vt)), (op, excl)
                got = rsx.segmented_scan(vtensor, ot, op=op, exclusive=excl, keys=kt)
                assert np.array_equal(got.cpu().numpy(), scan_oracle(v, off, keys, op, excl).astype(vt)), (op, excl)
                got = rsx.scan_by_key(kt, vtensor, op=op, exclusive=excl)
                assert np.array_equal(got.cpu().numpy(), scan_oracle(v, None, keys, op, excl).astype(vt)), (op, excl)
        want = scan_oracle(v, off, keys, "sum").astype(vt)
        other = t.zeros_like(vtensor)
        assert rsx.segmented_scan(vtensor, ot, keys=kt, out=other) is other and np.array_equal(other.cpu().numpy(), want)
        assert np.array_equal(vtensor.cpu().numpy(), v)
        assert rsx.segmented_scan(vtensor, ot, keys=kt, out=vtensor) is vtensor and np.array_equal(vtensor.cpu().numpy(), want)      # in place
    # shapes, a side stream, no offsets
    k2 = t.tensor([[5, 5, 5], [5, 7, 7]], dtype=t.int64, device="cuda")
    v2 = t.arange(1, 7, dtype=t.float32, device="cuda").reshape(2, 3)
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        got = rsx.scan_by_key(k2, v2)
    side.synchronize()
    assert got.tolist() == [[1, 3, 6], [10, 5, 11]] and side.cuda_stream in {key[1] for key in rsx._SCAN_ENGINES}
    assert rsx.segmented_scan(v2.reshape(-1), None, op="max", exclusive=True).tolist() == [-np.inf, 1, 2, 3, 4, 5]
    # the error types
    x = t.arange(10, dtype=t.int32, device="cuda")
    w = t.ones(10, dtype=t.float32, device="cuda")
    o = t.tensor([0, 10], dtype=t.int64, device="cuda")
    for dt in (t.bfloat16, t.float16, t.int16, t.bool):
        with pytest.raises(TypeError):
            rsx.segmented_scan(w.to(dt), o)
        with pytest.raises(TypeError):
            rsx.cumsum(w.to(dt))
        with pytest.raises(TypeError):
            rsx.scan_by_key(x.to(dt), w)
    for call in (lambda: rsx.segmented_scan(w.cpu(), o), lambda: rsx.scan_by_key(x.cpu(), w), lambda: rsx.cumsum(w.cpu()),
                 lambda: rsx.segmented_scan(w, o.to(t.int32)), lambda: rsx.segmented_scan(w, o, op="prod"), lambda: rsx.scan_by_key(x[:9], w),
                 lambda: rsx.segmented_scan(w, o, out=w.double()), lambda: rsx.segmented_scan(w.reshape(2, 5), o)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(rsx.RadixSortError):                                      # bad offsets raise at the next call or synchronisation
        rsx.segmented_scan(w, t.tensor([0, 9, 4], dtype=t.int64, device="cuda"))
        t.cuda.synchronize()
        rsx.segmented_scan(w, o)
    assert rsx.segmented_scan(w, o).tolist() == list(range(1, 11))               # the engine stays usable
