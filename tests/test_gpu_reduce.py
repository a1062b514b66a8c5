"""Reduce by key (rsx_segmented_reduce_by_key, radix_sort_amd.segmented_reduce_by_key / reduce_by_key) on the GPU.

The referee is tests/_reduce_ref.py: unique_oracle's grouping, the reduction over its inverse map.  Keys, run offsets and counts are compared
bit for bit.  Reduced values: integers bit for bit (sums wrap); float sums of integer-valued inputs whose every partial sum is exactly
representable (float32: |v| <= 1024 and runs of at most 2^13; float64: |v| <= 2^20 and runs of at most 2^20, checked from the referee's
counts) bit for bit, since every association gives the same bits; float sums of general inputs within (count - 1) * u * sum|v| per run,
u = 2^-24 / 2^-53, the bound of any summation order; float min / max numerically equal or NaN on both sides.  Every output starts out holding
a sentinel that must survive past run_offsets[S] and ends in a guard band; values outside [off[0], off[S]) are NaN (floats) or huge
(integers) so that reading one shows.
"""
import ctypes as C

import numpy as np
import pytest

from _reduce_ref import OPS, reduce_oracle
from test_gpu_float_keys import UINT, random_bits
from test_gpu_segmented import DTYPES, _torch, dev, offsets_from
from test_gpu_unique import FILL, FILL32, FILL64, GUARD, LENGTHS

pytestmark = pytest.mark.gpu

VTYPES = [np.int32, np.int64, np.float32, np.float64]
KIND = {np.dtype(np.int32): 0, np.dtype(np.int64): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}
OPCODE = {"sum": 0, "min": 1, "max": 2}
UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
EXACT_CAPS = {np.dtype(np.float32): (1024, 1 << 13), np.dtype(np.float64): (1 << 20, 1 << 20)}     # (|v|, run length)


def run(rsx, x, v, off, op="sum", descending=False, consecutive=False, payload=True, counts=True, eng=None, stream=None):
    """One rsx_segmented_reduce_by_key through the Engine API, every output pre-filled with the sentinel and followed by a guard band.
    Returns ({name: host array of the whole buffer}, engine)."""
    t = _torch()
    n = x.size
    nseg = 1 if off is None else len(off) - 1
    k_in, v_in = dev(t, x), dev(t, v)
    o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
    sizes = {"keys": n * x.dtype.itemsize, "run_offsets": (nseg + 1) * 8, "values": n * v.dtype.itemsize}
    if counts:
        sizes["counts"] = n * 4
    bufs = {name: dev(t, np.concatenate([np.full(size, FILL, dtype=np.uint8), np.full(GUARD, 0xA5, dtype=np.uint8)])) for name, size in sizes.items()}
    if eng is None:
        eng = rsx.Engine(x.dtype, max(n, 1), payload=payload, descending=descending)
    if stream is not None:
        t.cuda.synchronize()
        eng.set_stream(stream)
    eng.segmented_reduce_by_key(k_in.data_ptr(), v_in.data_ptr(), n, None if o is None else o.data_ptr(), nseg, OPCODE[op], KIND[v.dtype],
                                bufs["keys"].data_ptr(), bufs["run_offsets"].data_ptr(), bufs["values"].data_ptr(),
                                bufs["counts"].data_ptr() if counts else None, consecutive=consecutive)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    out = {}
    types = {"keys": UINT[x.dtype], "run_offsets": np.uint64, "values": UINT[v.dtype], "counts": np.uint32}
    for name, buf in bufs.items():
        b = buf.cpu().numpy().view(np.uint8)
        assert np.all(b[sizes[name]:] == 0xA5), f"{name}: guard band written"
        out[name] = b[:sizes[name]].copy().view(types[name])
    return out, eng


def check(x, v, off, got, op="sum", descending=False, consecutive=False, how="exact", ref=None):
    """how (float sums only): "exact" demands equal bits after checking the caps that make every association exact, "bound" the
    any-order error bound."""
    ref = reduce_oracle(x, v, off, op, descending, consecutive) if ref is None else ref
    total = int(ref["run_offsets"][-1])
    assert np.array_equal(got["run_offsets"], ref["run_offsets"]), "run offsets differ"
    fill = lambda dt: UINT[dt](FILL64 & ((1 << (8 * dt.itemsize)) - 1))
    for name in ("keys", "counts"):
        if name not in got:
            continue
        bad = np.flatnonzero(got[name][:total] != ref[name])
        assert bad.size == 0, f"{name} differ at runs {bad[:8].tolist()} (of {bad.size}): {got[name][bad[:8]].tolist()} != {ref[name][bad[:8]].tolist()}"
        assert np.all(got[name][total:] == (fill(x.dtype) if name == "keys" else np.uint32(FILL32))), f"{name}: written past run_offsets[S]"
    assert np.all(got["values"][total:] == fill(v.dtype)), "values: written past run_offsets[S]"
    have = got["values"][:total].view(v.dtype)
    want = ref["values"]
    if v.dtype.kind == "i":
        bad = np.flatnonzero(have != want)
    elif op != "sum":
        bad = np.flatnonzero(~((have == want) | (np.isnan(have) & np.isnan(want))))
    elif how == "exact":
        vmax, rmax = EXACT_CAPS[v.dtype]
        lo, hi = (0, x.size) if off is None else (int(off[0]), int(off[-1]))
        assert total == 0 or (int(ref["counts"].max()) <= rmax and float(np.abs(v[lo:hi]).max()) <= vmax and np.all(v[lo:hi] == np.rint(v[lo:hi]))), \
            "the input of an exact comparison breaks the caps"
        bad = np.flatnonzero(have != want.astype(v.dtype))
    else:
        wide = want.dtype.type
        err = np.abs(have.astype(wide) - want)
        bound = (ref["counts"].astype(wide) - 1) * wide(UNIT[v.dtype]) * ref["abs"]
        bad = np.flatnonzero(~(err <= bound))
        worst = float(np.max(err / np.maximum(bound, np.finfo(wide).tiny))) if total else 0.0
        print(f"float sum {v.dtype.name}: {total} runs, longest {int(ref['counts'].max()) if total else 0}, worst error / bound = {worst:.3g}")
    assert bad.size == 0, f"values ({op}) differ at runs {bad[:8].tolist()} (of {bad.size}): {have[bad[:8]].tolist()} != {want[bad[:8]].tolist()}"
    return ref


def make_keys(maker, dtype, n, rng):
    if maker == "bits":
        return random_bits(dtype, n, rng)
    if maker == "few":
        return rng.integers(0, 3, n).astype(dtype)
    if maker == "one":
        return np.full(n, 7, dtype=dtype)
    if maker == "perm":
        return rng.permutation(n).astype(dtype)
    return np.sort(rng.integers(0, 500, n)).astype(dtype)


def make_values(vt, n, rng, op, off=None, general=False):
    """integer-valued floats for exact sums (or general ones), wrapping integers, floats with NaN and infinities for min / max (no zero
    at all, so that -0.0 and +0.0 never meet in a run); NaN / huge outside [off[0], off[S])"""
    vt = np.dtype(vt)
    if vt.kind == "i":
        info = np.iinfo(vt)
        v = rng.integers(info.min, info.max, n, dtype=vt, endpoint=True)
    elif op == "sum" and general:
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(vt)
    elif op == "sum":
        v = rng.integers(-EXACT_CAPS[vt][0], EXACT_CAPS[vt][0] + 1, n).astype(vt)
    else:
        v = rng.standard_normal(n).astype(vt)
        v[v == 0] = 1
        pick = rng.integers(0, 400, n)
        v[pick == 0] = np.nan
        v[pick == 1] = np.inf
        v[pick == 2] = -np.inf
    if off is not None:
        lo, hi = int(off[0]), int(off[-1])
        outside = np.nan if vt.kind == "f" else np.iinfo(vt).max
        v[:lo] = outside
        v[hi:] = outside
    return v


@pytest.mark.parametrize("consecutive", [False, True], ids=["sorted", "consecutive"])
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_matrix(rsx, dtype, descending, consecutive):
    """all six key types, both directions, both modes, on the ragged segments with off[0] = 3 and a tail after off[S]: every value type and op"""
    rng = np.random.default_rng(DTYPES.index(dtype) * 4 + descending * 2 + consecutive)
    off = offsets_from(LENGTHS, start=3)
    n = int(off[-1]) + 5
    eng = rsx.Engine(dtype, n, payload=True, descending=descending)
    plain = rsx.Engine(dtype, n, payload=False, descending=descending) if consecutive else None
    for maker in ("bits", "few", "one", "perm", "sorted"):
        x = make_keys(maker, dtype, n, rng)
        for vt in VTYPES:
            for op in OPS:
                # "one" and "few" make runs of up to 20011 elements: beyond float32's exact cap, so those sums get the bound
                general = np.dtype(vt) == np.float32 and maker in ("one", "few")
                v = make_values(vt, n, rng, op, off, general=general)
                got, _ = run(rsx, x, v, off, op, descending, consecutive, eng=eng)
                ref = check(x, v, off, got, op, descending, consecutive, how="bound" if general else "exact")
                if op == "max":                            # without the counts, and (consecutive mode) on an engine without a payload
                    got, _ = run(rsx, x, v, off, op, descending, consecutive, counts=False, eng=plain if consecutive else eng)
                    assert "counts" not in got
                    check(x, v, off, got, op, descending, consecutive, ref=ref)
    eng.sync()


@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, (1 << 20) + 3])
def test_null_offsets(rsx, n):
    """d_offsets == NULL: one segment on the flat chains"""
    rng = np.random.default_rng(n)
    for dtype, vt in ((np.uint32, np.float32), (np.int64, np.float64), (np.float32, np.int32), (np.uint64, np.int64)):
        x = rng.integers(0, max(n // 300, 2), n).astype(dtype)
        for cons in (False, True):
            for op in OPS:
                v = make_values(vt, n, rng, op)
                got, _ = run(rsx, x, v, None, op, False, cons)
                check(x, v, None, got, op, False, cons)


def test_all_equal_2p22_one_run_over_1024_tiles(rsx):
    """one run that the carry wave joins from 1024 tile partials; with a few offsets the same keys are a handful of long runs"""
    rng = np.random.default_rng(22)
    n = 1 << 22
    x = np.full(n, 0xABCD, dtype=np.uint32)
    M = 1 << 20
    short = np.array([3, 3 + M, 2 * M - 4, 3 * M - 4, 4 * M - 9], dtype=np.uint64)       # four runs within float64's exact cap
    for off in (None, np.array([5, 4096 * 3, 4096 * 3 + 1, 4096 * 700 + 17, n - 4096], dtype=np.uint64), short):
        f64 = "exact" if off is short else "bound"
        for cons in (False, True):
            for vt, op, how in ((np.float64, "sum", f64), (np.int32, "sum", None), (np.int64, "sum", None), (np.float32, "sum", "bound"),
                                (np.float32, "min", None), (np.float64, "max", None), (np.int64, "min", None)):
                v = make_values(vt, n, rng, op, off, general=(how == "bound"))
                if op != "sum" and np.dtype(vt).kind == "f":
                    v[np.isnan(v)] = 3.0                   # one NaN would be the answer of the whole run: keep the infinities only ...
                    if off is not None:
                        v[:int(off[0])] = np.nan
                        v[int(off[-1]):] = np.nan
                got, _ = run(rsx, x, v, off, op, False, cons)
                check(x, v, off, got, op, False, cons, how=how)
        v = make_values(np.float32, n, rng, "min", off)    # ... and once with them
        got, _ = run(rsx, x, v, off, "min")
        check(x, v, off, got, "min")


def test_all_distinct(rsx):
    """every element a head: the reduced values are the values in key order"""
    rng = np.random.default_rng(3)
    n = (1 << 20) + 3
    for dtype in (np.uint32, np.int64):
        x = rng.permutation(n).astype(dtype)
        for vt in VTYPES:
            v = make_values(vt, n, rng, "sum")
            for cons in (False, True):
                got, _ = run(rsx, x, v, None, "sum", True, cons)
                ref = check(x, v, None, got, "sum", True, cons)
                assert int(ref["run_offsets"][-1]) == n


def test_2p16_distinct_values_at_2p24(rsx):
    rng = np.random.default_rng(16)
    n = 1 << 24
    x = rng.integers(0, 1 << 16, n).astype(np.uint32)
    for vt, how in ((np.float32, "exact"), (np.float32, "bound"), (np.int32, None)):
        v = make_values(vt, n, rng, "sum", general=(how == "bound"))
        got, _ = run(rsx, x, v, None, "sum")
        check(x, v, None, got, "sum", how=how)


def boundary_layout():
    """(keys, offsets): a run that starts in the last element of a tile, one that ends exactly at a tile boundary, runs crossing several
    tiles inside a segment that ends mid-tile, equal keys on both sides of a segment boundary"""
    T = 4096
    runs = [T - 1, 1 + T, 3 * T + 100, 5, T - 105, 2 * T, 7, 6 * T + 9, 1, 1, T - 2, 2 * T + 1, 300]
    x = np.repeat(np.arange(len(runs)) * 3 + 11, runs).astype(np.uint32)
    n = x.size
    ends = np.cumsum(runs)
    # segment boundaries: inside the 3T+100 run (mid-tile), at a run boundary that is a tile boundary, inside the 6T+9 run twice, and off[S] mid-tile
    off = np.array([0, ends[1] + T + 50, ends[5], ends[6] + 2 * T, ends[6] + 2 * T, ends[6] + 5 * T + 1, n - 123], dtype=np.uint64)
    return x, off


def test_runs_against_tile_and_segment_boundaries(rsx):
    """the runs of boundary_layout, with and without its offsets, sorted (from shuffled segments) and consecutive"""
    rng = np.random.default_rng(8)
    x, off = boundary_layout()
    n = x.size
    for cons in (False, True):
        for o in (off, None):
            xs = x.copy()
            if not cons and o is not None:                 # sorted mode: the same runs from shuffled segments
                for s in range(len(o) - 1):
                    a, b = int(o[s]), int(o[s + 1])
                    xs[a:b] = rng.permutation(xs[a:b])
            for vt in VTYPES:
                for op in ("sum", "min"):
                    general = np.dtype(vt) == np.float32 and op == "sum"          # runs beyond float32's exact cap
                    v = make_values(vt, n, rng, op, o, general=general)
                    got, _ = run(rsx, xs, v, o, op, False, cons)
                    check(xs, v, o, got, op, False, cons, how="bound" if general else "exact")


def test_2p20_segments_of_16(rsx):
    """many tiny segments.  The referee runs on the equivalent one-segment problem whose key is (segment, key): the same runs in the same
    order, without a million calls of np.unique"""
    rng = np.random.default_rng(20)
    nseg, L = 1 << 20, 16
    n = nseg * L
    x = rng.integers(0, 5, n).astype(np.uint32)
    off = (np.arange(nseg + 1) * L).astype(np.uint64)
    wide = (np.repeat(np.arange(nseg, dtype=np.uint64), L) << np.uint64(32)) | x.astype(np.uint64)
    for vt, op in ((np.float32, "sum"), (np.int32, "sum"), (np.float64, "max")):
        v = make_values(vt, n, rng, op)
        ref = reduce_oracle(wide, v, None, op)
        ref["keys"] = (ref["keys"] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        ref["run_offsets"] = np.searchsorted(ref["first"] // L, np.arange(nseg + 1)).astype(np.uint64)      # runs come segment by segment
        got, _ = run(rsx, x, v, off, op)
        check(x, v, off, got, op, ref=ref)


def test_general_float_sums_within_the_any_order_bound(rsx):
    rng = np.random.default_rng(77)
    off = offsets_from([70_000, 3, 0, 4097, 300_000, 12, 1 << 20], start=1)
    n = int(off[-1]) + 2
    for dtype in (np.int32, np.float64):
        x = rng.integers(0, 300, n).astype(dtype)
        for vt in (np.float32, np.float64):
            v = make_values(vt, n, rng, "sum", off, general=True)
            for cons in (False, True):
                got, _ = run(rsx, x, v, off, "sum", False, cons)
                check(x, v, off, got, "sum", False, cons, how="bound")


def test_float_sums_reproducible(rsx):
    """equal input, equal bits: the same call twice, a second engine of larger capacity, a side stream.  The index_add_ composition runs
    beside it; whether its result varied is printed, not asserted."""
    t = _torch()
    rng = np.random.default_rng(99)
    n = 1 << 22
    x = rng.integers(0, 1000, n).astype(np.uint32)
    off = np.array([0, 1 << 20, (1 << 20) + 5, n], dtype=np.uint64)
    for vt in (np.float32, np.float64):
        v = make_values(vt, n, rng, "sum", general=True)
        for o in (None, off):
            a, eng = run(rsx, x, v, o)
            check(x, v, o, a, how="bound")
            b, _ = run(rsx, x, v, o, eng=eng)
            c, _ = run(rsx, x, v, o, eng=rsx.Engine(np.uint32, 3 * n + 4099, payload=True))
            side = t.cuda.Stream()
            d, eng2 = run(rsx, x, v, o, stream=side.cuda_stream)
            eng2.sync()
            e, _ = run(rsx, x, v, o, consecutive=True)
            f, _ = run(rsx, x, v, o, consecutive=True, eng=rsx.Engine(np.uint32, 2 * n, payload=False))
            for name in a:
                assert np.array_equal(a[name], b[name]), ("second call", name)
                assert np.array_equal(a[name], c[name]), ("larger engine", name)
                assert np.array_equal(a[name], d[name]), ("side stream", name)
                assert np.array_equal(e[name], f[name]), ("consecutive, larger engine", name)
        keys, vals = dev(t, x), t.from_numpy(v).cuda()
        inv = t.unique(keys, return_inverse=True)[1]
        sums = [t.zeros(1000, dtype=vals.dtype, device="cuda").index_add_(0, inv, vals) for _ in range(2)]
        print(f"index_add_ of {n} {np.dtype(vt).name} values into 1000 slots, two runs: {'bits DIFFER' if not t.equal(sums[0], sums[1]) else 'equal bits this time'}")


def test_refusals(rsx):
    t = _torch()
    n = 1 << 12
    eng = rsx.Engine(np.uint32, n, payload=True)
    plain = rsx.Engine(np.uint32, n, payload=False)
    x = t.zeros(n + 4, dtype=t.int32, device="cuda")
    vals = t.ones(n + 4, dtype=t.float32, device="cuda")
    kout, vout, cnt = (t.zeros(n, dtype=t.int32, device="cuda") for _ in range(3))
    off = t.tensor([0, n], dtype=t.int64, device="cuda")
    uoff = t.zeros(2, dtype=t.int64, device="cuda")
    ok = lambda e, **kw: e.segmented_reduce_by_key(**{**dict(d_keys=x.data_ptr(), d_values=vals.data_ptr(), n=n, d_offsets=off.data_ptr(), num_segments=1,
                                                           op=rsx.REDUCE_SUM, value_kind=rsx.VALUE_FLOAT32, d_keys_out=kout.data_ptr(),
                                                           d_run_offsets_out=uoff.data_ptr(), d_values_out=vout.data_ptr(), d_counts_out=cnt.data_ptr()), **kw})
    for kw in (dict(d_keys=x.data_ptr() + 4),                                   # misaligned keys
               dict(d_values=vals.data_ptr() + 2),                              # misaligned values
               dict(d_values=vals.data_ptr() + 4, value_kind=rsx.VALUE_FLOAT64),
               dict(n=n + 1),                                                    # beyond capacity
               dict(d_values_out=vals.data_ptr()),                               # each overlap: values_out on values,
               dict(d_keys_out=x.data_ptr()),                                    # keys_out on keys,
               dict(d_counts_out=vout.data_ptr()),                               # two outputs,
               dict(d_values_out=kout.data_ptr() + 64),
               dict(d_values_out=off.data_ptr() - 8),                            # output on the offsets,
               dict(d_run_offsets_out=off.data_ptr()),
               dict(d_values=x.data_ptr()),                                      # two inputs,
               dict(d_keys_out=eng.result_device()[0]),                          # the engine's own buffers
               dict(d_values_out=eng.result_device()[0]),
               dict(d_values=eng.result_device()[0]),
               dict(d_values=eng.result_device()[1]),
               dict(d_run_offsets_out=uoff.data_ptr() + 4),                      # misaligned run offsets
               dict(d_values_out=vout.data_ptr() + 2),
               dict(d_keys_out=None), dict(d_run_offsets_out=None), dict(d_values_out=None), dict(d_values=None)):      # what is required
        with pytest.raises(rsx.RadixSortError) as ei:
            ok(eng, **kw)
        assert ei.value.status in (1, 7), kw
    for kw in (dict(), dict(d_counts_out=None), dict(d_offsets=None)):           # a sorted call on an engine without a payload
        with pytest.raises(rsx.RadixSortError) as ei:
            ok(plain, **kw)
        assert ei.value.status == 1 and "has_payload" in str(ei.value)
    lib = rsx.load_library()
    P = C.c_void_p
    call = lambda flags, op, kind: lib.rsx_segmented_reduce_by_key(eng._h, P(x.data_ptr()), P(vals.data_ptr()), n, P(off.data_ptr()), 1, flags, op, kind,
                                                                    P(kout.data_ptr()), P(uoff.data_ptr()), P(vout.data_ptr()), None)
    for flags, op, kind in ((2, 0, 2), (3, 0, 2), (1 << 31, 0, 2), (0, 3, 2), (0, 0xFFFFFFFF, 2), (0, 0, 4), (1, 2, 17)):      # unknown flag bits, op, value kind
        assert call(flags, op, kind) == 4
    # n == 0 and no segments: nothing is launched, nothing is written — the run offsets included
    uoff.fill_(-7)
    t.cuda.synchronize()
    ok(eng, n=0)
    ok(eng, num_segments=0)
    ok(eng, n=0, d_offsets=None)
    eng.sync()
    assert uoff.tolist() == [-7, -7]
    ok(plain, consecutive=True)                                                  # consecutive mode: any engine
    plain.sync()
    assert uoff.tolist() == [0, 1] and int(cnt[0]) == n and float(vout.view(t.float32)[0]) == n
    uoff.fill_(-7)
    ok(eng)
    eng.sync()
    assert uoff.tolist() == [0, 1] and int(cnt[0]) == n and float(vout.view(t.float32)[0]) == n
    with pytest.raises(rsx.RadixSortError):                                      # the result lives in the caller's buffers only
        eng.download()


@pytest.mark.parametrize("consecutive", [False, True], ids=["sorted", "consecutive"])
@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_reported_once(rsx, bad, consecutive):
    rng = np.random.default_rng(23)
    n = 40000
    x = rng.integers(0, 99, n).astype(np.uint32)
    v = make_values(np.float32, n, rng, "sum")
    off = np.array([0, 100, 5000, 4000 if bad == "decreasing" else n + 1, n], dtype=np.uint64)       # segment 2 is the first bad one
    eng = rsx.Engine(np.uint32, n, payload=True)
    got, _ = run(rsx, x, v, off, consecutive=consecutive, eng=eng)      # guard bands checked inside
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "segment 2 " in str(ei.value)
    eng.sync()                                                                   # reported once
    uoff = got["run_offsets"].astype(np.int64)
    assert np.all(np.diff(uoff) >= 0) and 0 <= uoff[0] and uoff[-1] <= n
    # the engine stays usable: a correct call right after gives correct results
    good = np.array([0, 3, 5000, 5001, 30000, n], dtype=np.uint64)
    got, _ = run(rsx, x, v, good, consecutive=consecutive, eng=eng)
    eng.sync()
    check(x, v, good, got, consecutive=consecutive)


@pytest.mark.parametrize("vname", ["int64", "float32"])
def test_helper_matches_unique_and_index_add(rsx, vname):
    t = _torch()
    g = t.Generator().manual_seed(5)
    vt = getattr(t, vname)
    for shape in [(), (1,), (5000,), (37, 211), (4, 5, 1000), (1 << 20,)]:
        keys = t.randint(-50, 50, shape, generator=g).to(t.int32).cuda()
        vals = t.randint(-1000, 1000, shape, generator=g).to(vt).cuda()          # integer-valued: the float64 sum below is exact and so is ours
        uk, inv, cnt = t.unique(keys, return_inverse=True, return_counts=True)
        want = t.zeros(uk.numel(), dtype=t.float64, device="cuda").index_add_(0, inv.reshape(-1), vals.reshape(-1).to(t.float64))
        gk, gs, gc = rsx.reduce_by_key(keys, vals, return_counts=True)
        assert t.equal(gk, uk) and t.equal(gc, cnt) and gc.dtype == t.int64 and gs.dtype == vt
        assert t.equal(gs.to(t.float64), want)
        gk2, gs2 = rsx.reduce_by_key(keys, vals)
        assert t.equal(gk2, uk) and t.equal(gs2, gs)
        for op, red in (("min", "amin"), ("max", "amax")):
            w = t.zeros(uk.numel(), dtype=vt, device="cuda").scatter_reduce_(0, inv.reshape(-1), vals.reshape(-1), red, include_self=False)
            assert t.equal(rsx.reduce_by_key(keys, vals, op=op)[1], w)
        if vt.is_floating_point:
            gk3, gm = rsx.reduce_by_key(keys, vals, op="mean")
            assert t.equal(gk3, uk) and t.equal(gm, gs / cnt.to(vt))
        ck, ci, cc = t.unique_consecutive(keys, return_inverse=True, return_counts=True)
        cw = t.zeros(ck.numel(), dtype=t.float64, device="cuda").index_add_(0, ci.reshape(-1), vals.reshape(-1).to(t.float64))
        rk, rs, rc = rsx.reduce_by_key(keys, vals, consecutive=True, return_counts=True)
        assert t.equal(rk, ck) and t.equal(rc, cc) and t.equal(rs.to(t.float64), cw)
    # non-contiguous and misaligned views of keys and values
    kb = t.randint(0, 9, (300, 64), generator=g).to(t.int32).cuda()
    vb = t.randint(-9, 9, (300, 64), generator=g).to(vt).cuda()
    for kv, vv in ((kb.t(), vb.t()), (kb[:, 1::3], vb[:, 1::3]), (kb.reshape(-1)[1:], vb.reshape(-1)[1:]), (kb.reshape(-1)[1:], vb.reshape(-1)[:-1])):
        uk, inv = t.unique(kv, return_inverse=True)
        want = t.zeros(uk.numel(), dtype=t.float64, device="cuda").index_add_(0, inv.reshape(-1), vv.reshape(-1).to(t.float64))
        gk, gs = rsx.reduce_by_key(kv, vv)
        assert t.equal(gk, uk) and t.equal(gs.to(t.float64), want)


def test_helper_segments_errors_and_side_stream(rsx):
    t = _torch()
    keys = t.tensor([9, 5, 3, 5, 3, 3, 7, 7, 7, 2, 2, 8, 1, 9], dtype=t.int32, device="cuda")
    vals = t.arange(1, 15, dtype=t.float32, device="cuda")
    off = t.tensor([1, 6, 6, 9, 9, 13, 13], dtype=t.int64, device="cuda")
    k, ro, s, c = rsx.segmented_reduce_by_key(keys, vals, off, return_counts=True)
    assert k.tolist() == [3, 5, 7, 1, 2, 8] and ro.tolist() == [0, 2, 2, 3, 3, 6, 6] and c.tolist() == [3, 2, 3, 1, 2, 1]
    assert s.tolist() == [14, 6, 24, 13, 21, 12] and c.dtype == ro.dtype == t.int64
    k, ro, m = rsx.segmented_reduce_by_key(keys, vals, off, op="mean", descending=True)
    assert k.tolist() == [5, 3, 7, 8, 2, 1] and m.tolist() == [3.0, float(np.float32(14) / np.float32(3)), 8.0, 12.0, 10.5, 13.0]
    k, ro, s = rsx.segmented_reduce_by_key(keys, vals.to(t.int64), off, op="max", consecutive=True)
    assert k.tolist() == [5, 3, 5, 3, 7, 2, 8, 1] and s.tolist() == [2, 3, 4, 6, 9, 11, 12, 13] and ro.tolist() == [0, 4, 4, 5, 5, 8, 8]
    with pytest.raises(rsx.RadixSortError):                                      # bad offsets raise
        rsx.segmented_reduce_by_key(keys, vals, t.tensor([0, 9, 4], dtype=t.int64, device="cuda"))
    assert rsx.segmented_reduce_by_key(keys, vals, off[:2])[2].tolist() == [14, 6]          # the engine stays usable
    x = t.randint(0, 1000, (1 << 18,), device="cuda", dtype=t.int32)
    w = t.randint(-100, 100, (1 << 18,), device="cuda").to(t.float32)
    for dt in (t.bfloat16, t.float16, t.bool):
        with pytest.raises(TypeError):
            rsx.reduce_by_key(x.to(dt), w)
    for dt in (t.bfloat16, t.float16, t.int16, t.bool):
        with pytest.raises(TypeError):
            rsx.reduce_by_key(x, w.to(dt))
    with pytest.raises(TypeError):
        rsx.reduce_by_key(x, x, op="mean")
    with pytest.raises(ValueError):
        rsx.reduce_by_key(x.cpu(), w)
    with pytest.raises(ValueError):
        rsx.reduce_by_key(x, w.cpu())
    with pytest.raises(ValueError):
        rsx.reduce_by_key(x, w[:-1])
    with pytest.raises(ValueError):
        rsx.reduce_by_key(x, w, op="prod")
    with pytest.raises(ValueError):
        rsx.segmented_reduce_by_key(x, w, t.tensor([0, 5], device="cuda", dtype=t.int32))
    uk, inv = t.unique(x, return_inverse=True)
    want = t.zeros(uk.numel(), dtype=t.float64, device="cuda").index_add_(0, inv, w.to(t.float64))
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        gk, gs = rsx.reduce_by_key(x, w)
    side.synchronize()
    assert t.equal(gk, uk) and t.equal(gs.to(t.float64), want)
    assert side.cuda_stream in {key[1] for key in rsx._SEG_ENGINES}
