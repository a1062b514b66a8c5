"""Segmented unique (rsx_segmented_unique, radix_sort_amd.segmented_unique / unique / unique_consecutive) on the GPU.

The referee is numpy's np.unique per segment on the order-mapped keys (a != on neighbours in consecutive mode; tests/_unique_ref.py),
compared bit for bit: keys, run offsets, counts, first positions and the inverse map.  Every output starts out holding a sentinel that must
survive wherever the call may not write (per-run outputs past run_offsets[S], the inverse map outside [off[0], off[S])), and ends in a
guard band that must come back untouched.  Every comparison is exact equality.
"""
import numpy as np
import pytest

from _unique_ref import unique_oracle
from test_gpu_float_keys import UINT, random_bits, special
from test_gpu_segmented import DTYPES, _torch, dev, offsets_from

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xC3
FILL32 = 0xC3C3C3C3
FILL64 = 0xC3C3C3C3C3C3C3C3


def run(rsx, x, off, descending=False, consecutive=False, payload=True, want=("counts", "first", "inverse"), eng=None):
    """One rsx_segmented_unique through the Engine API, every output pre-filled with the sentinel and followed by a guard band.
    Returns ({name: host array of the whole buffer}, engine)."""
    t = _torch()
    n = x.size
    nseg = 1 if off is None else len(off) - 1
    ks = x.dtype.itemsize
    k_in = dev(t, x)
    o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
    sizes = {"keys": n * ks, "run_offsets": (nseg + 1) * 8, "counts": n * 4, "first": n * 4, "inverse": n * 4}
    bufs = {}
    for name, size in sizes.items():
        if name in ("keys", "run_offsets") or name in want:
            bufs[name] = dev(t, np.concatenate([np.full(size, FILL, dtype=np.uint8), np.full(GUARD, 0xA5, dtype=np.uint8)]))
    if eng is None:
        eng = rsx.Engine(x.dtype, max(n, 1), payload=payload, descending=descending)
    ptr = lambda name: bufs[name].data_ptr() if name in bufs else None
    eng.segmented_unique(k_in.data_ptr(), n, None if o is None else o.data_ptr(), nseg, ptr("keys"), ptr("run_offsets"), ptr("counts"), ptr("first"),
                         ptr("inverse"), consecutive=consecutive)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    out = {}
    types = {"keys": UINT[x.dtype], "run_offsets": np.uint64, "counts": np.uint32, "first": np.uint32, "inverse": np.uint32}
    for name, buf in bufs.items():
        b = buf.cpu().numpy().view(np.uint8)
        assert np.all(b[sizes[name]:] == 0xA5), f"{name}: guard band written"
        out[name] = b[:sizes[name]].copy().view(types[name])
    return out, eng


def check(x, off, got, descending=False, consecutive=False, ref=None):
    ref = unique_oracle(x, off, descending, consecutive) if ref is None else ref
    total = int(ref["run_offsets"][-1])
    assert np.array_equal(got["run_offsets"], ref["run_offsets"]), "run offsets differ"
    fill = {"keys": UINT[x.dtype](FILL64 & ((1 << (8 * x.dtype.itemsize)) - 1)), "counts": np.uint32(FILL32), "first": np.uint32(FILL32)}
    for name in ("keys", "counts", "first"):
        if name not in got:
            continue
        bad = np.flatnonzero(got[name][:total] != ref[name])
        assert bad.size == 0, f"{name} differ at runs {bad[:8].tolist()} (of {bad.size}): {got[name][bad[:8]].tolist()} != {ref[name][bad[:8]].tolist()}"
        assert np.all(got[name][total:] == fill[name]), f"{name}: written past run_offsets[S]"
    if "inverse" in got:
        want = np.where(ref["written"], ref["inverse"], np.uint32(FILL32))
        bad = np.flatnonzero(got["inverse"] != want)
        assert bad.size == 0, f"inverse differs at {bad[:8].tolist()} (of {bad.size}): {got['inverse'][bad[:8]].tolist()} != {want[bad[:8]].tolist()}"
    return ref


def make(maker, dtype, n, rng):
    if maker == "bits":
        return random_bits(dtype, n, rng)
    if maker == "few":
        return rng.integers(0, 3, n).astype(dtype)
    if maker == "one":
        return np.full(n, 7, dtype=dtype)
    if maker == "perm":
        return rng.permutation(n).astype(dtype)
    if maker == "sorted":
        return np.sort(rng.integers(0, 500, n)).astype(dtype)
    return special(dtype, n, rng)


LENGTHS = [0, 1, 2, 255, 256, 257, 1024, 1025, 4096, 4097, 9000, 0, 3, 20011]


@pytest.mark.parametrize("payload", [True, False], ids=["payload", "nopayload"])
@pytest.mark.parametrize("consecutive", [False, True], ids=["sorted", "consecutive"])
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_matrix(rsx, dtype, descending, consecutive, payload):
    rng = np.random.default_rng(DTYPES.index(dtype) * 8 + descending * 4 + consecutive * 2 + payload)
    off = offsets_from(LENGTHS, start=3)
    n = int(off[-1]) + 5
    positions = payload or consecutive           # sorted mode serves positions on payload engines only
    every = ("counts", "first", "inverse") if positions else ("counts",)
    eng = rsx.Engine(dtype, n, payload=payload, descending=descending)
    makers = ["bits", "few", "one", "perm", "sorted"] + (["special"] if np.dtype(dtype).kind == "f" else [])
    for maker in makers:
        x = make(maker, dtype, n, rng)
        got, _ = run(rsx, x, off, descending, consecutive, payload, every, eng=eng)
        ref = check(x, off, got, descending, consecutive)
        # every optional output also as NULL
        for want in [()] + [(w,) for w in every] + ([("first", "inverse")] if positions else []):
            got, _ = run(rsx, x, off, descending, consecutive, payload, want, eng=eng)
            assert set(got) == {"keys", "run_offsets"} | set(want)
            check(x, off, got, descending, consecutive, ref=ref)
    eng.sync()


def reconstructs(x, off, got):
    """values[run_offsets[s] + inverse[i]] is bitwise keys[i]; the counts of a segment sum to its length"""
    n = x.size
    off = np.array([0, n], dtype=np.int64) if off is None else np.asarray(off, dtype=np.int64)
    xu = x.view(UINT[x.dtype])
    seg = np.repeat(np.arange(len(off) - 1), np.diff(off))
    lo, hi = int(off[0]), int(off[-1])
    base = got["run_offsets"][seg].astype(np.int64)
    assert np.array_equal(got["keys"][base + got["inverse"][lo:hi]], xu[lo:hi])
    csum = np.concatenate([[0], np.cumsum(got["counts"][:int(got["run_offsets"][-1])].astype(np.int64))])
    sums = csum[got["run_offsets"][1:].astype(np.int64)] - csum[got["run_offsets"][:-1].astype(np.int64)]
    assert np.array_equal(sums, np.diff(off))


@pytest.mark.parametrize("n", [1, 4096, 4097, (1 << 20) + 5, (1 << 24) + 5])
def test_null_offsets_every_chain(rsx, n):
    """d_offsets == NULL: the flat sort chains (one tile, self-scan, the large-table chain), sorted and consecutive, two key widths"""
    rng = np.random.default_rng(n)
    for dtype in (np.uint32, np.int64):
        x = rng.integers(0, max(n // 3, 2), n).astype(dtype)
        for cons in (False, True):
            got, _ = run(rsx, x, None, False, cons, True)
            check(x, None, got, False, cons)
            reconstructs(x, None, got)
    x = random_bits(np.float32, n, rng)
    got, _ = run(rsx, x, None, True, False, False, ("counts",))
    check(x, None, got, True, False)


SHAPES = {
    "4096x4096": lambda rng: np.full(4096, 4096),
    "2p16_tiny": lambda rng: rng.integers(0, 65, 1 << 16),
    "large_among_tiny": lambda rng: np.concatenate([rng.integers(0, 9, 3000), [3_000_001], rng.integers(0, 9, 3000)]),
    "large_segments": lambda rng: np.array([50_000, 4096 * 9, 123_457, 0, 70_001, 4097]),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes(rsx, shape):
    rng = np.random.default_rng(len(shape))
    lens = SHAPES[shape](rng)
    off = offsets_from(lens, start=7)
    n = int(off[-1]) + 9
    x = rng.integers(0, 1000, n).astype(np.uint32)
    if shape == "large_segments":
        # a run of one key that spans several tiles and several large segments, and runs that end exactly on tile edges
        x[40_000:140_000] = 5
        x[4096 * 40:4096 * 42] = 77
    for cons in (False, True):
        got, eng = run(rsx, x, off, False, cons, True)
        check(x, off, got, False, cons)
        reconstructs(x, off, got)
        eng.sync()
    y = x.astype(np.uint64) << np.uint64(29)
    got, _ = run(rsx, y, off, True, False, True)
    check(y, off, got, True, False)


def test_two_calls_bitwise_equal(rsx):
    rng = np.random.default_rng(5)
    off = offsets_from([70_000, 3, 0, 4097, 300_000, 12], start=1)
    x = rng.integers(0, 5000, int(off[-1]) + 2).astype(np.int32)
    eng = rsx.Engine(np.int32, x.size, payload=True)
    a, _ = run(rsx, x, off, eng=eng)
    b, _ = run(rsx, x, off, eng=eng)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    check(x, off, a)


def test_refusals(rsx):
    t = _torch()
    n = 1 << 12
    eng = rsx.Engine(np.uint32, n, payload=True)
    plain = rsx.Engine(np.uint32, n, payload=False)
    x = t.zeros(n + 4, dtype=t.int32, device="cuda")
    vals, cnt, fst, inv = (t.zeros(n, dtype=t.int32, device="cuda") for _ in range(4))
    off = t.tensor([0, n], dtype=t.int64, device="cuda")
    uoff = t.zeros(2, dtype=t.int64, device="cuda")
    ok = lambda e, **kw: e.segmented_unique(**{**dict(d_keys=x.data_ptr(), n=n, d_offsets=off.data_ptr(), num_segments=1, d_keys_out=vals.data_ptr(),
                                                  d_run_offsets_out=uoff.data_ptr(), d_counts_out=cnt.data_ptr(), d_first_out=fst.data_ptr(),
                                                  d_inverse_out=inv.data_ptr()), **kw})
    for kw in (dict(d_keys=x.data_ptr() + 4),                                   # misaligned keys
               dict(n=n + 1),                                                    # beyond capacity
               dict(d_keys_out=x.data_ptr()),                                    # each overlap: output on input,
               dict(d_counts_out=vals.data_ptr()),                               # two outputs,
               dict(d_first_out=inv.data_ptr() + 64),
               dict(d_inverse_out=off.data_ptr() - 8),                           # output on the offsets,
               dict(d_run_offsets_out=off.data_ptr()),
               dict(d_keys_out=eng.result_device()[0]),                          # the engine's own buffers
               dict(d_run_offsets_out=uoff.data_ptr() + 4),                      # misaligned run offsets
               dict(d_keys_out=None), dict(d_run_offsets_out=None)):             # the required outputs
        with pytest.raises(rsx.RadixSortError):
            ok(eng, **kw)
    for kw in (dict(), dict(d_first_out=None), dict(d_inverse_out=None)):        # positions of a sorted call on a non-payload engine
        with pytest.raises(rsx.RadixSortError) as ei:
            ok(plain, **kw)
        assert ei.value.status == 1 and "has_payload" in str(ei.value)
    lib = rsx.load_library()
    import ctypes as C
    P = C.c_void_p
    for flags in (2, 3, 1 << 31):                                                # unknown flag bits
        assert lib.rsx_segmented_unique(eng._h, P(x.data_ptr()), n, P(off.data_ptr()), 1, flags, P(vals.data_ptr()), P(uoff.data_ptr()), None, None, None) == 4
    # n == 0 and no segments: nothing is launched, nothing is written — the run offsets included
    uoff.fill_(-7)
    t.cuda.synchronize()
    ok(eng, n=0)
    ok(eng, num_segments=0)
    ok(eng, n=0, d_offsets=None)
    eng.sync()
    assert uoff.tolist() == [-7, -7]
    ok(plain, d_first_out=None, d_inverse_out=None)                              # keys and counts: any engine
    ok(plain, consecutive=True)                                                  # consecutive mode: every output on any engine
    plain.sync()
    ok(eng)
    eng.sync()
    assert uoff.tolist() == [0, 1] and int(cnt[0]) == n
    with pytest.raises(rsx.RadixSortError):                                      # the result lives in the caller's buffers only
        eng.download()


@pytest.mark.parametrize("consecutive", [False, True], ids=["sorted", "consecutive"])
@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_reported_once(rsx, bad, consecutive):
    rng = np.random.default_rng(23)
    n = 40000
    x = rng.integers(0, 99, n).astype(np.uint32)
    off = np.array([0, 100, 5000, 4000 if bad == "decreasing" else n + 1, n], dtype=np.uint64)       # segment 2 is the first bad one
    eng = rsx.Engine(np.uint32, n, payload=True)
    got, _ = run(rsx, x, off, consecutive=consecutive, eng=eng)      # guard bands checked inside
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "segment 2 " in str(ei.value)
    eng.sync()                                                                   # reported once
    uoff = got["run_offsets"].astype(np.int64)
    assert np.all(np.diff(uoff) >= 0) and 0 <= uoff[0] and uoff[-1] <= n
    # the engine stays usable: a correct call right after gives correct results
    good = np.array([0, 3, 5000, 5001, 30000, n], dtype=np.uint64)
    got, _ = run(rsx, x, good, consecutive=consecutive, eng=eng)
    eng.sync()
    check(x, good, got, consecutive=consecutive)


TORCH_DTYPES = ["int32", "int64", "float32", "float64"]


@pytest.mark.parametrize("name", TORCH_DTYPES)
def test_helpers_match_torch(rsx, name):
    t = _torch()
    g = t.Generator().manual_seed(11)
    dt = getattr(t, name)
    for shape in [(), (0,), (1,), (5000,), (37, 211), (4, 5, 1000), (1 << 20,)]:
        x = t.randint(-50, 50, shape, generator=g).to(dt).cuda()             # floats without -0.0 / NaN
        if dt.is_floating_point:
            x = x * 0.5
            x = t.where(x == 0, t.zeros_like(x), x)                            # +0.0 only
        wv, wi, wc = t.unique(x, sorted=True, return_inverse=True, return_counts=True)
        gv, gi, gc = rsx.unique(x, return_inverse=True, return_counts=True)
        assert t.equal(gv, wv) and t.equal(gi, wi) and t.equal(gc, wc) and gi.shape == x.shape and gi.dtype == gc.dtype == t.int64
        assert t.equal(rsx.unique(x, sorted=False), wv)
        gv, gc = rsx.unique(x, return_counts=True)
        assert t.equal(gv, wv) and t.equal(gc, wc)
        wv, wi, wc = t.unique_consecutive(x, return_inverse=True, return_counts=True)
        gv, gi, gc = rsx.unique_consecutive(x, return_inverse=True, return_counts=True)
        assert t.equal(gv, wv) and t.equal(gi, wi) and t.equal(gc, wc) and gi.shape == x.shape
        assert t.equal(rsx.unique_consecutive(x), wv)
    # non-contiguous and misaligned views
    base = t.randint(0, 9, (300, 64), generator=g).to(dt).cuda()
    for view in (base.t(), base[:, 1::3], base.reshape(-1)[1:]):
        wv, wi, wc = t.unique(view, return_inverse=True, return_counts=True)
        gv, gi, gc = rsx.unique(view, return_inverse=True, return_counts=True)
        assert t.equal(gv, wv) and t.equal(gi, wi) and t.equal(gc, wc)
        wv, wi, wc = t.unique_consecutive(view, return_inverse=True, return_counts=True)
        gv, gi, gc = rsx.unique_consecutive(view, return_inverse=True, return_counts=True)
        assert t.equal(gv, wv) and t.equal(gi, wi) and t.equal(gc, wc)


def test_helper_float_semantics_and_segments(rsx):
    t = _torch()
    x = t.tensor([0.0, -0.0, float("nan"), 1.0, float("nan"), -0.0], device="cuda")
    v, inv, cnt = rsx.unique(x, return_inverse=True, return_counts=True)
    assert v.view(t.int32).tolist() == [-0x80000000, 0, 0x3F800000, 0x7FC00000]      # -0.0 and +0.0 apart, the two equal-bit NaNs one value
    assert cnt.tolist() == [2, 1, 1, 2] and inv.tolist() == [1, 0, 3, 2, 3, 0]
    keys = t.tensor([9, 5, 3, 5, 3, 3, 7, 7, 7, 2, 2, 8, 1, 9], dtype=t.int32, device="cuda")
    off = t.tensor([1, 6, 6, 9, 9, 13, 13], dtype=t.int64, device="cuda")
    v, ro, inv, cnt, fst = rsx.segmented_unique(keys, off, return_inverse=True, return_counts=True, return_first=True)
    assert v.tolist() == [3, 5, 7, 1, 2, 8] and ro.tolist() == [0, 2, 2, 3, 3, 6, 6] and cnt.tolist() == [3, 2, 3, 1, 2, 1]
    assert fst.tolist() == [1, 0, 0, 3, 0, 2] and inv.tolist() == [0, 1, 0, 1, 0, 0, 0, 0, 0, 1, 1, 2, 0, 0]
    assert inv.dtype == cnt.dtype == fst.dtype == ro.dtype == t.int64
    v, ro, cnt = rsx.segmented_unique(keys, off, return_counts=True, descending=True)
    assert v.tolist() == [5, 3, 7, 8, 2, 1] and cnt.tolist() == [2, 3, 3, 1, 2, 1]
    v, ro = rsx.segmented_unique(keys, off, consecutive=True)
    assert v.tolist() == [5, 3, 5, 3, 7, 2, 8, 1] and ro.tolist() == [0, 4, 4, 5, 5, 8, 8]
    with pytest.raises(rsx.RadixSortError):                                      # bad offsets raise
        rsx.segmented_unique(keys, t.tensor([0, 9, 4], dtype=t.int64, device="cuda"))
    assert rsx.segmented_unique(keys, off[:2])[0].tolist() == [3, 5]             # the engine stays usable


def test_helper_errors_and_side_stream(rsx):
    t = _torch()
    x = t.randint(0, 1000, (1 << 18,), device="cuda", dtype=t.int32)
    for dt in (t.bfloat16, t.float16, t.bool):
        with pytest.raises(TypeError):
            rsx.unique(x.to(dt))
        with pytest.raises(TypeError):
            rsx.unique_consecutive(x.to(dt))
    with pytest.raises(ValueError):
        rsx.unique(x.cpu())
    with pytest.raises(ValueError):
        rsx.segmented_unique(x, t.tensor([0, 5], device="cuda", dtype=t.int32))
    with pytest.raises(NotImplementedError):
        rsx.unique(x.reshape(512, 512), dim=0)
    with pytest.raises(NotImplementedError):
        rsx.unique_consecutive(x.reshape(512, 512), dim=-1)
    want = t.unique(x, return_inverse=True, return_counts=True)
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        got = rsx.unique(x, return_inverse=True, return_counts=True)
    side.synchronize()
    for a, b in zip(got, want):
        assert t.equal(a, b)
    streams = {key[1] for key in rsx._SEG_ENGINES}
    assert side.cuda_stream in streams
