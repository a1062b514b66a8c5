"""The histogram (rsx_segmented_histogram, radix_sort_amd.segmented_histogram / bincount / histc / histogram / bincount_rows /
histogram_rows) on the GPU.

The referee is tests/_histogram_ref.py; every comparison is exact equality with histogram_oracle: the call counts, there is no tolerance
anywhere.  The counters start out holding the family's sentinel — the call must overwrite every one of them, zeros included — and end in
a guard band; the bytes before them must survive.  Keys outside [off[0], off[S]) are random, so that reading one changes a count.  Every
engine here has capacity 4096: the call is not bound by it.  The layouts come from _histogram_ref, where tests/test_histogram.py checks
from the layout alone that each reaches the path it is named after.
"""
import numpy as np
import pytest

import _histogram_ref as H
from _histogram_ref import NO_BIN, bins_of, histogram_oracle
from _search_ref import UINT
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, GUARD

pytestmark = pytest.mark.gpu

CAP = 4096
GUARD_BYTE = 0xA5
FRONT = 12                                          # bytes before the counters: they then start 4-byte aligned only


def run(rsx, keys, off, bins, lo=0, hi=0, shift=0, descending=False, eng=None, payload=False):
    """One rsx_segmented_histogram through the Engine API.  Returns (counts [S, B] int64, engine)."""
    t = _torch()
    n = keys.size
    nseg = 1 if off is None else len(off) - 1
    even = np.isscalar(bins)
    B = int(bins) if even else len(bins) - 1
    k = dev(t, keys) if n else None
    o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
    e = None if even else dev(t, np.ascontiguousarray(bins, dtype=keys.dtype))
    out = dev(t, np.concatenate([np.full(FRONT + nseg * B * 4, FILL, dtype=np.uint8), np.full(GUARD, GUARD_BYTE, dtype=np.uint8)]))
    if eng is None:
        eng = rsx.Engine(keys.dtype, CAP, payload=payload, descending=descending)
    eng.segmented_histogram(k.data_ptr() if n else None, n, None if o is None else o.data_ptr(), nseg, B, out.data_ptr() + FRONT,
                            d_edges=None if even else e.data_ptr(), lo=lo, hi=hi, width_shift=shift)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    raw = out.cpu().numpy().view(np.uint8)
    assert np.all(raw[-GUARD:] == GUARD_BYTE), "guard band written"
    assert np.all(raw[:FRONT] == FILL), "bytes before the counters written"
    return raw[FRONT:-GUARD].copy().view(np.uint32).astype(np.int64).reshape(nseg, B), eng


def check(got, want, what=""):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: counts differ at (segment, bin) {bad[:6].tolist()} (of {len(bad)}): {got[tuple(bad[:6].T)].tolist()} != {want[tuple(bad[:6].T)].tolist()}"


def run_check(rsx, keys, off, what="", **kw):
    got, eng = run(rsx, keys, off, **kw)
    ref_kw = {k: v for k, v in kw.items() if k in ("bins", "lo", "hi", "shift", "descending")}
    check(got, histogram_oracle(keys, off, **ref_kw), what)
    return got, eng


# -- 1. the ragged layout: six dtypes x {even, edges} x {ascending, descending} x B ----------------------------------------------------------

@pytest.mark.parametrize("form", ["even", "edges"])
@pytest.mark.parametrize("dt", H.DTYPES)
def test_ragged_matrix(rsx, dt, form):
    n, off = H.ragged_layout()
    o = off.astype(np.int64)
    u = UINT[np.dtype(dt).itemsize]
    for descending in (False, True):
        eng = rsx.Engine(dt, CAP, descending=descending)
        for B in H.MATRIX_BINS:
            rng = np.random.default_rng(1000 + H.DTYPES.index(dt) * 100 + B)          # (tests/test_histogram.py draws the same cases)
            args = H.form_args(dt, form, descending, B, rng)
            keys = H.case_keys(rng, dt, n, off, args)
            live = keys[o[0]:o[-1]]
            b = bins_of(live, descending=descending, **args)
            assert np.any(b == NO_BIN) and np.any(b != NO_BIN)                         # out-of-range keys occur
            if form == "edges":
                assert np.all(np.isin(args["bins"].view(u), live.view(u)))             # ties with every edge
            else:
                assert np.any(live == np.dtype(dt).type(args["lo"]))
                assert np.dtype(dt).kind != "f" or np.any(live == np.dtype(dt).type(args["hi"]))
            run_check(rsx, keys, off, f"{form} B={B} descending={descending}", eng=eng, descending=descending, **args)
        eng.sync()


# -- 2. the direct path by bin count ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [4097, 50257])
def test_direct_path_by_bin_count(rsx, B):
    rng = np.random.default_rng(B)
    for dt in (np.int32, np.uint64):
        eng = rsx.Engine(dt, CAP)
        for n, off in ((H.SKEW_N, None), H.ragged_layout()):
            keys = rng.integers(-50 if np.dtype(dt).kind == "i" else 0, B + 50, n).astype(dt)
            got, _ = run_check(rsx, keys, off, f"B={B} {np.dtype(dt).name}", eng=eng, bins=B)
            assert 0 < got.sum() < n
        eng.sync()
    x = (rng.random(H.SKEW_N) * 3.0 - 0.5).astype(np.float32)                        # the float form too
    run_check(rsx, x, None, f"B={B} float32", bins=B, lo=0.0, hi=2.0)[1].sync()


# -- 3. skew, for the wave-private and the shared LDS layout -----------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [256, 4096], ids=["wave_private", "shared"])
def test_skew(rsx, B):
    assert H.lds_layout(B) == ("wave_private" if B == 256 else "shared")
    n = H.SKEW_N
    eng = rsx.Engine(np.uint32, CAP)
    for what, keys in (("one bin", np.full(n, B - 3, dtype=np.uint32)), ("one key a bin", (np.arange(n) % B).astype(np.uint32)),
                       ("an alternating pair", np.where(np.arange(n) % 2 == 0, 1, B - 1).astype(np.uint32))):
        got, _ = run_check(rsx, keys, None, what, eng=eng, bins=B)
        assert got.sum() == n
    eng.sync()


# -- 4. floats ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float32", "float64"])
def test_float_specials(rsx, dt):
    rng = np.random.default_rng(40)
    dt = np.dtype(dt)
    n = 9000
    off = np.array([5, 300, 300, 8990], dtype=np.uint64)
    keys = rng.integers(-6, 7, n).astype(dt) / dt.type(2)
    keys[rng.permutation(n)[:600]] = np.tile(H.special_floats(dt), 100)
    assert np.any(np.isnan(keys) & np.signbit(keys)) and np.any(np.isnan(keys) & ~np.signbit(keys))
    for descending in (False, True):
        eng = rsx.Engine(dt, CAP, descending=descending)
        # even form: -0.0 counts as 0.0; NaN and the infinities are dropped
        got, _ = run_check(rsx, keys, off, "even", eng=eng, descending=descending, bins=8, lo=-2.0, hi=2.0)
        assert got.sum() < int(off[-1] - off[0])
        # edges form: -0.0 and +0.0 are two edges, the NaNs and the infinities ordinary keys
        inf = dt.type(np.inf)
        for edges in (np.array([-inf, -1.0, -0.0, 0.0, 1.0, inf], dtype=dt), np.array([-np.nan, -inf, -0.0, 0.0, inf, np.nan], dtype=dt)):
            e = edges[::-1].copy() if descending else edges
            got, _ = run_check(rsx, keys, off, "edges", eng=eng, descending=descending, bins=e)
            zero_bins = bins_of(np.array([-0.0, 0.0], dtype=dt), e, descending=descending)
            assert zero_bins[0] != zero_bins[1] and got[[0, 2]][:, zero_bins].min() > 0
        eng.sync()


# -- 5. two-tile workgroups ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_keys():
    return np.random.default_rng(50).integers(0, 300, H.BIG_N).astype(np.uint32)        # (bins 256 .. 299 do not exist: dropped)


@pytest.mark.parametrize("layout", ["big_one_segment", "big_boundaries"])
def test_two_tile_workgroups(rsx, big_keys, layout):
    """2^24 + 4096 + 5 keys: a workgroup walks two tiles on 256 CUs and keeps its counters between them"""
    n, off = H.LAYOUTS[layout][0]()
    B = H.LAYOUTS[layout][1]
    run_check(rsx, big_keys, off, layout, bins=B)[1].sync()


# -- 6. many short segments -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["pairs", "empties", "fifties"])
def test_many_short_segments(rsx, layout):
    rng = np.random.default_rng(60)
    n, off = H.LAYOUTS[layout][0]()
    B = H.LAYOUTS[layout][1]
    keys = rng.integers(0, B + 3, n).astype(np.uint32)
    eng = rsx.Engine(np.uint32, CAP)
    run_check(rsx, keys, off, layout, eng=eng, bins=B)
    edges = np.arange(0, B + 1, dtype=np.uint32)
    run_check(rsx, keys, off, layout + " edges", eng=eng, bins=edges)
    eng.sync()


# -- 7. bad offsets ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_reported_once(rsx, bad):
    rng = np.random.default_rng(23)
    n = 40000
    x = rng.integers(0, 99, n).astype(np.uint32)
    off = np.array([0, 100, 5000, 4000 if bad == "decreasing" else n + 1, n], dtype=np.uint64)       # segment 2 is the first bad one
    eng = rsx.Engine(np.uint32, CAP)
    for args in (dict(bins=64), dict(bins=np.arange(0, 101, 10, dtype=np.uint32)), dict(bins=5000)):
        got, _ = run(rsx, x, off, eng=eng, **args)                                # guard bands checked inside
        with pytest.raises(rsx.RadixSortError) as ei:
            eng.sync()
        assert ei.value.status == 4 and "rsx_segmented_histogram" in str(ei.value) and "segment 2 " in str(ei.value)
        eng.sync()                                                               # reported once
        assert np.all(got == 0)
        good = np.array([0, 3, 5000, 5001, n], dtype=np.uint64)                    # the engine stays usable: the next call is right
        run_check(rsx, x, good, "after bad offsets", eng=eng, **args)
        eng.sync()


# -- 8. engine state --------------------------------------------------------------------------------------------------------------------------------------

def test_sort_state_is_untouched_and_n_exceeds_capacity(rsx):
    t = _torch()
    rng = np.random.default_rng(61)
    x = rng.integers(0, 1 << 32, CAP, dtype=np.uint32)
    xd = dev(t, x)
    n = 3 * CAP
    keys = rng.integers(0, 80, n).astype(np.uint32)
    off = np.array([7, 5000, 5000, n - 10], dtype=np.uint64)
    res = []
    for payload in (False, True):
        eng = rsx.Engine(np.uint32, CAP, payload=payload)
        pd = dev(t, np.arange(CAP, dtype=np.uint32)) if payload else None
        eng.sort_from(xd.data_ptr(), CAP, pd.data_ptr() if payload else None)
        got, _ = run_check(rsx, keys, off, f"payload={payload}", eng=eng, bins=64)
        res.append(got)
        assert eng.geometry().num_keys == CAP
        out = t.zeros(CAP, dtype=t.int32, device="cuda")
        t.cuda.synchronize()                                                     # (the engine copies on its own stream)
        eng.copy_result(out.data_ptr())
        eng.sync()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), np.sort(x))
    assert np.array_equal(res[0], res[1])


# -- 9. capture ----------------------------------------------------------------------------------------------------------------------------------------------

def test_capture_and_replay(rsx):
    """one captured call replayed twice with the keys rewritten in between: the zero-fill is inside the graph"""
    t = _torch()
    rng = np.random.default_rng(70)
    n, off = H.ragged_layout()
    nseg, B = len(off) - 1, 64
    side = t.cuda.Stream()
    eng = rsx.Engine(np.int32, CAP)
    eng.set_stream(side.cuda_stream)
    keys = rng.integers(-20, 90, n).astype(np.int32)
    kd, od = dev(t, keys), dev(t, off)
    out = dev(t, np.full(4 * nseg * B, FILL, dtype=np.uint8))
    call = lambda: eng.segmented_histogram(kd.data_ptr(), n, od.data_ptr(), nseg, B, out.data_ptr(), lo=-4)
    result = lambda: out.cpu().numpy().view(np.uint32).astype(np.int64).reshape(nseg, B)
    call()                                                                       # eager: the first call of an engine allocates its status words
    eng.sync()
    check(result(), histogram_oracle(keys, off, B, lo=-4), "eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for rep in range(2):
        keys = rng.integers(-20, 90, n).astype(np.int32)
        kd.copy_(t.from_numpy(keys))
        graph.replay()                                                           # (on top of the last replay's counts)
        t.cuda.synchronize()
        check(result(), histogram_oracle(keys, off, B, lo=-4), f"replay {rep}")
    del graph
    eng.sync()


# -- 10. refusals ---------------------------------------------------------------------------------------------------------------------------------------------

OK, BUFFERS, CALC = 0, 1, 4
ORDER = "d_keys n d_offsets num_segments d_edges lo_bits hi_bits width_shift num_bins flags d_counts_out".split()


def f32(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


@pytest.mark.parametrize("kind", ["uint32", "int64", "float32"])
def test_refusals(rsx, kind):
    """every rule of the call as a table: (status, changed arguments[, a word of the message]); a refused call launches nothing"""
    t = _torch()
    N, S, B = 1000, 2, 8
    dt = np.dtype(kind)
    kb = dt.itemsize
    slot = 64 << 10
    arena = t.zeros(5 * slot, dtype=t.uint8, device="cuda")
    keys, off, edges, counts, spare = (arena.data_ptr() + i * slot for i in range(5))
    arena[slot:slot + 24] = t.tensor([0, N // 2, N], dtype=t.int64, device="cuda").view(t.uint8)
    e_host = np.arange(B + 1).astype(dt)
    arena[2 * slot:2 * slot + e_host.nbytes] = t.from_numpy(e_host.view(np.uint8)).cuda()
    eng = rsx.Engine(dt, CAP)
    eng.sort_from(keys, N)
    eng.sync()
    own = eng.result_device()[0] + 64
    is_float = dt.kind == "f"
    even = dict(d_keys=keys, n=N, d_offsets=off, num_segments=S, d_edges=None, lo_bits=f32(0.0) if is_float else 0, hi_bits=f32(8.0) if is_float else 0,
                width_shift=0, num_bins=B, flags=0, d_counts_out=counts)
    with_edges = dict(even, d_edges=edges, lo_bits=0, hi_bits=0)
    rows = [
        (CALC, dict(flags=1)), (CALC, dict(flags=4)), (CALC, dict(flags=1 << 31)),
        (CALC, dict(num_bins=0)), (CALC, dict(num_bins=(1 << 31) + 1)),
        (CALC, dict(num_bins=(1 << 30) + 1), "2^31"),                                # S x B > 2^31
        (OK, dict(num_segments=0)),
        (CALC, dict(num_segments=(1 << 32) - 1), "segments"), (CALC, dict(n=(1 << 31) + 1), "elements"),
        (BUFFERS, dict(d_keys=None)), (BUFFERS, dict(d_keys=keys + 4)), (BUFFERS, dict(d_counts_out=None)), (BUFFERS, dict(d_counts_out=counts + 2)),
        (BUFFERS, dict(d_offsets=off + 4)),
        (BUFFERS, dict(d_counts_out=keys), "overlap"), (BUFFERS, dict(d_counts_out=off), "overlap"), (BUFFERS, dict(d_counts_out=own), "engine"),
        (BUFFERS, dict(d_keys=own), "engine"), (BUFFERS, dict(d_counts_out=keys + N * kb - 4), "overlap"),
        (OK, dict(d_counts_out=keys + N * kb)),                                      # adjacent is no overlap
        (OK, dict(d_offsets=None)), (OK, dict(n=0, d_offsets=None)), (OK, dict(n=0, d_keys=None, d_offsets=None)), (OK, dict(d_counts_out=counts + 4)),
        # two faults: a limit before a pointer, a misaligned pointer before an overlap
        (CALC, dict(flags=1, d_keys=None)), (CALC, dict(n=(1 << 31) + 1, d_keys=keys + 4)), (BUFFERS, dict(d_keys=keys + 4, d_counts_out=off), "aligned"),
    ]
    if is_float:
        rows += [(CALC, dict(width_shift=1), "width_shift"), (CALC, dict(lo_bits=f32(8.0)), "lo < hi"), (CALC, dict(lo_bits=f32(9.0)), "lo < hi"),
                 (CALC, dict(hi_bits=f32(np.inf)), "finite"), (CALC, dict(lo_bits=f32(np.nan)), "finite"), (CALC, dict(lo_bits=f32(-np.inf)), "finite"),
                 (CALC, dict(lo_bits=f32(-3e38), hi_bits=f32(3e38)), "finite positive")]
    else:
        rows += [(CALC, dict(hi_bits=1), "hi_bits"), (CALC, dict(width_shift=8 * kb), "width_shift"), (OK, dict(width_shift=8 * kb - 1)),
                 (OK, dict(lo_bits=(1 << 64) - 1))]                                  # (the low key_bytes count)
    edge_rows = [
        (OK, dict()), (OK, dict(num_bins=1)),
        (CALC, dict(num_bins=4097), "4096"), (CALC, dict(lo_bits=1), "edges form"), (CALC, dict(hi_bits=1), "edges form"),
        (CALC, dict(width_shift=1), "edges form"), (CALC, dict(flags=2)),
        (BUFFERS, dict(d_edges=edges + kb // 2), "edges"), (BUFFERS, dict(d_edges=own), "engine"),
        (BUFFERS, dict(d_counts_out=edges), "overlap"), (BUFFERS, dict(d_counts_out=edges + B * kb), "overlap"),
        (OK, dict(d_counts_out=edges + (B + 1) * kb + (4 if kb == 8 else 0))),
    ]
    lib = rsx.load_library()

    def call(args):
        vals = [args[k] for k in ORDER]
        rc = lib.rsx_segmented_histogram(eng._h, *vals)
        return rc, lib.rsx_last_error().decode()

    null_rc = lib.rsx_segmented_histogram(None, *[even[k] for k in ORDER])
    assert null_rc == CALC and "rsx_segmented_histogram: null engine" in lib.rsx_last_error().decode()
    for base, table in ((even, rows), (with_edges, edge_rows)):
        for row in table:
            status, change = row[0], row[1]
            arena[3 * slot:3 * slot + 4 * S * B] = 0xC3
            rc, msg = call(dict(base, **change))
            t.cuda.synchronize()                                                 # (an accepted row runs on the engine's stream: before the next fill)
            assert rc == status, (row, msg)
            if status != OK:
                assert "rsx_segmented_histogram" in msg and (len(row) < 3 or row[2] in msg), (row, msg)
                assert bool((arena[3 * slot:3 * slot + 4 * S * B] == 0xC3).all()), ("a refused call wrote something", row)
    eng.sync()
    # n == 0 with a valid shape still zeroes the counters; no segments: nothing is written
    arena[3 * slot:3 * slot + 4 * S * B] = 0xC3
    assert call(dict(even, n=0, d_offsets=None))[0] == OK                          # (one segment: B counters)
    eng.sync()
    assert bool((arena[3 * slot:3 * slot + 4 * B] == 0).all()) and bool((arena[3 * slot + 4 * B:3 * slot + 4 * S * B] == 0xC3).all())
    arena[3 * slot:3 * slot + 4 * S * B] = 0xC3
    assert call(dict(even, num_segments=0))[0] == OK
    eng.sync()
    assert bool((arena[3 * slot:3 * slot + 4 * S * B] == 0xC3).all())
    assert call(even)[0] == OK                                                     # and the call these were variations of works: all keys are zero
    eng.sync()
    got = arena[3 * slot:3 * slot + 4 * S * B].cpu().numpy().view(np.uint32).reshape(S, B)
    assert got[:, 0].tolist() == [N // 2, N - N // 2] and got[:, 1:].sum() == 0


# -- 11. the helpers against torch ------------------------------------------------------------------------------------------------------------------------

def test_helpers_against_torch(rsx):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(5)
    x = t.randint(0, 1000, (50000,), device="cuda", generator=g)
    assert t.equal(rsx.bincount(x), t.bincount(x))
    assert t.equal(rsx.bincount(x, minlength=2000), t.bincount(x, minlength=2000))
    assert t.equal(rsx.bincount(x, num_bins=1000), t.bincount(x, minlength=1000))
    assert t.equal(rsx.bincount(x, num_bins=300), t.bincount(x)[:300])               # values from num_bins on are dropped
    assert t.equal(rsx.bincount(x.to(t.int32)), t.bincount(x))
    assert rsx.bincount(x[:0]).numel() == 0 and t.equal(rsx.bincount(x[:0], minlength=5), t.zeros(5, dtype=t.int64, device="cuda"))
    with pytest.raises(ValueError, match="negative"):
        rsx.bincount(x - 1)
    assert int(rsx.bincount(x - 1, num_bins=10).sum()) == int(((x >= 1) & (x <= 10)).sum())          # no read-back: negatives are dropped
    # non-contiguous and misaligned inputs are copied
    assert t.equal(rsx.bincount(x[::3]), t.bincount(x[::3])) and t.equal(rsx.bincount(x[1:]), t.bincount(x[1:]))
    # rows
    ids = t.randint(0, 64, (7, 33, 129), device="cuda", generator=g)
    rows = rsx.bincount_rows(ids, 64)
    assert rows.shape == (7, 33, 64) and rows.dtype == t.int64
    want = t.stack([t.bincount(r, minlength=64) for r in ids.reshape(-1, 129)]).reshape(7, 33, 64)
    assert t.equal(rows, want)
    assert t.equal(rsx.bincount_rows(ids.transpose(0, 1), 64), want.transpose(0, 1))
    # histc / histogram on exact inputs: integer-valued floats on a power-of-two range
    for dt in (t.float32, t.float64):
        f = t.randint(-40, 100, (30000,), device="cuda", generator=g).to(dt)
        for bins, lo, hi in ((64, 0.0, 64.0), (16, -32.0, 32.0), (128, 0.0, 64.0)):
            assert t.equal(rsx.histc(f, bins=bins, min=lo, max=hi), t.histc(f, bins=bins, min=lo, max=hi)), (dt, bins)
            counts, edges = rsx.histogram(f, bins, range=(lo, hi))
            wc, _ = t.histogram(f.cpu(), bins, range=(lo, hi))
            assert t.equal(counts.cpu(), wc.to(t.int64)) and t.equal(edges, t.linspace(lo, hi, bins + 1, dtype=dt, device="cuda"))
        f2 = t.cat([f.clamp(-40.0, 88.0), t.tensor([-40.0, 88.0], dtype=dt, device="cuda")])        # min == max: the data's range, [-40, 88], 128 wide
        assert t.equal(rsx.histc(f2, bins=128), t.histc(f2, bins=128))
        e = t.tensor([-50.0, -40.0, -3.5, 0.0, 0.5, 64.0, 99.0], dtype=dt, device="cuda")
        counts, edges = rsx.histogram(f, e)
        assert t.equal(counts.cpu(), t.histogram(f.cpu(), e.cpu())[0].to(t.int64)) and edges is e
        fr = f[:29952].reshape(3, 4, 2496)
        counts, edges = rsx.histogram_rows(fr, e)
        want = t.stack([t.histogram(r, e.cpu())[0] for r in fr.cpu().reshape(-1, 2496)]).reshape(3, 4, 6).to(t.int64)
        assert t.equal(counts.cpu(), want)
        counts, edges = rsx.histogram_rows(fr, 16, range=(-32.0, 32.0))
        want = t.stack([t.histc(r, bins=16, min=-32.0, max=32.0) for r in fr.reshape(-1, 2496)]).reshape(3, 4, 16).to(t.int64)
        assert t.equal(counts, want) and edges.numel() == 17
    with pytest.raises(TypeError):
        rsx.histogram(f, e.to(t.float32))                                            # the edges have another dtype
    # integer keys with edges: numpy.histogram
    xi = t.randint(-500, 500, (20000,), device="cuda", generator=g)
    ei = t.tensor([-400, -1, 0, 1, 250, 499], device="cuda")
    counts, _ = rsx.histogram(xi, ei)
    assert np.array_equal(counts.cpu().numpy(), np.histogram(xi.cpu().numpy(), bins=ei.cpu().numpy())[0])
    # a non-default current stream
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        got = rsx.bincount(x, num_bins=1000)
        got_rows = rsx.bincount_rows(ids, 64)
    side.synchronize()
    assert t.equal(got, t.bincount(x, minlength=1000)) and t.equal(got_rows, rows)
    seg = rsx.segmented_histogram(x, t.tensor([5, 100, 100, 40000], device="cuda"), 16, lo=8, width_shift=6)
    xh = x.cpu().numpy()
    assert np.array_equal(seg.cpu().numpy(), histogram_oracle(xh, np.array([5, 100, 100, 40000]), 16, lo=8, shift=6))


# -- 12. unsorted edges -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [np.uint32, np.float64], ids=["uint32", "float64"])
def test_unsorted_edges_stay_inside(rsx, dt):
    """counts are unspecified, but every key is counted at most once and nothing outside the counters is written (run checks the bands)"""
    rng = np.random.default_rng(120)
    n, off = H.ragged_layout()
    keys = H.random_keys(rng, dt, n, H.SPAN)
    for B in (1, 13, 4096):
        edges = rng.permutation(H.sorted_edges(rng, dt, B, H.SPAN))
        got, eng = run(rsx, keys, off, edges)
        eng.sync()
        assert np.all(got >= 0) and np.all(got.sum(axis=1) <= np.diff(off.astype(np.int64)))
