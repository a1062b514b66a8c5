"""The weighted histogram (rsx_segmented_weighted_histogram, radix_sort_amd.segmented_weighted_histogram and the weights= / weight= keywords of
bincount, bincount_rows, histogram, histogram_rows) on the GPU.

The referee is tests/_whistogram_ref.py; every comparison of masses is exact int64 equality with whistogram_oracle: the sums are integers,
there is no tolerance anywhere.  The harness is tests/test_gpu_histogram.py's: engines of capacity 4096 (the call is not bound by it), the
sums pre-filled with the family's sentinel — the call must overwrite every one of them, zeros included — and followed by a guard band, 8
bytes in front of them so that they start 8-byte aligned only, and random keys and weights outside [off[0], off[S]), so that reading one
changes a sum.  The layouts come from _histogram_ref and _whistogram_ref, where tests/test_whistogram.py checks from the layout alone that
each reaches the path it is named after with this kernel's constants (2048 bins in LDS, wave-private up to 512, direct below 256 keys).
"""
import numpy as np
import pytest

import _histogram_ref as H
import _whistogram_ref as W
from _histogram_ref import NO_BIN, bins_of
from _search_ref import UINT
from _whistogram_ref import signed_mass_np, whistogram_oracle
from _wselect_ref import kind_of
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, GUARD

pytestmark = pytest.mark.gpu

CAP = 4096
GUARD_BYTE = 0xA5
FRONT = 8                                           # bytes before the sums: they then start 8-byte aligned only


def run(rsx, keys, weights, off, bins, lo=0, hi=0, shift=0, descending=False, weight_exp=0, signed=False, eng=None, payload=False, skew=0):
    """One rsx_segmented_weighted_histogram through the Engine API.  skew: the weights start that many elements past a 16-byte boundary.
    Returns (sums [S, B] int64, engine)."""
    t = _torch()
    n = keys.size
    nseg = 1 if off is None else len(off) - 1
    even = np.isscalar(bins)
    B = int(bins) if even else len(bins) - 1
    k = dev(t, keys) if n else None
    w = dev(t, np.concatenate([np.zeros(skew, dtype=weights.dtype), weights, np.zeros(1, dtype=weights.dtype)]))       # (never empty: the call wants a pointer)
    wptr = w.data_ptr() + skew * weights.dtype.itemsize
    assert w.data_ptr() % 16 == 0
    o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
    e = None if even else dev(t, np.ascontiguousarray(bins, dtype=keys.dtype))
    out = dev(t, np.concatenate([np.full(FRONT + nseg * B * 8, FILL, dtype=np.uint8), np.full(GUARD, GUARD_BYTE, dtype=np.uint8)]))
    assert (out.data_ptr() + FRONT) % 16 == 8
    if eng is None:
        eng = rsx.Engine(keys.dtype, CAP, payload=payload, descending=descending)
    eng.segmented_weighted_histogram(k.data_ptr() if n else None, wptr, n, None if o is None else o.data_ptr(), nseg, B, out.data_ptr() + FRONT,
                                     kind_of(weights), weight_exp, rsx.WHIST_SIGNED if signed else 0, d_edges=None if even else e.data_ptr(), lo=lo, hi=hi,
                                     width_shift=shift)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    raw = out.cpu().numpy().view(np.uint8)
    assert np.all(raw[-GUARD:] == GUARD_BYTE), "guard band written"
    assert np.all(raw[:FRONT] == FILL), "bytes before the sums written"
    return raw[FRONT:-GUARD].copy().view(np.int64).reshape(nseg, B), eng


def check(got, want, what=""):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: sums differ at (segment, bin) {bad[:6].tolist()} (of {len(bad)}): {got[tuple(bad[:6].T)].tolist()} != {want[tuple(bad[:6].T)].tolist()}"


REF_KEYS = ("bins", "lo", "hi", "shift", "descending", "weight_exp", "signed")


def run_check(rsx, keys, weights, off, what="", **kw):
    got, eng = run(rsx, keys, weights, off, **kw)
    check(got, whistogram_oracle(keys, weights, off, **{k: v for k, v in kw.items() if k in REF_KEYS}), what)
    return got, eng


def weight_cases(rng, n, off):
    """(name, weights, weight_exp, signed) of the three kinds, the float kinds unsigned and signed, at exponents of their own"""
    for wdt, wexp in ((np.uint32, 0), (np.float32, -3), (np.float64, 5)):
        w = W.case_weights(rng, wdt, n, off, wexp)
        for signed in ((False,) if wdt == np.uint32 else (False, True)):
            yield f"{np.dtype(wdt).name} signed={signed}", w, wexp, signed


# -- 1. the ragged layout: six key dtypes x {even, edges} x {ascending, descending} x B x the weight kinds ---------------------------------------------

@pytest.mark.parametrize("form", ["even", "edges"])
@pytest.mark.parametrize("dt", H.DTYPES)
def test_ragged_matrix(rsx, dt, form):
    n, off = H.ragged_layout()
    o = off.astype(np.int64)
    u = UINT[np.dtype(dt).itemsize]
    for descending in (False, True):
        eng = rsx.Engine(dt, CAP, descending=descending)
        for B in W.MATRIX_BINS:
            rng = np.random.default_rng(3000 + H.DTYPES.index(dt) * 100 + B)
            args = W.form_args(dt, form, descending, B, rng)
            keys = H.case_keys(rng, dt, n, off, args)
            live = keys[o[0]:o[-1]]
            b = bins_of(live, descending=descending, **args)
            assert np.any(b == NO_BIN) and np.any(b != NO_BIN)                         # out-of-range keys occur
            if form == "edges":
                assert np.all(np.isin(args["bins"].view(u), live.view(u)))             # ties with every edge
            for name, w, wexp, signed in weight_cases(rng, n, off):
                got, _ = run_check(rsx, keys, w, off, f"{form} B={B} descending={descending} {name}", eng=eng, descending=descending, weight_exp=wexp,
                                   signed=signed, **args)
                assert np.any(got != 0) and (not signed or np.any(got < 0))
        eng.sync()


# -- 2. the paths by bin count -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", W.PATH_BINS + [4096, 50257])
def test_paths_by_bin_count(rsx, B):
    """512 / 513: the last wave-private and the first shared size; 2048 / 2049: the last LDS and the first direct size; 4096: the edges
    form, direct with its edges staged in LDS; 50257: direct"""
    rng = np.random.default_rng(B)
    edges_form = B == 4096
    for dt in (np.int32, np.uint64):
        eng = rsx.Engine(dt, CAP)
        for n, off in ((H.SKEW_N, None), H.ragged_layout()):
            keys = rng.integers(-50 if np.dtype(dt).kind == "i" else 0, B + 50, n).astype(dt)
            bins = np.arange(0, B + 1).astype(dt) if edges_form else B
            for name, w, wexp, signed in weight_cases(rng, n, off):
                got, _ = run_check(rsx, keys, w, off, f"B={B} {np.dtype(dt).name} {name}", eng=eng, bins=bins, weight_exp=wexp, signed=signed)
                assert np.count_nonzero(got) > min(B, 300) // 2
        eng.sync()
    x = (rng.random(H.SKEW_N) * 3.0 - 0.5).astype(np.float32)                        # the float form too, one kernel per bin count
    if not edges_form:
        w = W.case_weights(rng, np.float32, H.SKEW_N, None, 0)
        run_check(rsx, x, w, None, f"B={B} float32 keys", bins=B, lo=0.0, hi=2.0, signed=True)[1].sync()


# -- 3. skew: the 64-bit fold of a run ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [256, 2048], ids=["wave_private", "shared"])
def test_skew(rsx, B):
    assert W.lds_layout(B) == ("wave_private" if B == 256 else "shared")
    n = H.SKEW_N
    rng = np.random.default_rng(B + 1)
    eng = rsx.Engine(np.uint32, CAP)
    heavy = np.full(n, 0xFFFFFFFF, dtype=np.uint32)                                  # a thread's 16 keys fold to 16 * (2^32 - 1): past 32 bits
    mixed = W.case_weights(rng, np.float32, n, None, 0)
    for what, keys in (("one bin", np.full(n, B - 3, dtype=np.uint32)), ("one key a bin", (np.arange(n) % B).astype(np.uint32)),
                       ("an alternating pair", np.where(np.arange(n) % 2 == 0, 1, B - 1).astype(np.uint32))):
        got, _ = run_check(rsx, keys, heavy, None, what + " heavy", eng=eng, bins=B)
        assert int(got.sum()) == n * 0xFFFFFFFF
        run_check(rsx, keys, mixed, None, what + " signed", eng=eng, bins=B, signed=True)
        run_check(rsx, keys, mixed, None, what + " unsigned", eng=eng, bins=B)
    eng.sync()


# -- 4. carry-over and flush on two-tile workgroups ---------------------------------------------------------------------------------------------------------------

def test_carry_over_and_flush(rsx):
    """2^24 + 4101 keys: a workgroup walks two tiles on 256 CUs, keeps its sums between them and flushes at a segment change"""
    n, off = H.big_boundaries_layout()
    B = 256
    assert {p[3] for p in W.piece_paths(n, off, B)} == {"lds_first", "lds_same", "lds_flush", "direct"}
    rng = np.random.default_rng(50)
    keys = rng.integers(0, 300, n).astype(np.uint32)                                 # (bins 256 .. 299 do not exist: dropped)
    w = ((rng.random(n) * 2.0 - 1.0)).astype(np.float32)
    run_check(rsx, keys, w, off, "big_boundaries", bins=B, signed=True)[1].sync()


# -- 5. piece slots and many short segments ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", sorted(H.SLOT_LAYOUTS) + ["pairs", "empties", "fifties"])
def test_piece_slots_and_short_segments(rsx, layout):
    rng = np.random.default_rng(60)
    n, off = (H.SLOT_LAYOUTS[layout] if layout in H.SLOT_LAYOUTS else H.LAYOUTS[layout][0])()
    B = 16
    keys = H.shifted_bins(rng, n, off, B).astype(np.uint32)                          # neighbours' histograms differ
    eng = rsx.Engine(np.uint32, CAP)
    for name, w, wexp, signed in weight_cases(rng, n, off):
        run_check(rsx, keys, w, off, f"{layout} {name}", eng=eng, bins=B, weight_exp=wexp, signed=signed)
    run_check(rsx, keys, W.case_weights(rng, np.float64, n, off, 0), off, layout + " edges", eng=eng, bins=np.arange(0, B + 1, dtype=np.uint32), signed=True)
    eng.sync()


# -- 6. weight alignment ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wdt", [np.float32, np.float64], ids=["float32", "float64"])
def test_weight_alignment(rsx, wdt):
    """weights that start one element past a 16-byte boundary take the element loads: the result of the aligned call on the same data"""
    rng = np.random.default_rng(77)
    eng = rsx.Engine(np.int32, CAP)
    for n, off in ((H.SKEW_N, None), H.ragged_layout()):
        keys = rng.integers(-5, 70, n).astype(np.int32)
        w = W.case_weights(rng, wdt, n, off, 2)
        aligned, _ = run_check(rsx, keys, w, off, "aligned", eng=eng, bins=64, weight_exp=2, signed=True)
        shifted, _ = run_check(rsx, keys, w, off, "one element past", eng=eng, bins=64, weight_exp=2, signed=True, skew=1)
        assert np.array_equal(aligned, shifted)
    eng.sync()


# -- 7. the magnitude of a sum --------------------------------------------------------------------------------------------------------------------------------------------

def test_sum_magnitude_and_cancellation(rsx):
    n = 1 << 16
    eng = rsx.Engine(np.uint32, CAP)
    keys = np.full(n, 5, dtype=np.uint32)
    got, _ = run_check(rsx, keys, np.full(n, 0xFFFFFFFF, dtype=np.uint32), None, "2^16 x (2^32 - 1)", eng=eng, bins=8)
    assert int(got[0, 5]) == n * 0xFFFFFFFF > 1 << 47 and np.count_nonzero(got) == 1
    # signed sums that cancel to exactly 0: every weight beside its negative, in LDS and on the direct path
    rng = np.random.default_rng(8)
    half = rng.random(n // 2).astype(np.float32) + np.float32(0.001)
    w = np.concatenate([half, -half])[rng.permutation(n)]
    for B in (8, 5000):
        got, _ = run_check(rsx, keys, w, None, f"cancel B={B}", eng=eng, bins=B, signed=True)
        assert np.all(got == 0)
        got, _ = run_check(rsx, keys, w, None, f"unsigned B={B}", eng=eng, bins=B)
        assert int(got[0, 5]) == int(signed_mass_np(half).sum()) > 0
    eng.sync()


# -- 8. the row sums are the weighted select's totals ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wdt", W.WEIGHT_DTYPES, ids=["uint32", "float32", "float64"])
def test_row_sums_equal_weighted_select_totals(rsx, wdt):
    from test_gpu_wselect import run as wselect_run
    rng = np.random.default_rng(90)
    n, off = H.ragged_layout()
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    wexp = 0 if wdt == np.uint32 else 4
    w = W.case_weights(rng, wdt, n, off, wexp)
    edges = np.array([0, 0xFFFFFFFF], dtype=np.uint32)                                # one bin, closed on both sides: every key
    got, eng = run_check(rsx, keys, w, off, "one bin", bins=edges, weight_exp=wexp)
    eng.sync()
    nseg = len(off) - 1
    total = wselect_run(rsx, keys, off, w, np.ones((nseg, 1), dtype=np.uint64), weight_exp=wexp)[4]
    assert got.shape == (nseg, 1) and np.array_equal(got[:, 0].view(np.uint64), total) and np.any(total > 0)


# -- 9. reproducibility ------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_reproducible_across_engines_streams_and_replays(rsx):
    t = _torch()
    rng = np.random.default_rng(70)
    n, off = H.ragged_layout()
    nseg, B = len(off) - 1, 64
    keys = rng.integers(-20, 90, n).astype(np.int32)
    w = W.case_weights(rng, np.float32, n, off, 1)
    want = whistogram_oracle(keys, w, off, B, lo=-4, weight_exp=1, signed=True)
    kd, wd, od = dev(t, keys), dev(t, w), dev(t, off)
    results = []
    graph = None
    for i in range(2):
        side = t.cuda.Stream()
        eng = rsx.Engine(np.int32, CAP)
        eng.set_stream(side.cuda_stream)
        out = dev(t, np.full(8 * nseg * B, FILL, dtype=np.uint8))
        call = lambda: eng.segmented_weighted_histogram(kd.data_ptr(), wd.data_ptr(), n, od.data_ptr(), nseg, B, out.data_ptr(), rsx.WEIGHT_FLOAT32, 1,
                                                        rsx.WHIST_SIGNED, lo=-4)
        result = lambda: out.cpu().numpy().view(np.int64).reshape(nseg, B).copy()
        call()                                                                       # eager: the first call of an engine allocates its status words
        eng.sync()
        results.append(result())
        if i == 1:                                                                   # a linear capture: the zero-fill, the offset check and the walk
            graph = t.cuda.CUDAGraph()
            with t.cuda.graph(graph, stream=side):
                call()
            for rep in range(2):
                out.fill_(FILL - 256)
                t.cuda.synchronize()
                graph.replay()
                t.cuda.synchronize()
                results.append(result())
            del graph
        eng.sync()
    for r in results:
        check(r, want, "reproducibility")
    assert all(r.tobytes() == results[0].tobytes() for r in results) and len(results) == 4


# -- 10. the contract's edges ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_empty_input_zeroes_and_no_segments_write_nothing(rsx):
    t = _torch()
    w = np.ones(4, dtype=np.float32)
    eng = rsx.Engine(np.uint32, CAP)
    got, _ = run(rsx, np.zeros(0, dtype=np.uint32), w[:0], None, 8, eng=eng)          # n == 0, one segment
    assert got.shape == (1, 8) and np.all(got == 0)
    got, _ = run(rsx, np.zeros(0, dtype=np.uint32), w[:0], np.array([0, 0, 0], dtype=np.uint64), 8, eng=eng, signed=True)
    assert got.shape == (2, 8) and np.all(got == 0)
    eng.sync()
    out = dev(t, np.full(64, FILL, dtype=np.uint8))
    kd, wd, od = dev(t, np.arange(4, dtype=np.uint32)), dev(t, w), dev(t, np.zeros(1, dtype=np.uint64))
    eng.segmented_weighted_histogram(kd.data_ptr(), wd.data_ptr(), 4, od.data_ptr(), 0, 8, out.data_ptr(), rsx.WEIGHT_FLOAT32)
    eng.sync()
    assert bool((out == FILL - 256).all())                                            # d_offsets with num_segments == 0: nothing is written


@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_reported_once(rsx, bad):
    rng = np.random.default_rng(23)
    n = 40000
    x = rng.integers(0, 99, n).astype(np.uint32)
    w = W.case_weights(rng, np.float32, n, None, 0)
    off = np.array([0, 100, 5000, 4000 if bad == "decreasing" else n + 1, n], dtype=np.uint64)       # segment 2 is the first bad one
    eng = rsx.Engine(np.uint32, CAP)
    for args in (dict(bins=64), dict(bins=np.arange(0, 101, 10, dtype=np.uint32)), dict(bins=5000)):
        got, _ = run(rsx, x, w, off, eng=eng, signed=True, **args)                 # guard bands checked inside
        with pytest.raises(rsx.RadixSortError) as ei:
            eng.sync()
        assert ei.value.status == 4 and "rsx_segmented_weighted_histogram" in str(ei.value) and "segment 2 " in str(ei.value)
        eng.sync()                                                               # reported once
        assert np.all(got == 0)
        good = np.array([0, 3, 5000, 5001, n], dtype=np.uint64)                    # the engine stays usable: the next call is right
        run_check(rsx, x, w, good, "after bad offsets", eng=eng, signed=True, **args)
        eng.sync()


def test_sort_state_is_untouched_and_n_exceeds_capacity(rsx):
    t = _torch()
    rng = np.random.default_rng(61)
    x = rng.integers(0, 1 << 32, CAP, dtype=np.uint32)
    xd = dev(t, x)
    n = 3 * CAP
    keys = rng.integers(0, 80, n).astype(np.uint32)
    w = W.case_weights(rng, np.float64, n, None, 0)
    off = np.array([7, 5000, 5000, n - 10], dtype=np.uint64)
    res = []
    for payload in (False, True):
        eng = rsx.Engine(np.uint32, CAP, payload=payload)
        pd = dev(t, np.arange(CAP, dtype=np.uint32)) if payload else None
        eng.sort_from(xd.data_ptr(), CAP, pd.data_ptr() if payload else None)
        got, _ = run_check(rsx, keys, w, off, f"payload={payload}", eng=eng, bins=64, signed=True)
        res.append(got)
        assert eng.geometry().num_keys == CAP
        out = t.zeros(CAP, dtype=t.int32, device="cuda")
        t.cuda.synchronize()                                                     # (the engine copies on its own stream)
        eng.copy_result(out.data_ptr())
        eng.sync()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), np.sort(x))
    assert np.array_equal(res[0], res[1])


# -- 11. refusals -----------------------------------------------------------------------------------------------------------------------------------------------------------------------

OK, BUFFERS, CALC = 0, 1, 4
ORDER = "d_keys d_weights n d_offsets num_segments d_edges lo_bits hi_bits width_shift num_bins flags weight_kind weight_exp d_sums_out".split()


def f32(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


@pytest.mark.parametrize("kind", ["uint32", "int64", "float32"])
def test_refusals(rsx, kind):
    """every rule of the call as a table: (status, changed arguments[, a word of the message]); a refused call launches nothing.  16 keys."""
    t = _torch()
    N, S, B = 16, 2, 8
    dt = np.dtype(kind)
    kb = dt.itemsize
    slot = 4 << 10
    arena = t.zeros(6 * slot, dtype=t.uint8, device="cuda")
    keys, off, edges, sums, weights, spare = (arena.data_ptr() + i * slot for i in range(6))
    arena[slot:slot + 24] = t.tensor([0, N // 2, N], dtype=t.int64, device="cuda").view(t.uint8)
    e_host = np.arange(B + 1).astype(dt)
    arena[2 * slot:2 * slot + e_host.nbytes] = t.from_numpy(e_host.view(np.uint8)).cuda()
    arena[4 * slot:4 * slot + 4 * N] = t.from_numpy(np.full(N, 0.5, dtype=np.float32).view(np.uint8)).cuda()
    eng = rsx.Engine(dt, CAP)
    eng.sort_from(keys, N)
    eng.sync()
    own = eng.result_device()[0] + 64
    is_float = dt.kind == "f"
    F32, F64, U32, SIGNED = rsx.WEIGHT_FLOAT32, rsx.WEIGHT_FLOAT64, rsx.WEIGHT_UINT32, rsx.WHIST_SIGNED
    even = dict(d_keys=keys, d_weights=weights, n=N, d_offsets=off, num_segments=S, d_edges=None, lo_bits=f32(0.0) if is_float else 0,
                hi_bits=f32(8.0) if is_float else 0, width_shift=0, num_bins=B, flags=0, weight_kind=F32, weight_exp=0, d_sums_out=sums)
    with_edges = dict(even, d_edges=edges, lo_bits=0, hi_bits=0)
    rows = [
        # what the unweighted call refuses
        (CALC, dict(flags=1)), (CALC, dict(flags=128)), (CALC, dict(flags=SIGNED | 512)), (CALC, dict(flags=1 << 31)), (OK, dict(flags=SIGNED)),
        (CALC, dict(num_bins=0)), (CALC, dict(num_bins=(1 << 30) + 1), "2^30"),
        (CALC, dict(num_bins=(1 << 29) + 1), "2^30"),                                # S x B > 2^30
        (OK, dict(num_segments=0)),
        (CALC, dict(num_segments=(1 << 32) - 1), "segments"), (CALC, dict(n=(1 << 31) + 1), "elements"),
        (BUFFERS, dict(d_keys=None)), (BUFFERS, dict(d_keys=keys + 4)), (BUFFERS, dict(d_sums_out=None)), (BUFFERS, dict(d_sums_out=sums + 4), "8-byte"),
        (BUFFERS, dict(d_offsets=off + 4)),
        (BUFFERS, dict(d_sums_out=keys), "overlap"), (BUFFERS, dict(d_sums_out=off), "overlap"), (BUFFERS, dict(d_sums_out=own), "engine"),
        (BUFFERS, dict(d_keys=own), "engine"), (BUFFERS, dict(d_sums_out=keys + N * kb - 8), "overlap"),
        (OK, dict(d_sums_out=keys + N * kb)),                                        # adjacent is no overlap
        (OK, dict(d_offsets=None)), (OK, dict(n=0, d_offsets=None)), (OK, dict(n=0, d_keys=None, d_offsets=None)), (OK, dict(d_sums_out=sums + 8)),
        # the weights
        (CALC, dict(weight_kind=3), "weight_kind"), (CALC, dict(weight_kind=U32, weight_exp=1), "weight_exp"), (CALC, dict(weight_exp=2049), "weight_exp"),
        (CALC, dict(weight_exp=-2049), "weight_exp"), (OK, dict(weight_exp=2048)), (OK, dict(weight_exp=-2048)), (OK, dict(weight_kind=U32)),
        (OK, dict(weight_kind=F64, n=N // 2, d_offsets=None)),
        (CALC, dict(weight_kind=U32, flags=SIGNED), "RSX_WHIST_SIGNED"), (OK, dict(weight_kind=F64, n=N // 2, d_offsets=None, flags=SIGNED)),
        (BUFFERS, dict(d_weights=None), "weights"), (BUFFERS, dict(d_weights=None, n=0, d_offsets=None), "weights"),
        (BUFFERS, dict(d_weights=weights + 2), "weights"), (BUFFERS, dict(d_weights=weights + 4, weight_kind=F64, n=N // 2, d_offsets=None), "weights"),
        (OK, dict(d_weights=weights + 4, n=N - 1, d_offsets=None)),                  # element-aligned weights are enough
        (BUFFERS, dict(d_sums_out=weights), "overlap"), (BUFFERS, dict(d_sums_out=weights + 4 * N - 8), "overlap"), (BUFFERS, dict(d_weights=own), "engine"),
        (OK, dict(d_weights=keys)),                                                  # two inputs may share memory: only the output is exclusive
        # two faults: a limit before a pointer, a misaligned pointer before an overlap
        (CALC, dict(flags=1, d_keys=None)), (CALC, dict(n=(1 << 31) + 1, d_keys=keys + 4)), (CALC, dict(weight_kind=3, d_weights=None)),
        (BUFFERS, dict(d_keys=keys + 4, d_sums_out=off), "aligned"),
    ]
    if is_float:
        rows += [(CALC, dict(width_shift=1), "width_shift"), (CALC, dict(lo_bits=f32(8.0)), "lo < hi"), (CALC, dict(hi_bits=f32(np.inf)), "finite"),
                 (CALC, dict(lo_bits=f32(np.nan)), "finite"), (CALC, dict(lo_bits=f32(-3e38), hi_bits=f32(3e38)), "finite positive")]
    else:
        rows += [(CALC, dict(hi_bits=1), "hi_bits"), (CALC, dict(width_shift=8 * kb), "width_shift"), (OK, dict(width_shift=8 * kb - 1))]
    edge_rows = [
        (OK, dict()), (OK, dict(num_bins=1)), (OK, dict(flags=SIGNED)),
        (CALC, dict(num_bins=4097), "4096"), (CALC, dict(lo_bits=1), "edges form"), (CALC, dict(hi_bits=1), "edges form"),
        (CALC, dict(width_shift=1), "edges form"), (CALC, dict(flags=2)),
        (BUFFERS, dict(d_edges=edges + kb // 2), "edges"), (BUFFERS, dict(d_edges=own), "engine"),
        (BUFFERS, dict(d_sums_out=edges), "overlap"), (BUFFERS, dict(d_sums_out=edges + B * kb), "overlap"),
        (OK, dict(d_sums_out=edges + (B + 1) * kb + (4 if kb == 4 else 0))),
    ]
    lib = rsx.load_library()

    def call(args):
        rc = lib.rsx_segmented_weighted_histogram(eng._h, *[args[k] for k in ORDER])
        return rc, lib.rsx_last_error().decode()

    null_rc = lib.rsx_segmented_weighted_histogram(None, *[even[k] for k in ORDER])
    assert null_rc == CALC and "rsx_segmented_weighted_histogram: null engine" in lib.rsx_last_error().decode()
    for base, table in ((even, rows), (with_edges, edge_rows)):
        for row in table:
            status, change = row[0], row[1]
            arena[3 * slot:3 * slot + 8 * S * B] = 0xC3
            rc, msg = call(dict(base, **change))
            t.cuda.synchronize()                                                 # (an accepted row runs on the engine's stream: before the next fill)
            assert rc == status, (row, msg)
            if status != OK:
                assert "rsx_segmented_weighted_histogram" in msg and (len(row) < 3 or row[2] in msg), (row, msg)
                assert bool((arena[3 * slot:3 * slot + 8 * S * B] == 0xC3).all()), ("a refused call wrote something", row)
    eng.sync()
    assert call(even)[0] == OK                                                     # and the call these were variations of works: all keys are zero
    eng.sync()
    got = arena[3 * slot:3 * slot + 8 * S * B].cpu().numpy().view(np.int64).reshape(S, B)
    assert got[:, 0].tolist() == [(N // 2) << 30, (N - N // 2) << 30] and np.all(got[:, 1:] == 0)        # 0.5 weighs 2^30


def test_helper_refusals(rsx):
    """the torch helpers' own refusals on device tensors of at most 16 elements; 'more than 2^31' on a stride-0 view of one element"""
    t = _torch()
    x = t.arange(6, dtype=t.int32, device="cuda")
    f = t.linspace(0, 1, 6, device="cuda")
    w = t.ones(6, device="cuda")
    off = t.tensor([0, 3, 6], device="cuda")
    huge = t.zeros(1, dtype=t.int32, device="cuda").expand((1 << 31) + 1)
    hugew = t.zeros(1, dtype=t.float32, device="cuda").expand((1 << 31) + 1)
    for exc, pattern, call in (
            (ValueError, "shaped like the keys", lambda: rsx.segmented_weighted_histogram(x, off, w[:5], 4)),
            (ValueError, "device tensor", lambda: rsx.segmented_weighted_histogram(x, off, w.cpu(), 4)),
            (TypeError, "unsupported weight type", lambda: rsx.segmented_weighted_histogram(x, off, w.half(), 4)),
            (ValueError, "1-D", lambda: rsx.segmented_weighted_histogram(x.reshape(2, 3), off, w.reshape(2, 3), 4)),
            (ValueError, "2\\^31 elements and 2\\^30 sums", lambda: rsx.segmented_weighted_histogram(huge, None, hugew, 4, weight_max=1.0)),
            (ValueError, "2\\^31 elements and 2\\^30 sums", lambda: rsx.segmented_weighted_histogram(x, None, w, (1 << 30) + 1, weight_max=1.0)),
            (ValueError, "at least one bin", lambda: rsx.segmented_weighted_histogram(x, off, w, 0)),
            (ValueError, "shaped like", lambda: rsx.bincount(x, num_bins=4, weights=w[:5])),
            (ValueError, "shaped like ids", lambda: rsx.bincount_rows(x.reshape(2, 3), 4, weights=w)),
            (ValueError, "shaped like the input", lambda: rsx.histogram(f, 4, range=(0.0, 1.0), weight=w[:5])),
            (ValueError, "shaped like the input", lambda: rsx.histogram_rows(f.reshape(2, 3), 4, range=(0.0, 1.0), weight=w)),
            (ValueError, "device tensor", lambda: rsx.bincount(x, num_bins=4, weights=w.cpu())),
            (TypeError, "integer tensor", lambda: rsx.bincount(f, weights=w))):
        with pytest.raises(exc, match=pattern):
            call()


# -- 12. the helpers against torch and numpy ---------------------------------------------------------------------------------------------------------------------------------------------

def test_helpers_against_torch(rsx):
    t = _torch()
    rng = np.random.default_rng(5)
    n = 50000
    xh = rng.integers(0, 1000, n)
    x = t.from_numpy(xh).cuda()
    for dt in (np.float32, np.float64):
        wh = W.dyadic_weights(rng, n, dt)                                            # multiples of 2^-20 in [-1, 1]: both sides are exact
        w = t.from_numpy(wh).cuda()
        want = t.bincount(x, weights=w.double())
        got = rsx.bincount(x, weights=w)
        assert got.dtype == t.float64 and t.equal(got, want)
        assert t.equal(rsx.bincount(x, weights=w, weight_max=1.0), want)
        assert t.equal(rsx.bincount(x, minlength=2000, weights=w), t.bincount(x, weights=w.double(), minlength=2000))
        assert t.equal(rsx.bincount(x, num_bins=300, weights=w, weight_max=1.0), want[:300])
        assert t.equal(rsx.bincount(x[::3], weights=w[::3]), t.bincount(x[::3], weights=w[::3].double()))       # strided inputs are copied
        assert t.equal(rsx.bincount(x[1:], weights=w[1:]), t.bincount(x[1:], weights=w[1:].double()))         # weights one element past a boundary
        # histogram with edges and with a range against numpy
        f = t.from_numpy(rng.integers(-40, 100, n).astype(dt)).cuda()
        e = t.tensor([-50.0, -40.0, -3.5, 0.0, 0.5, 64.0, 99.0], dtype=f.dtype, device="cuda")
        sums, edges = rsx.histogram(f, e, weight=w)
        assert edges is e and np.array_equal(sums.cpu().numpy(), np.histogram(f.cpu().numpy(), bins=e.cpu().numpy(), weights=wh.astype(np.float64))[0])
        sums, edges = rsx.histogram(f, 16, range=(-32.0, 32.0), weight=w, weight_max=1.0)
        assert np.array_equal(sums.cpu().numpy(), np.histogram(f.cpu().numpy(), bins=16, range=(-32.0, 32.0), weights=wh.astype(np.float64))[0])
        fr, wr = f[:49920].reshape(4, 5, 2496), w[:49920].reshape(4, 5, 2496)
        sums, _ = rsx.histogram_rows(fr, e, weight=wr)
        want_rows = np.stack([np.histogram(r, bins=e.cpu().numpy(), weights=q.astype(np.float64))[0]
                              for r, q in zip(fr.cpu().numpy().reshape(-1, 2496), wr.cpu().numpy().reshape(-1, 2496))]).reshape(4, 5, 6)
        assert np.array_equal(sums.cpu().numpy(), want_rows)
    # integer weights are masses: int64 sums; an empty input
    wi = t.from_numpy(rng.integers(0, 1 << 31, n).astype(np.int32)).cuda()
    got = rsx.bincount(x, weights=wi)
    assert got.dtype == t.int64 and np.array_equal(got.cpu().numpy(), W.exact_sums(xh, wi.cpu().numpy(), int(xh.max()) + 1))
    assert rsx.bincount(x[:0], weights=w[:0]).numel() == 0
    assert t.equal(rsx.bincount(x[:0], minlength=5, weights=w[:0]), t.zeros(5, dtype=t.float64, device="cuda"))
    # the masses themselves, and the unsigned rule
    m = rsx.segmented_weighted_histogram(x.to(t.int32), None, w, 1000, weight_max=1.0, return_mass=True)
    assert m.dtype == t.int64 and np.array_equal(m.cpu().numpy(), whistogram_oracle(xh.astype(np.int32), wh, None, 1000, signed=True))
    m = rsx.segmented_weighted_histogram(x.to(t.int32), None, w, 1000, weight_max=1.0, signed=False, return_mass=True)
    assert np.array_equal(m.cpu().numpy(), whistogram_oracle(xh.astype(np.int32), wh, None, 1000, signed=False))
    # weight_max None: the exponent comes from the data (0.25 at most: e = -2, four times finer units)
    m = rsx.segmented_weighted_histogram(x.to(t.int32), None, w / 4, 1000, return_mass=True)
    assert np.array_equal(m.cpu().numpy(), whistogram_oracle(xh.astype(np.int32), wh / 4, None, 1000, weight_exp=-2, signed=True))


def test_router_gate_mass_per_expert(rsx):
    t = _torch()
    rng = np.random.default_rng(6)
    ids_h = rng.integers(-1, 9, (5, 300))                                             # ids outside [0, 8) are dropped
    gate_h = W.dyadic_weights(rng, 1500).reshape(5, 300)
    ids, gate = t.from_numpy(ids_h).cuda(), t.from_numpy(gate_h).cuda()
    got = rsx.bincount_rows(ids, 8, weights=gate)
    want = np.stack([np.bincount(r[(r >= 0) & (r < 8)], weights=g[(r >= 0) & (r < 8)].astype(np.float64), minlength=8) for r, g in zip(ids_h, gate_h)])
    assert got.shape == (5, 8) and got.dtype == t.float64 and np.array_equal(got.cpu().numpy(), want)
    assert t.equal(rsx.bincount_rows(ids.to(t.int32), 8, weights=gate.double(), weight_max=1.0), got)
    # without weights the wrappers are what they were
    assert t.equal(rsx.bincount_rows(ids, 8), t.stack([t.bincount(r[(r >= 0) & (r < 8)], minlength=8) for r in ids]))


def test_weight_max_given_reads_nothing_back(rsx):
    """with weight_max the helpers synchronise nowhere: the calls are captured (a read-back would fail the capture) and replayed"""
    t = _torch()
    rng = np.random.default_rng(7)
    n = 5000
    x = t.from_numpy(rng.integers(0, 64, n)).cuda()
    w = t.from_numpy(W.dyadic_weights(rng, n)).cuda()
    f = x.to(t.float32)
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):                                                         # eager on this stream: its engines and their status words exist
        rsx.bincount(x, num_bins=64, weights=w, weight_max=1.0)
        rsx.histogram(f, 16, range=(0.0, 64.0), weight=w, weight_max=1.0)
    side.synchronize()
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        a = rsx.bincount(x, num_bins=64, weights=w, weight_max=1.0)
        b, _ = rsx.histogram(f, 16, range=(0.0, 64.0), weight=w, weight_max=1.0)
    for rep in range(2):
        w.copy_(t.from_numpy(W.dyadic_weights(rng, n)).cuda())
        t.cuda.synchronize()
        graph.replay()
        t.cuda.synchronize()
        want = t.bincount(x, weights=w.double(), minlength=64)
        assert t.equal(a, want) and t.equal(b, want.reshape(16, 4).sum(1))
    del graph
