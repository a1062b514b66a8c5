"""rsx_segmented_histogram on the paths of rsx_bins.hpp and rsx_bin_math.hpp that tests/test_gpu_histogram.py never reaches: the bin
arithmetic ON THE DEVICE (the round-to-nearest intrinsics and codec_encode, where the CPU selftest runs their host twins) on the keys one
ulp either side of every bin boundary; all 16 piece slots of a tile and pieces of 255, 256 and 257 keys; B at the boundary between the
wave-private and the shared counters; the zero fill's element-store head and tail at every alignment and the second trip of its
grid-stride loop.

The cases and layouts are held in tests/_histogram_ref.py, where tests/test_histogram.py sends the same keys through the g++ build of
the arithmetic and checks from the layouts alone that each reaches the path it is named after.  Every comparison is exact equality with
histogram_oracle; sentinel fill and guard bands as in test_gpu_histogram.py, with the bytes in front of the counters a parameter.
"""
import numpy as np
import pytest

import _histogram_ref as H
from _histogram_ref import NO_BIN, bins_of, histogram_oracle
from test_gpu_histogram import CAP, GUARD_BYTE, check
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, GUARD

pytestmark = pytest.mark.gpu


def run(rsx, keys, off, bins, lo=0, hi=0, shift=0, descending=False, eng=None, front=12):
    """test_gpu_histogram.run with `front` bytes of sentinel before the counters (the buffer itself is 16-byte aligned: the counters lie
    front % 16 bytes past a 16-byte boundary).  Returns (counts [S, B] int64, engine)."""
    t = _torch()
    n = keys.size
    nseg = 1 if off is None else len(off) - 1
    even = np.isscalar(bins)
    B = int(bins) if even else len(bins) - 1
    k = dev(t, keys) if n else None
    o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
    e = None if even else dev(t, np.ascontiguousarray(bins, dtype=keys.dtype))
    out = dev(t, np.concatenate([np.full(front + nseg * B * 4, FILL, dtype=np.uint8), np.full(GUARD, GUARD_BYTE, dtype=np.uint8)]))
    assert out.data_ptr() % 16 == 0 and front % 4 == 0
    if eng is None:
        eng = rsx.Engine(keys.dtype, CAP, descending=descending)
    eng.segmented_histogram(k.data_ptr() if n else None, n, None if o is None else o.data_ptr(), nseg, B, out.data_ptr() + front,
                            d_edges=None if even else e.data_ptr(), lo=lo, hi=hi, width_shift=shift)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    raw = out.cpu().numpy().view(np.uint8)
    assert np.all(raw[-GUARD:] == GUARD_BYTE), "guard band written"
    assert np.all(raw[:front] == FILL), "bytes before the counters written"
    return raw[front:-GUARD].copy().view(np.uint32).astype(np.int64).reshape(nseg, B), eng


def run_check(rsx, keys, off, what="", **kw):
    got, eng = run(rsx, keys, off, **kw)
    ref_kw = {k: v for k, v in kw.items() if k in ("bins", "lo", "hi", "shift", "descending")}
    check(got, histogram_oracle(keys, off, **ref_kw), what)
    return got, eng


# -- H1. the bin arithmetic on the device ----------------------------------------------------------------------------------------------------

def send_case(rsx, eng, keys, what, **args):
    """the case's keys as one segment, as two, and in pieces of 255 (tests/test_histogram.py: LDS, LDS, direct)"""
    for name, n, off in H.arith_forms(keys.size):
        run_check(rsx, np.resize(keys, n), off, f"{what}, {name}", eng=eng, **args)


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt", H.DTYPES)
def test_edges_form_around_every_edge(rsx, dt, descending):
    """test_selftest_edges_form's keys through codec_encode and the LDS bisection: every edge and the keys next to it, -0.0 and +0.0 as
    two edges, B = 4096 and B = 1"""
    eng = rsx.Engine(dt, CAP, descending=descending)
    for B, edges, keys in H.edges_cases(dt, descending):
        want = bins_of(keys, edges, descending=descending)
        assert np.any(want == NO_BIN) and np.any(want == B - 1) and np.any(want == 0)
        send_case(rsx, eng, keys, f"edges B={B}", bins=edges, descending=descending)
    eng.sync()


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt", ["uint32", "int32", "uint64", "int64"])
def test_even_integer_form_around_every_boundary(rsx, dt, descending):
    """test_selftest_even_integer_form's keys: lo at info.min and at info.max - 70, width_shift up to width - 1"""
    eng = rsx.Engine(dt, CAP, descending=descending)
    seen = set()
    for shift, lo, B, keys in H.even_int_cases(dt, descending):
        want = bins_of(keys, B, lo=lo, shift=shift, descending=descending)
        assert np.any(want != NO_BIN) and (np.any(want == NO_BIN) or (B << shift) >> (8 * np.dtype(dt).itemsize - 1) != 0)       # keys are dropped unless the bins cover half the type
        seen.add((shift, lo))
        send_case(rsx, eng, keys, f"even shift={shift} lo={lo} B={B}", bins=B, lo=lo, shift=shift, descending=descending)
    info = np.iinfo(dt)
    assert {(8 * np.dtype(dt).itemsize - 1, info.max - 70), (0, info.max - 70)} <= seen and (np.dtype(dt).kind == "u" or (5, info.min) in seen)
    eng.sync()


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_even_float_form_one_ulp_either_side(rsx, dt, descending):
    """test_selftest_even_float_form's keys through __fsub_rn / __fmul_rn / __dsub_rn / __dmul_rn and the device's float-to-uint
    conversion: x = lo + b / scale and its neighbours; B = 50257 is the direct path by itself"""
    eng = rsx.Engine(dt, CAP, descending=descending)
    for B, lo, hi, keys in H.even_float_cases(dt, descending):
        want = bins_of(keys, B, lo=lo, hi=hi, descending=descending)
        H.even_float_case_holds(keys, B, lo, hi, want, descending)
        send_case(rsx, eng, keys, f"even B={B} [{lo}, {hi}]", bins=B, lo=lo, hi=hi, descending=descending)
    eng.sync()


# -- H2. piece slots ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [64, 4096], ids=["64 even uint32", "4096 edges uint64"])
@pytest.mark.parametrize("name", list(H.SLOT_LAYOUTS))
def test_piece_slots(rsx, name, B):
    """16 LDS pieces in one tile, pieces of 255 / 256 / 257 keys, a piece that ends with its tile; segment s counts in bins s, s + 1, s + 2
    (mod B), so that a count credited to a neighbour shows"""
    rng = np.random.default_rng(200 + B + list(H.SLOT_LAYOUTS).index(name))
    n, off = H.SLOT_LAYOUTS[name]()
    b = H.shifted_bins(rng, n, off, B)
    if B == 64:
        got, eng = run_check(rsx, b.astype(np.uint32), off, name, bins=B)
    else:
        step = H.SLOT_EDGE_STEP
        keys = (b.astype(np.uint64) * np.uint64(step) + np.uint64(step // 2))
        got, eng = run_check(rsx, keys, off, name, bins=np.arange(B + 1, dtype=np.uint64) * np.uint64(step))
    o = off.astype(np.int64)
    assert 0 < got.sum() < int(o[-1] - o[0])
    eng.sync()


# -- H3. B at the boundary between the wave-private and the shared counters ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", H.BOUNDARY_BINS)
def test_bins_at_the_counter_layout_boundary(rsx, B):
    assert H.lds_layout(B) == ("wave_private" if B <= 1024 else "shared")
    n, off = H.ragged_layout()
    for dt in ("uint32", "float64"):
        eng = rsx.Engine(dt, CAP)
        for form in ("even", "edges"):
            rng = np.random.default_rng(3000 + B + (form == "edges"))
            args = H.form_args(dt, form, False, B, rng)
            got, _ = run_check(rsx, H.case_keys(rng, dt, n, off, args), off, f"{dt} {form} B={B}", eng=eng, **args)
            assert got.sum() > 0
        eng.sync()
    n = H.SKEW_N
    eng = rsx.Engine(np.uint32, CAP)
    for what, keys in (("bin B - 1 alone", np.full(n, B - 1, dtype=np.uint32)), ("bin 0 alone", np.zeros(n, dtype=np.uint32)),
                       ("one key a bin", (np.arange(n) % B).astype(np.uint32)),
                       ("an alternating pair", np.where(np.arange(n) % 2 == 0, 0, B - 1).astype(np.uint32))):
        got, _ = run_check(rsx, keys, None, what, eng=eng, bins=B)
        assert got.sum() == n
    eng.sync()


# -- H4. the zero fill --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", H.ZERO_ALIGN)
def test_zero_fill_of_a_few_counters(rsx, align):
    """S * B in {1, 2, 3, 4, 5, 7, 8, 9} counters that start `align` bytes past a 16-byte boundary: the head, the tail, no 16-byte store at
    all; with a few keys and with none"""
    rng = np.random.default_rng(align)
    eng = rsx.Engine(np.uint32, CAP)
    for total, (S, B) in H.ZERO_SMALL.items():
        n, off = H.zero_small_layout(S)
        keys = rng.integers(0, B + 1, n).astype(np.uint32)
        got, _ = run_check(rsx, keys, off, f"{S} x {B} at {align}", eng=eng, bins=B, front=16 + align)
        assert got.shape == (S, B)
        got, _ = run_check(rsx, keys[:0], np.zeros(S + 1, dtype=np.uint64), f"{S} x {B} at {align}, no keys", eng=eng, bins=B, front=16 + align)
        assert np.all(got == 0)
    eng.sync()


def test_zero_fill_second_trip(rsx):
    """2^16 + 1 segments x 65 bins = 4,259,905 counters at 4 mod 16: the grid-stride loop of bins_zero_kernel goes round twice on 256 CUs;
    a counter it missed keeps the sentinel"""
    rng = np.random.default_rng(65)
    n, off = H.zero_big_layout()
    B = H.ZERO_BIG_BINS
    assert (len(off) - 1) * B / 4 > 256 * 16 * 256
    keys = rng.integers(0, B + 3, n).astype(np.uint32)
    got, eng = run_check(rsx, keys, off, "zero fill, second trip", bins=B, front=16 + 4)
    assert 0 < got.sum() < n
    eng.sync()
