"""Segmented top-k at the shapes it is built for, on the GPU: many vocabulary-wide rows (tile groups of the select rounds that hold
the end of one segment and the start of the next, pick and final-sort grids that stride over segments), keys that differ in one digit
of the select only, keys equal to the LDS sorts' pad, the torch helper on logits, one engine across shapes and calls, and capture and
replay.

Every answer is compared bit for bit (keys and positions) with the linear-time host reference of tests/_topk_ref.py, computed once per
layout and direction at k = 4096 and cut to each k.  Outputs start out holding a sentinel that must survive in the slots the call may
not write, inside guard bands that must come back untouched.  tests/test_topk.py checks that each layout here still reaches its path.
"""
import numpy as np
import pytest

import _topk_ref as R
from test_gpu_float_keys import UINT, random_bits
from test_gpu_segmented import DTYPES, _torch, dev, offsets_from
from test_gpu_segmented import check as seg_check
from test_gpu_segmented import run as seg_run
from test_gpu_topk import GUARD, IDX_FILL, KEY_FILL

pytestmark = pytest.mark.gpu


class Guarded:
    """A device byte buffer of `nbytes` between guard bands; refill() puts the sentinel back, body() checks the bands and reads."""

    def __init__(self, t, nbytes):
        self.nbytes = nbytes
        self.buf = t.empty(GUARD + nbytes + GUARD, dtype=t.uint8, device="cuda")
        self.buf[:GUARD] = 0x5A
        self.buf[GUARD + nbytes:] = 0xA5
        self.ptr = self.buf.data_ptr() + GUARD

    def refill(self, t, fill):
        if isinstance(fill, np.ndarray):
            self.buf[GUARD:GUARD + self.nbytes].copy_(t.from_numpy(fill.view(np.uint8)))
        else:
            self.buf[GUARD:GUARD + self.nbytes] = fill

    def body(self):
        b = self.buf.cpu().numpy()
        assert np.all(b[:GUARD] == 0x5A) and np.all(b[GUARD + self.nbytes:] == 0xA5), "guard band written"
        return b[GUARD:GUARD + self.nbytes].copy()


def topk_on(t, eng, kd, n, od, nseg, k, u):
    """One segmented_topk of device keys kd / offsets od into fresh sentinel-filled guarded outputs: (keys [S, k], positions [S, k])."""
    ko, io = Guarded(t, nseg * k * np.dtype(u).itemsize), Guarded(t, nseg * k * 4)
    ko.refill(t, KEY_FILL)
    io.refill(t, KEY_FILL)
    t.cuda.synchronize()                  # the fills run on torch's stream, the engine on its own
    eng.segmented_topk(kd.data_ptr(), n, od.data_ptr(), nseg, k, ko.ptr, io.ptr)
    eng.sync()
    return ko.body().view(u).reshape(nseg, k), io.body().view(np.uint32).reshape(nseg, k)


def expect(ref, k, got_k, got_i, what=""):
    wk, wi, written = ref.at(k)
    u = got_k.dtype
    fill_k = np.frombuffer(bytes([KEY_FILL]) * u.itemsize, dtype=u)[0]
    bad = np.argwhere(got_k != np.where(written, wk, fill_k))
    assert bad.size == 0, f"{what} k={k}: keys differ at (segment, slot) {bad[:8].tolist()} (of {len(bad)})"
    bad = np.argwhere(got_i != np.where(written, wi, np.uint32(IDX_FILL)))
    assert bad.size == 0, f"{what} k={k}: positions differ at (segment, slot) {bad[:8].tolist()} (of {len(bad)})"


def run_layout(rsx, x, off, ks, what=""):
    """Every k of `ks` in both directions on one upload, against one reference per direction."""
    t = _torch()
    n, nseg, u = x.size, len(off) - 1, UINT[x.dtype]
    kd, od = dev(t, x), dev(t, np.asarray(off, dtype=np.uint64))
    for desc in (False, True):
        ref = R.fast_topk(x, off, max(ks), desc)
        eng = rsx.Engine(x.dtype, n, descending=desc)
        for k in ks:
            gk, gi = topk_on(t, eng, kd, n, od, nseg, k, u)
            expect(ref, k, gk, gi, f"{what} {'desc' if desc else 'asc'}")
        eng.close()


# -- 3. many large rows, shared tile groups ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_many_large_rows(rsx, shape):
    dtype, make = R.SHAPES[shape]
    off = make()
    n = R.shape_n(off)
    rng = np.random.default_rng(list(R.SHAPES).index(shape) + 100)
    if np.dtype(dtype).kind == "f":
        x = rng.standard_normal(n).astype(dtype) * 4                          # logits: rounded, so values repeat within a row
        x = np.round(x * 64) / 64 + dtype(0.0)
        x[rng.integers(0, n, n // 50)] = random_bits(dtype, n // 50, rng)     # and every bit pattern: NaNs, ±inf, -0.0
    elif shape == "64x151936_i64":
        x = rng.integers(-(1 << 40), 1 << 40, n).astype(dtype)
        x[::3] = rng.integers(-20, 20, x[::3].size)                           # long tie runs in the middle of the order
    else:
        x = random_bits(dtype, n, rng)
        x[rng.integers(0, n, n // 3)] = x[rng.integers(0, n, n // 3)]
    run_layout(rsx, x, off, R.SHAPE_KS, shape)


# -- 4. keys that differ in one digit of the select --------------------------------------------------------------------------------

DIGIT_LENGTHS = [300, 70000, 5000, 1025, 4097, 20000, 9000, (1 << 18) + 5, 2, 4096, 33333, 12000, (1 << 17) + 1, 7000, 50000, 256]


@pytest.mark.parametrize("variant", ["window", "low", "straddle"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_digit_local_keys(rsx, dtype, variant):
    t = _torch()
    off = offsets_from(DIGIT_LENGTHS * 2, start=1)
    n = int(off[-1]) + 2
    nseg, u = len(off) - 1, UINT[np.dtype(dtype)]
    ks = (1000,) if variant == "straddle" else (1, 1000, 4096)
    for desc in (False, True):
        rng = np.random.default_rng(DTYPES.index(dtype) * 8 + 2 * ["window", "low", "straddle"].index(variant) + desc)
        x = R.digit_local(dtype, off, n, rng, variant, desc, k=1000)
        ref = R.fast_topk(x, off, max(ks), desc)
        kd, od = dev(t, x), dev(t, off)
        eng = rsx.Engine(dtype, n, descending=desc)
        for k in ks:
            gk, gi = topk_on(t, eng, kd, n, od, nseg, k, u)
            expect(ref, k, gk, gi, f"{variant} {'desc' if desc else 'asc'}")
        eng.close()


# -- 5. keys equal to the pad --------------------------------------------------------------------------------------------------------

PAD_LENGTHS = [256, 257, 1024, 1025, 4096, 4097, 3 * 4096 + 77, 2, 100003, 4095, (1 << 18) + 1, 1, 255, 9001]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_keys_equal_to_the_pad(rsx, dtype):
    t = _torch()
    off = offsets_from(PAD_LENGTHS, start=5)                                  # large segments with partial tiles at both ends
    n = int(off[-1]) + 3
    nseg, u = len(off) - 1, UINT[np.dtype(dtype)]
    for desc in (False, True):
        rng = np.random.default_rng(DTYPES.index(dtype) * 2 + desc + 200)
        x = R.pad_heavy(dtype, off, n, rng, desc)
        ref = R.fast_topk(x, off, 4096, desc)
        kd, od = dev(t, x), dev(t, off)
        eng = rsx.Engine(dtype, n, descending=desc)
        for k in (7, 1000, 4096):
            gk, gi = topk_on(t, eng, kd, n, od, nseg, k, u)
            expect(ref, k, gk, gi, f"pad {'desc' if desc else 'asc'}")
        eng.close()
        sk, sp, seng = seg_run(rsx, x, off, desc, payload=True)                # the segmented sort pads its LDS sorts the same way
        seg_check(x, off, sk, sp, desc, payload=True)
        seng.close()


# -- 6. the torch helper at vocabulary shapes ----------------------------------------------------------------------------------------

def _logits(t, rows, cols, seed):
    g = t.Generator(device="cuda").manual_seed(seed)
    x = t.randn((rows, cols), device="cuda", generator=g) * 3
    x = t.round(x * 8) / 8 + 0.0                                             # real ties; + 0.0 turns -0.0 into +0.0
    mask = t.rand((rows, cols), device="cuda", generator=g) < 0.6            # a large -inf mask
    mask[rows // 2:] = False
    x[mask] = float("-inf")
    x[: rows // 8] = float("-inf")                                           # rows with fewer than k finite values: the k-th is a -inf tie
    for r in range(rows // 8):
        keep = t.randint(0, cols, (r % 1100,), device="cuda", generator=g)
        x[r, keep] = t.round(t.randn(keep.numel(), device="cuda", generator=g) * 8) / 8 + 0.0
    return x


@pytest.mark.parametrize("rows,cols", [(4096, 32000), (512, 50257)], ids=["4096x32000", "512x50257"])
def test_topk_helper_vocab_shapes(rsx, rows, cols):
    t = _torch()
    x = _logits(t, rows, cols, rows)
    _, si = t.sort(x, dim=-1, descending=True, stable=True)
    si = si[:, :1024].clone()
    for k in (1, 50, 1024):
        v, i = rsx.topk(x, k)
        wv, _ = t.topk(x, k)
        assert t.equal(v, wv), f"k={k}: values differ from torch.topk in {int((v != wv).any(dim=1).sum())} rows"
        assert t.equal(i, si[:, :k]), f"k={k}: indices differ from the stable sort in {int((i != si[:, :k]).any(dim=1).sum())} rows"
    if rows == 512:
        xh = x.cpu().numpy()
        ref = R.fast_topk(xh.reshape(-1), R.rows(rows, cols), 1024, descending=True)
        v, i = rsx.topk(x, 1024)
        expect(ref, 1024, v.cpu().numpy().view(np.uint32), i.cpu().numpy().astype(np.uint32), "helper")


# -- 7. one engine across shapes and calls -------------------------------------------------------------------------------------------

def test_one_engine_across_shapes_and_calls(rsx):
    t = _torch()
    rng = np.random.default_rng(77)
    small = offsets_from([300, 5000, 70000, 9000, 4097], start=1)
    large = R.rows(1500, 6001, start=3)                                      # more large segments and tiles: the scratch grows
    n_small, n_large = int(small[-1]) + 1, int(large[-1]) + 1
    eng = rsx.Engine(np.uint32, n_large)
    xs = random_bits(np.uint32, n_small, rng)
    xl = random_bits(np.uint32, n_large, rng)
    xl[::5] = xl[11]
    ref_s, ref_l = R.fast_topk(xs, small, 1000), R.fast_topk(xl, large, 4096)
    ds, dos = dev(t, xs), dev(t, small)
    dl, dol = dev(t, xl), dev(t, large)
    for k in (1000, 64):
        expect(ref_s, k, *topk_on(t, eng, ds, n_small, dos, len(small) - 1, k, np.uint32), "small")
    for k in (4096, 50):
        expect(ref_l, k, *topk_on(t, eng, dl, n_large, dol, len(large) - 1, k, np.uint32), "large")
    expect(ref_s, 1000, *topk_on(t, eng, ds, n_small, dos, len(small) - 1, 1000, np.uint32), "small again")
    with pytest.raises(rsx.RadixSortError):                                  # top-k used keys[0] / keys[1] as scratch: no result to download
        eng.download()
    sk, sp, _ = seg_run(rsx, xl, large, False, payload=False, eng=eng)
    seg_check(xl, large, sk, sp, False, payload=False)
    keys = random_bits(np.uint32, (1 << 20) + 3, rng)
    eng.upload(keys)
    eng.sort()
    assert np.array_equal(eng.download(), np.sort(keys))
    expect(ref_l, 1000, *topk_on(t, eng, dl, n_large, dol, len(large) - 1, 1000, np.uint32), "large after a sort")
    eng.close()


# -- 8. capture and replay -----------------------------------------------------------------------------------------------------------

CAPTURE_LENGTHS = [5000, 300, 70000, 4097, 1025, 20000, 1, 9000, 0, 130001]


def test_capture_and_replay(rsx):
    t = _torch()
    rng = np.random.default_rng(88)
    k = 1000
    off = offsets_from(CAPTURE_LENGTHS, start=1)
    n, nseg = int(off[-1]) + 2, len(off) - 1
    u = np.uint32
    side = t.cuda.Stream()
    eng = rsx.Engine(np.float32, n, payload=True, descending=True)
    eng.set_stream(side.cuda_stream)
    x = random_bits(np.float32, n, rng)
    kd, od = dev(t, x), dev(t, off)
    pd = dev(t, np.arange(n, dtype=np.uint32))
    tk, ti = Guarded(t, nseg * k * 4), Guarded(t, nseg * k * 4)
    sk, sp = Guarded(t, n * 4), Guarded(t, n * 4)

    def calls():
        eng.segmented_topk(kd.data_ptr(), n, od.data_ptr(), nseg, k, tk.ptr, ti.ptr)
        eng.segmented_sort(kd.data_ptr(), n, od.data_ptr(), nseg, sk.ptr, pd.data_ptr(), sp.ptr)

    def refill(xv):
        tk.refill(t, KEY_FILL)
        ti.refill(t, KEY_FILL)
        sk.refill(t, ~xv.view(u))
        sp.refill(t, ~np.arange(n, dtype=np.uint32))

    def verify(xv, ov, what):
        expect(R.fast_topk(xv, ov, k, True), k, tk.body().view(u).reshape(nseg, k), ti.body().view(np.uint32).reshape(nseg, k), what)
        seg_check(xv, ov, sk.body().view(np.float32), sp.body().view(np.uint32), True, payload=True)

    refill(x)
    t.cuda.synchronize()
    calls()                                                                  # eager: sizes every buffer of this (n, segment count)
    eng.sync()
    verify(x, off, "eager")

    g = t.cuda.CUDAGraph()
    with t.cuda.graph(g, stream=side):
        calls()
    for rep in range(2):                                                     # new keys and offsets in the captured buffers
        x = random_bits(np.float32, n, rng)
        x[rng.integers(0, n, n // 4)] = x[rng.integers(0, n, n // 4)]
        lens = list(rng.permutation(CAPTURE_LENGTHS))
        lens[-1] += 1 - rep
        off = offsets_from(lens, start=rep)                                   # same segment count, ends within n
        assert len(off) - 1 == nseg and int(off[-1]) <= n
        kd.copy_(t.from_numpy(x.view(np.int32)))
        od.copy_(t.from_numpy(off.view(np.int64)))
        refill(x)
        t.cuda.synchronize()
        g.replay()
        t.cuda.synchronize()
        verify(x, off, f"replay {rep}")
    del g

    # a fresh engine cannot size its buffers inside a capture, nor grow them after a smaller eager call: refused by name (nothing is
    # captured), and fine eagerly afterwards
    fresh = rsx.Engine(np.float32, n, descending=True)
    fresh.set_stream(side.cuda_stream)
    small = offsets_from([100, 5000, 300])
    ds, dos = dev(t, x[:5400].copy()), dev(t, small)
    for first in (True, False):
        if not first:
            expect(R.fast_topk(x[:5400], small, 50, True), 50, *topk_on(t, fresh, ds, 5400, dos, 3, 50, u), "small eager")
        g2 = t.cuda.CUDAGraph()
        with t.cuda.graph(g2, stream=side):
            with pytest.raises(rsx.RadixSortError) as ei:
                fresh.segmented_topk(kd.data_ptr(), n, od.data_ptr(), nseg, k, tk.ptr, ti.ptr)
        assert "capture" in str(ei.value), str(ei.value)
        del g2
    refill(x)
    t.cuda.synchronize()
    fresh.segmented_topk(kd.data_ptr(), n, od.data_ptr(), nseg, k, tk.ptr, ti.ptr)
    fresh.sync()
    expect(R.fast_topk(x, off, k, True), k, tk.body().view(u).reshape(nseg, k), ti.body().view(np.uint32).reshape(nseg, k), "after capture")
    fresh.close()
    eng.close()
