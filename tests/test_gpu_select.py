"""Segmented select (rsx_segmented_select, radix_sort_amd.segmented_select / kthvalue / median / quantile) on the GPU.

The referee is entry `rank` of every valid segment's stable argsort of the order-mapped keys (tests/_select_ref.py), compared bit for
bit: keys AND positions.  The outputs start out holding a sentinel that must survive in every slot the call may not write (ranks not
below the segment's length, rows of invalid segments) and sit inside guard bands that must come back untouched.  Lengths reach every
path: one-key segments, the three LDS classes (<= 256, <= 1024, <= 4096 keys) and the select chain over the tiles of larger segments.
"""
import numpy as np
import pytest

import _topk_ref
from _select_ref import NONE, fast_select, random_ranks, select_oracle
from test_gpu_float_keys import UINT, random_bits, special
from test_gpu_segmented import DTYPES, _torch, dev, offsets_from

pytestmark = pytest.mark.gpu

GUARD = 64
KEY_FILL, IDX_FILL = 0xC3, 0xC3C3C3C3


def run(rsx, x, off, ranks, descending=False, eng=None, out_shift=0):
    """One rsx_segmented_select through the Engine API, outputs inside guard bands and pre-filled with the sentinel.
    Returns (keys [S, R] unsigned words, positions [S, R] uint32, engine)."""
    t = _torch()
    n = x.size
    nseg = len(off) - 1
    ranks = np.ascontiguousarray(np.asarray(ranks, dtype=np.uint32).reshape(nseg, -1))
    R = ranks.shape[1]
    ks = x.dtype.itemsize
    u = UINT[x.dtype]
    k_in = dev(t, x)
    o = dev(t, np.asarray(off, dtype=np.uint64))
    r_in = dev(t, ranks.view(np.int32))
    g = GUARD + out_shift
    body_k = np.full(nseg * R * ks, KEY_FILL, dtype=np.uint8)
    body_i = np.full(nseg * R * 4, KEY_FILL, dtype=np.uint8)
    k_buf = dev(t, np.concatenate([np.full(g, 0x5A, dtype=np.uint8), body_k, np.full(GUARD * ks, 0xA5, dtype=np.uint8)]))
    i_buf = dev(t, np.concatenate([np.full(g, 0x5A, dtype=np.uint8), body_i, np.full(GUARD * 4, 0xA5, dtype=np.uint8)]))
    if eng is None:
        eng = rsx.Engine(x.dtype, max(n, 1), descending=descending)
    eng.segmented_select(k_in.data_ptr(), n, o.data_ptr(), nseg, r_in.data_ptr(), R, k_buf.data_ptr() + g, i_buf.data_ptr() + g)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    kb = k_buf.cpu().numpy().view(np.uint8)
    ib = i_buf.cpu().numpy().view(np.uint8)
    assert np.all(kb[:g] == 0x5A) and np.all(kb[g + nseg * R * ks:] == 0xA5), "key guard band written"
    assert np.all(ib[:g] == 0x5A) and np.all(ib[g + nseg * R * 4:] == 0xA5), "index guard band written"
    return (kb[g:g + nseg * R * ks].copy().view(u).reshape(nseg, R), ib[g:g + nseg * R * 4].copy().view(np.uint32).reshape(nseg, R), eng)


def check(x, off, ranks, got_k, got_i, descending=False, referee=select_oracle):
    wk, wi, written = referee(x, off, ranks, descending)
    u = UINT[x.dtype]
    fill_k = np.frombuffer(bytes([KEY_FILL]) * np.dtype(u).itemsize, dtype=u)[0]
    bad = np.argwhere(got_k != np.where(written, wk, fill_k))
    assert bad.size == 0, f"keys differ at (segment, slot) {bad[:8].tolist()} (of {len(bad)})"
    bad = np.argwhere(got_i != np.where(written, wi, np.uint32(IDX_FILL)))
    assert bad.size == 0, f"positions differ at (segment, slot) {bad[:8].tolist()} (of {len(bad)})"


LENGTHS = [0, 1, 2, 6, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 1, 0, 3, 9000, 5000, 7, 1,
           1 << 19, 12345]


@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_kinds_directions_ranks(rsx, dtype, descending, R):
    rng = np.random.default_rng(DTYPES.index(dtype) * 16 + descending * 8 + R)
    off = offsets_from(LENGTHS, start=3)
    n = int(off[-1]) + 5
    x = random_bits(dtype, n, rng)
    x[rng.integers(0, n, n // 3)] = x[rng.integers(0, n, n // 3)]           # ties
    ranks = random_ranks(off, R, rng)
    for s, L in enumerate(LENGTHS):                                          # every edge rank at least once per length, in unsorted order
        edge = [L, 0, NONE, max(L - 1, 0), L // 2, 0, max(L - 1, 0), L + 1]
        if s % 2 == 0:
            ranks[s] = edge[:R]
    k, i, _ = run(rsx, x, off, ranks, descending, out_shift=np.dtype(dtype).itemsize if R == 3 else 0)     # R = 3: outputs element-aligned only
    check(x, off, ranks, k, i, descending)


@pytest.mark.parametrize("case", ["few", "all_equal", "heavy"])
@pytest.mark.parametrize("dtype", [np.int32, np.uint64], ids=lambda d: np.dtype(d).name)
def test_ties_first_middle_last(rsx, case, dtype):
    """Ranks at the first, a middle and the last tie of a run: an implementation that returns the first tie of the k-th value fails."""
    rng = np.random.default_rng(31)
    lens = [70000, 4097, 300, 3000, (1 << 18) + 11, 1025]
    off = offsets_from(lens, start=2)
    n = int(off[-1]) + 3
    if case == "few":
        x = rng.integers(0, 3, n).astype(dtype)
    elif case == "all_equal":
        x = np.full(n, 77, dtype=dtype)
    else:
        x = random_bits(dtype, n, rng)
        x[::5] = x[7]                                                        # a heavy value
    for desc in (False, True):
        ranks = np.empty((len(lens), 8), dtype=np.uint32)
        for s, L in enumerate(lens):
            a = int(off[s])
            seg = x[a:a + L]
            vals, counts = np.unique(seg, return_counts=True)
            v = vals[np.argmax(counts)]                                      # the longest run of ties
            c = int(counts.max())
            better = int(np.count_nonzero(seg > v if desc else seg < v))
            ranks[s] = [better, better + c // 2, better + c - 1, better + c - 1, better + 1 if c > 1 else better, L - 1, 0, better + c // 3]
        for R in (8, 3, 1):
            r = np.ascontiguousarray(ranks[:, 1:1 + R])                      # R = 1: the middle tie alone
            k, i, _ = run(rsx, x, off, r, desc)
            check(x, off, r, k, i, desc)
            if case != "heavy" and R == 3:
                assert np.any(i[:, 0] != i[:, 1])                            # middle and last tie are different elements


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_float_specials(rsx, dtype):
    rng = np.random.default_rng(41)
    off = offsets_from([100, 3000, 9000, 1 << 17], start=1)
    x = special(dtype, int(off[-1]), rng)
    for desc in (False, True):
        ranks = random_ranks(off, 8, rng)
        k, i, _ = run(rsx, x, off, ranks, desc)
        check(x, off, ranks, k, i, desc)


@pytest.mark.parametrize("variant", ["window", "low", "straddle"])
@pytest.mark.parametrize("dtype", [np.uint32, np.int64, np.float64], ids=lambda d: np.dtype(d).name)
def test_digit_local_keys(rsx, dtype, variant):
    """Keys that differ only where one select round decides; the large segments cycle through every round (rounds 4..8 of 64-bit keys too)."""
    rng = np.random.default_rng(61)
    lens = [4097 + 1000 * j for j in range(10)] + [300, 2000, 4096, 40000, 9000, 4100]
    off = offsets_from(lens, start=5)
    n = int(off[-1]) + 2
    for desc in (False, True):
        x = _topk_ref.digit_local(dtype, off, n, rng, variant, desc)
        ranks = random_ranks(off, 8, rng)
        k, i, _ = run(rsx, x, off, ranks, desc)
        check(x, off, ranks, k, i, desc)


@pytest.mark.parametrize("dtype", [np.int32, np.uint64, np.float32], ids=lambda d: np.dtype(d).name)
def test_pad_heavy_keys(rsx, dtype):
    rng = np.random.default_rng(67)
    off = offsets_from([5, 200, 1000, 4096, 4097, 30000, 2, 70001], start=0)
    n = int(off[-1])
    for desc in (False, True):
        x = _topk_ref.pad_heavy(dtype, off, n, rng, desc)
        ranks = random_ranks(off, 3, rng)
        k, i, _ = run(rsx, x, off, ranks, desc)
        check(x, off, ranks, k, i, desc)


@pytest.mark.parametrize("shape", list(_topk_ref.SHAPES))
def test_production_shapes(rsx, shape):
    """1024 x 50257 float32, 2048 x 5000 uint64, 64 x 151936 int64, and the ragged rows whose tile groups are shared by two segments."""
    dtype, make = _topk_ref.SHAPES[shape]
    off = make()
    n = _topk_ref.shape_n(off)
    rng = np.random.default_rng(71)
    x = random_bits(dtype, n, rng)
    x[rng.integers(0, n, n // 4)] = x[rng.integers(0, n, n // 4)]
    if shape == "ragged_i32":
        assert _topk_ref.select_geometry(off, n)["switches"] > 0            # groups of tiles that two segments share
    desc = shape.endswith("u64")
    R = 8 if shape == "ragged_i32" else 2
    ranks = random_ranks(off, R, rng)
    ranks[:, 0] = (np.diff(np.asarray(off, dtype=np.int64)) - 1).clip(0) // 2      # the median of every row
    k, i, _ = run(rsx, x, off, ranks, desc)
    check(x, off, ranks, k, i, desc, referee=fast_select)


def test_one_segment_2p24_rank_2p23(rsx):
    """A rank far above the top-k's 4096."""
    rng = np.random.default_rng(24)
    n = 1 << 24
    x = random_bits(np.uint32, n, rng)
    x[::3] = x[5]
    off = np.array([0, n], dtype=np.uint64)
    ranks = np.array([[1 << 23, n - 1, 0, 4097, n, (1 << 23) + 1, 123456, NONE]], dtype=np.uint32)
    k, i, eng = run(rsx, x, off, ranks)
    check(x, off, ranks, k, i, referee=fast_select)
    k1, i1, _ = run(rsx, x, off, ranks[:, :1], eng=eng)
    check(x, off, ranks[:, :1], k1, i1, referee=fast_select)
    k2, i2, _ = run(rsx, x, off, ranks, eng=eng)                             # bitwise the same from run to run
    assert k.tobytes() == k2.tobytes() and i.tobytes() == i2.tobytes()


@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_reported_once(rsx, bad):
    rng = np.random.default_rng(43)
    n = 60000
    x = random_bits(np.uint32, n, rng)
    if bad == "decreasing":
        off = np.array([0, 100, 20000, 5000], dtype=np.uint64)                # segment 2 = [20000, 5000)
    else:
        off = np.array([0, 100, 20000, n + 1], dtype=np.uint64)               # segment 2 ends past n
    ranks = np.array([[0, 50], [10000, 0], [0, 1]], dtype=np.uint32)
    eng = rsx.Engine(np.uint32, n)
    k, i, _ = run(rsx, x, off, ranks, eng=eng)                               # guard bands checked inside
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "segment 2 " in str(ei.value)
    eng.sync()                                                               # reported once
    check(x, off, ranks, k, i)                                               # the bad row keeps the sentinel
    good = np.array([0, 3, 5000, 5001, 30000, n], dtype=np.uint64)
    ranks = random_ranks(good, 2, rng)
    k, i, _ = run(rsx, x, good, ranks, eng=eng)
    eng.sync()
    check(x, good, ranks, k, i)


def test_refusals(rsx):
    t = _torch()
    n = 1 << 14
    eng = rsx.Engine(np.uint32, n)
    x = t.zeros(n, dtype=t.int32, device="cuda")
    off = t.tensor([0, n], dtype=t.int64, device="cuda")
    ranks = t.zeros(16, dtype=t.int32, device="cuda")
    out = t.full((16,), 7, dtype=t.int32, device="cuda")
    idx = t.full((16,), 7, dtype=t.int32, device="cuda")
    with pytest.raises(rsx.RadixSortError) as ei:                            # R = 9
        eng.segmented_select(x.data_ptr(), n, off.data_ptr(), 1, ranks.data_ptr(), 9, out.data_ptr(), idx.data_ptr())
    assert ei.value.status == 4 and "sort" in str(ei.value)
    eng.segmented_select(x.data_ptr(), n, off.data_ptr(), 1, ranks.data_ptr(), 0, out.data_ptr(), idx.data_ptr())     # R == 0: nothing
    eng.segmented_select(x.data_ptr(), n, off.data_ptr(), 0, ranks.data_ptr(), 4, out.data_ptr(), idx.data_ptr())     # no segments: nothing
    with pytest.raises(rsx.RadixSortError) as ei:                            # output overlaps the input
        eng.segmented_select(x.data_ptr(), n, off.data_ptr(), 1, ranks.data_ptr(), 8, x.data_ptr() + 64, idx.data_ptr())
    assert ei.value.status == 1
    with pytest.raises(rsx.RadixSortError):                                  # output overlaps the ranks
        eng.segmented_select(x.data_ptr(), n, off.data_ptr(), 1, ranks.data_ptr(), 8, out.data_ptr(), ranks.data_ptr() + 16)
    with pytest.raises(rsx.RadixSortError):                                  # the two outputs overlap
        eng.segmented_select(x.data_ptr(), n, off.data_ptr(), 1, ranks.data_ptr(), 8, out.data_ptr(), out.data_ptr() + 16)
    with pytest.raises(rsx.RadixSortError):                                  # misaligned keys
        eng.segmented_select(x.data_ptr() + 4, 100, off.data_ptr(), 1, ranks.data_ptr(), 8, out.data_ptr(), idx.data_ptr())
    with pytest.raises(rsx.RadixSortError):                                  # misaligned ranks
        eng.segmented_select(x.data_ptr(), n, off.data_ptr(), 1, ranks.data_ptr() + 2, 8, out.data_ptr(), idx.data_ptr())
    with pytest.raises(rsx.RadixSortError) as ei:                            # beyond capacity
        eng.segmented_select(x.data_ptr(), n + 1, off.data_ptr(), 1, ranks.data_ptr(), 8, out.data_ptr(), idx.data_ptr())
    assert ei.value.status == 7
    eng.sync()
    assert bool((out == 7).all()) and bool((idx == 7).all())                # nothing was written by any of them


@pytest.mark.parametrize("dtype", ["int32", "int64", "float32", "float64"])
def test_kthvalue_median_match_torch(rsx, dtype):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(5)
    for shape, kk in (((64, 1 << 17), 1 << 16), ((4096, 300), 32), ((3, 20000), 4097), ((7,), 3), ((5, 1), 1)):
        if dtype.startswith("float"):
            x = t.randn(shape, device="cuda", generator=g, dtype=getattr(t, dtype))
            x.view(-1)[::11] = 0.5                                           # ties
            x.view(-1)[::97] = float("inf")
        else:
            x = t.randint(-50, 50, shape, device="cuda", generator=g, dtype=getattr(t, dtype))
        sv, si = t.sort(x, dim=-1, stable=True)
        v, i = rsx.kthvalue(x, kk)
        wv, _ = t.kthvalue(x, kk)
        assert i.dtype == t.int64 and v.shape == wv.shape and i.shape == wv.shape
        assert t.equal(v, wv) and t.equal(x.gather(-1, i.unsqueeze(-1)).squeeze(-1), v) and t.equal(i, si[..., kk - 1])
        v, i = rsx.median(x)
        wv, _ = t.median(x, dim=-1)
        mid = (x.shape[-1] - 1) // 2
        assert v.shape == wv.shape and t.equal(v, wv) and t.equal(x.gather(-1, i.unsqueeze(-1)).squeeze(-1), v) and t.equal(i, si[..., mid])
    # +NaN is the largest key, as torch.kthvalue ranks it
    y = t.tensor([[1.0, float("nan"), -2.0, float("nan"), 0.0]], device="cuda", dtype=getattr(t, dtype) if dtype.startswith("float") else t.float32)
    v, i = rsx.kthvalue(y, 3)
    assert v.item() == 1.0 and i.item() == 0
    v, i = rsx.kthvalue(y, 5)
    assert t.isnan(v).item() and i.item() == 3 and t.isnan(t.kthvalue(y, 5)[0]).item()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("mode", ["linear", "lower", "higher", "midpoint", "nearest"])
def test_quantile_matches_torch(rsx, dtype, mode):
    t = _torch()
    dt = getattr(t, dtype)
    g = t.Generator(device="cuda").manual_seed(9)
    qs = [0.0, 0.1, 0.25, 1 / 3, 0.5, 0.77, 0.999, 1.0, 0.5]                 # 9 quantiles: up to 18 ranks, three engine calls
    for shape in ((16, 50257), (300, 1001), (2, 6), (4, 1)):
        x = t.randn(shape, device="cuda", generator=g, dtype=dt)
        x.view(-1)[::7] = 0.25
        got = rsx.quantile(x, qs, interpolation=mode)
        want = t.quantile(x, t.tensor(qs, device="cuda", dtype=dt), dim=-1, interpolation=mode)
        assert got.shape == want.shape and t.equal(got, want), (shape, mode)
        got = rsx.quantile(x, t.tensor(qs[:4], device="cuda", dtype=dt), dim=0, keepdim=True, interpolation=mode)      # q on the device: not read back
        want = t.quantile(x, t.tensor(qs[:4], device="cuda", dtype=dt), dim=0, keepdim=True, interpolation=mode)
        assert got.shape == want.shape and t.equal(got, want)
        got = rsx.quantile(x, 0.3, interpolation=mode)
        want = t.quantile(x, 0.3, dim=-1, interpolation=mode)
        assert got.shape == want.shape and t.equal(got, want)


def test_dims_layouts_stream(rsx):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(7)
    x = t.randint(-1000, 1000, (5, 3000, 6), device="cuda", generator=g, dtype=t.int32)
    for dim in (0, 1, -1):
        for keep in (False, True):
            sv, si = t.sort(x, dim=dim, stable=True)
            size = x.shape[dim]
            v, i = rsx.kthvalue(x, size // 3 + 1, dim=dim, keepdim=keep)
            wv, _ = t.kthvalue(x, size // 3 + 1, dim=dim, keepdim=keep)
            wi = si.narrow(dim % 3, size // 3, 1)
            assert v.shape == wv.shape and t.equal(v, wv) and t.equal(i, wi if keep else wi.squeeze(dim))
            v, i = rsx.median(x, dim=dim, keepdim=keep)
            wv, _ = t.median(x, dim=dim, keepdim=keep)
            wi = si.narrow(dim % 3, (size - 1) // 2, 1)
            assert v.shape == wv.shape and t.equal(v, wv) and t.equal(i, wi if keep else wi.squeeze(dim))
            xf = x.double()
            for q in (0.4, [0.1, 0.9]):
                got = rsx.quantile(xf, q, dim=dim, keepdim=keep)
                want = t.quantile(xf, t.tensor(q, device="cuda", dtype=t.float64), dim=dim, keepdim=keep)
                assert got.shape == want.shape and t.equal(got, want)
    xt = x[:, :, 2].t()                                                      # non-contiguous
    v, i = rsx.median(xt)
    sv, si = t.sort(xt, dim=-1, stable=True)
    assert t.equal(v, t.median(xt, dim=-1)[0]) and t.equal(i, si[:, 2])
    xs = x[:, ::2, 1]                                                        # strided rows of 1500
    v, i = rsx.kthvalue(xs, 1500)
    assert t.equal(v, xs.max(dim=-1)[0]) and t.equal(xs.gather(-1, i.unsqueeze(-1)).squeeze(-1), v)
    z = t.tensor(4.5, device="cuda")                                         # 0-d
    v, i = rsx.kthvalue(z, 1)
    assert v.shape == () and v.item() == 4.5 and i.item() == 0
    assert rsx.median(z)[0].item() == 4.5 and rsx.quantile(z, 0.5).item() == 4.5 and rsx.quantile(z, 0.5).shape == t.quantile(z, 0.5).shape
    with pytest.raises(ValueError):
        rsx.kthvalue(x, 7)                                                   # k > size
    with pytest.raises(ValueError):
        rsx.quantile(x.float(), 1.5)
    for bad in (t.float16, t.bfloat16, t.bool):
        for fn in (lambda y: rsx.kthvalue(y, 2), rsx.median, lambda y: rsx.quantile(y, 0.5)):
            with pytest.raises(TypeError):
                fn(t.zeros(10, dtype=bad, device="cuda"))
    with pytest.raises(TypeError):
        rsx.quantile(x, 0.5)                                                 # integers have no quantile, as in torch
    # work runs on the current torch stream: an engine of that stream, the result ordered after work queued there
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        y = x.float() * 2
        v2, _ = rsx.median(y, dim=1)
    side.synchronize()
    assert t.equal(v2, t.median(x.float() * 2, dim=1)[0])
    assert side.cuda_stream in {key[1] for key in rsx._SEG_ENGINES}


def test_segmented_select_helper(rsx):
    t = _torch()
    rng = np.random.default_rng(53)
    x = random_bits(np.float32, 30001, rng)
    off = offsets_from([100, 0, 1, 7000, 3000, 5], start=1)
    keys = t.from_numpy(x).cuda()[1:]                                        # misaligned view: copied first
    offsets = t.from_numpy(off.astype(np.int64)).cuda()
    xs = x[1:]
    for R in (1, 8, 19):                                                     # 19: three engine calls
        ranks = random_ranks(off, R, rng)
        r64 = ranks.astype(np.int64)
        r64[r64 == NONE] = -1                                                # negative: selects nothing
        for desc in (False, True):
            v, i = rsx.segmented_select(keys, offsets, t.from_numpy(r64).cuda(), descending=desc)
            wk, wi, written = select_oracle(xs, off, ranks, desc)
            assert v.shape == (6, R) and i.dtype == t.int64
            assert np.array_equal(v.cpu().numpy().view(np.uint32), np.where(written, wk, 0))
            assert np.array_equal(i.cpu().numpy(), np.where(written, wi.astype(np.int64), -1))
    v, i = rsx.segmented_select(keys, offsets, t.tensor([3, 0, 0, 6999, 2999, 9], device="cuda", dtype=t.int32))      # ranks [S]
    wk, wi, written = select_oracle(xs, off, np.array([3, 0, 0, 6999, 2999, 9], dtype=np.uint32))
    assert v.shape == (6, 1) and np.array_equal(i.cpu().numpy(), np.where(written, wi.astype(np.int64), -1))


def test_one_engine_growing_shapes_interleaved(rsx):
    """One engine: select on growing shapes and growing R between segmented sorts and top-ks (they share scratch buffers)."""
    import test_gpu_segmented as seg
    import test_gpu_topk as topk
    rng = np.random.default_rng(59)
    eng = rsx.Engine(np.uint32, 1 << 22)
    for step, (lens, R) in enumerate([([5000, 100], 1), ([70000, 4097, 3], 8), ([1 << 20, 9000, 9000, 1], 3), ([1 << 22], 8), ([4097] * 200, 8)]):
        off = offsets_from(lens, start=0)
        x = random_bits(np.uint32, int(off[-1]), rng)
        x[::4] = x[1]
        ranks = random_ranks(off, R, rng)
        k, i, _ = run(rsx, x, off, ranks, eng=eng)
        check(x, off, ranks, k, i)
        if step % 2 == 0:
            tk, ti, _ = topk.run(rsx, x, off, 100, eng=eng)
            topk.check(x, off, 100, tk, ti)
        else:
            sk, sp, _ = seg.run(rsx, x, off, payload=False, eng=eng)
            seg.check(x, off, sk, sp, False, payload=False)
        k, i, _ = run(rsx, x, off, ranks, eng=eng)
        check(x, off, ranks, k, i)
    eng.sync()


def test_graph_capture_and_replay(rsx):
    """A warmed call is captured into a graph; the replay reads new keys, offsets and ranks from the same buffers."""
    t = _torch()
    rng = np.random.default_rng(73)
    n, nseg, R = 300000, 6, 8
    stream = t.cuda.Stream()
    eng = rsx.Engine(np.int64, n)
    eng.set_stream(stream.cuda_stream)
    keys = t.zeros(n, dtype=t.int64, device="cuda")
    offs = t.zeros(nseg + 1, dtype=t.int64, device="cuda")
    ranks = t.zeros((nseg, R), dtype=t.int32, device="cuda")
    out = t.zeros((nseg, R), dtype=t.int64, device="cuda")
    idx = t.zeros((nseg, R), dtype=t.int32, device="cuda")

    def load(lens):
        off = offsets_from(lens, start=0)
        x = random_bits(np.int64, n, rng)
        x[::3] = x[0]
        r = random_ranks(off, R, rng)
        keys.copy_(t.from_numpy(x))
        offs.copy_(t.from_numpy(off.astype(np.int64)))
        ranks.copy_(t.from_numpy(r.view(np.int32)))
        out.fill_(-7)
        idx.fill_(-7)
        t.cuda.synchronize()
        return x, off, r

    def call():
        eng.segmented_select(keys.data_ptr(), n, offs.data_ptr(), nseg, ranks.data_ptr(), R, out.data_ptr(), idx.data_ptr())

    def verify(x, off, r):
        wk, wi, written = select_oracle(x, off, r)
        assert np.array_equal(out.cpu().numpy().view(np.uint64), np.where(written, wk, np.uint64(np.int64(-7).astype(np.uint64))))
        assert np.array_equal(idx.cpu().numpy().view(np.uint32), np.where(written, wi, np.uint32(0xFFFFFFF9)))

    first = load([100000, 5000, 1, 0, 150000, 300])
    call()                                                                   # warm-up: scratch grows here
    stream.synchronize()
    verify(*first)
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=stream):
        call()
    second = load([4097, 200000, 2, 90000, 0, 5000])
    graph.replay()
    t.cuda.synchronize()
    verify(*second)
    third = load([0, 0, 299000, 1, 1, 998])
    graph.replay()
    t.cuda.synchronize()
    verify(*third)
    eng.sync()
