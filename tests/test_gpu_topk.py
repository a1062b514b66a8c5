"""Segmented top-k (rsx_segmented_topk, radix_sort_amd.segmented_topk / topk) on the GPU.

The oracle is the first min(k, L) entries of every valid segment's stable argsort (seg_oracle of tests/test_gpu_segmented.py, itself
np.lexsort over the engine's key encoding), compared bit for bit: keys AND positions.  The outputs start out holding a sentinel that
must survive in every slot the call may not write (slots past min(k, L), rows of invalid segments), and sit inside guard bands that
must come back untouched.  Lengths reach every path: one-key segments, the three LDS classes (<= 256, <= 1024, <= 4096 keys) and the
select chain over the tiles of larger segments.
"""
import numpy as np
import pytest

from test_gpu_float_keys import UINT, random_bits, special
from test_gpu_segmented import DTYPES, _torch, dev, offsets_from, seg_oracle

pytestmark = pytest.mark.gpu

GUARD = 64
KEY_FILL, IDX_FILL = 0xC3, 0xC3C3C3C3


def topk_oracle(x: np.ndarray, off: np.ndarray, k: int, descending: bool = False):
    """(keys [S, k] as unsigned words, positions [S, k] uint32, written [S, k] bool): the first min(k, L) entries of the stable sort of
    every valid segment; `written` marks the slots the call writes (everything else keeps the caller's contents)."""
    n = x.size
    off = np.asarray(off, dtype=np.int64)
    nseg = len(off) - 1
    u = UINT[x.dtype]
    want = seg_oracle(x, off, n, descending)
    keys = np.zeros((nseg, k), dtype=u)
    pos = np.zeros((nseg, k), dtype=np.uint32)
    written = np.zeros((nseg, k), dtype=bool)
    for s in range(nseg):
        a, b = int(off[s]), int(off[s + 1])
        if not (a <= b <= n):
            continue
        m = min(k, b - a)
        src = want[a:a + m]
        keys[s, :m] = x[src].view(u)
        pos[s, :m] = (src - a).astype(np.uint32)
        written[s, :m] = True
    return keys, pos, written


def run(rsx, x, off, k, descending=False, eng=None, out_shift=0):
    """One rsx_segmented_topk through the Engine API, outputs inside guard bands and pre-filled with the sentinel.
    Returns (keys [S, k] unsigned words, positions [S, k] uint32, engine)."""
    t = _torch()
    n = x.size
    nseg = len(off) - 1
    ks = x.dtype.itemsize
    u = UINT[x.dtype]
    k_in = dev(t, x)
    o = dev(t, np.asarray(off, dtype=np.uint64))
    g = GUARD + out_shift
    body_k = np.full(nseg * k * ks, KEY_FILL, dtype=np.uint8)
    body_i = np.full(nseg * k * 4, KEY_FILL, dtype=np.uint8)
    k_buf = dev(t, np.concatenate([np.full(g, 0x5A, dtype=np.uint8), body_k, np.full(GUARD * ks, 0xA5, dtype=np.uint8)]))
    i_buf = dev(t, np.concatenate([np.full(g, 0x5A, dtype=np.uint8), body_i, np.full(GUARD * 4, 0xA5, dtype=np.uint8)]))
    if eng is None:
        eng = rsx.Engine(x.dtype, max(n, 1), descending=descending)
    eng.segmented_topk(k_in.data_ptr(), n, o.data_ptr(), nseg, k, k_buf.data_ptr() + g, i_buf.data_ptr() + g)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    kb = k_buf.cpu().numpy().view(np.uint8)
    ib = i_buf.cpu().numpy().view(np.uint8)
    assert np.all(kb[:g] == 0x5A) and np.all(kb[g + nseg * k * ks:] == 0xA5), "key guard band written"
    assert np.all(ib[:g] == 0x5A) and np.all(ib[g + nseg * k * 4:] == 0xA5), "index guard band written"
    return (kb[g:g + nseg * k * ks].copy().view(u).reshape(nseg, k), ib[g:g + nseg * k * 4].copy().view(np.uint32).reshape(nseg, k), eng)


def check(x, off, k, got_k, got_i, descending=False):
    wk, wi, written = topk_oracle(x, off, k, descending)
    u = UINT[x.dtype]
    fill_k = np.frombuffer(bytes([KEY_FILL]) * np.dtype(u).itemsize, dtype=u)[0]
    bad = np.argwhere(got_k != np.where(written, wk, fill_k))
    assert bad.size == 0, f"keys differ at (segment, slot) {bad[:8].tolist()} (of {len(bad)})"
    bad = np.argwhere(got_i != np.where(written, wi, np.uint32(IDX_FILL)))
    assert bad.size == 0, f"positions differ at (segment, slot) {bad[:8].tolist()} (of {len(bad)})"


LENGTHS = [0, 1, 2, 6, 7, 8, 63, 64, 65, 255, 256, 257, 999, 1000, 1001, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 1, 0, 3,
           5000, 7, 1, 1 << 20, 12345]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_kinds_directions(rsx, dtype, descending):
    rng = np.random.default_rng(DTYPES.index(dtype) * 2 + descending)
    off = offsets_from(LENGTHS, start=3)
    n = int(off[-1]) + 5
    x = random_bits(dtype, n, rng)
    x[rng.integers(0, n, n // 3)] = x[rng.integers(0, n, n // 3)]           # ties
    k, i, _ = run(rsx, x, off, 1000, descending)
    check(x, off, 1000, k, i, descending)


@pytest.mark.parametrize("kk", [1, 7, 64, 1000, 4096])
@pytest.mark.parametrize("dtype", [np.uint32, np.float64], ids=lambda d: np.dtype(d).name)
def test_every_k(rsx, kk, dtype):
    rng = np.random.default_rng(kk)
    off = offsets_from(LENGTHS, start=1)
    x = random_bits(dtype, int(off[-1]), rng)
    x[::5] = x[7]                                                            # a heavy value
    desc = dtype == np.float64
    k, i, _ = run(rsx, x, off, kk, desc, out_shift=np.dtype(dtype).itemsize)     # outputs element-aligned only
    check(x, off, kk, k, i, desc)


def test_k_above_one_tile_refused(rsx):
    t = _torch()
    eng = rsx.Engine(np.uint32, 1 << 14)
    x = t.zeros(1 << 14, dtype=t.int32, device="cuda")
    off = t.tensor([0, 1 << 14], dtype=t.int64, device="cuda")
    out = t.zeros(4097, dtype=t.int32, device="cuda")
    idx = t.zeros(4097, dtype=t.int32, device="cuda")
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.segmented_topk(x.data_ptr(), 1 << 14, off.data_ptr(), 1, 4097, out.data_ptr(), idx.data_ptr())
    assert ei.value.status == 4 and "sort" in str(ei.value)
    eng.segmented_topk(x.data_ptr(), 1 << 14, off.data_ptr(), 1, 0, out.data_ptr(), idx.data_ptr())     # k == 0: nothing
    with pytest.raises(rsx.RadixSortError):                                  # output overlaps the input
        eng.segmented_topk(x.data_ptr(), 1 << 14, off.data_ptr(), 1, 16, x.data_ptr() + 64, idx.data_ptr())
    with pytest.raises(rsx.RadixSortError):                                  # misaligned input
        eng.segmented_topk(x.data_ptr() + 4, 100, off.data_ptr(), 1, 16, out.data_ptr(), idx.data_ptr())
    with pytest.raises(rsx.RadixSortError):                                  # beyond capacity
        eng.segmented_topk(x.data_ptr(), (1 << 14) + 1, off.data_ptr(), 1, 16, out.data_ptr(), idx.data_ptr())
    # the Python fallback for k > 4096 is still torch.topk's answer
    y = t.randint(-1000, 1000, (3, 9000), device="cuda", dtype=t.int32)
    v, i = rsx.topk(y, 4097)
    wv, wi = t.sort(y, dim=-1, descending=True, stable=True)
    assert t.equal(v, wv[:, :4097]) and t.equal(i, wi[:, :4097])


def test_one_segment_2p26(rsx):
    rng = np.random.default_rng(26)
    n = 1 << 26
    x = random_bits(np.uint32, n, rng)
    off = np.array([0, n], dtype=np.uint64)
    k, i, _ = run(rsx, x, off, 1000)
    check(x, off, 1000, k, i)
    k, i, _ = run(rsx, x, off, 4096, True)
    check(x, off, 4096, k, i, True)


@pytest.mark.parametrize("case", ["all_equal", "few_values", "straddle", "sorted", "reversed"])
def test_ties_and_orders(rsx, case):
    rng = np.random.default_rng(31)
    lens = [70000, 4097, 300, 3000, (1 << 18) + 11]
    off = offsets_from(lens, start=2)
    n = int(off[-1]) + 3
    if case == "all_equal":
        x = np.full(n, 77, dtype=np.int32)
    elif case == "few_values":
        x = rng.integers(0, 4, n).astype(np.int32)
    elif case == "straddle":
        # in every segment: a run of the k-th value spread over several tiles, with better keys before and after it
        x = rng.integers(1000, 2000, n).astype(np.int32)
        for a, b in zip(off[:-1], off[1:]):
            a, b = int(a), int(b)
            L = b - a
            x[a + rng.integers(0, L, min(L, 600))] = rng.integers(0, 500, min(L, 600))      # better (ascending)
            x[a + np.arange(L // 7, L, 3)[:3000]] = 700                                      # the tie run
    elif case == "sorted":
        x = np.sort(rng.integers(-1 << 30, 1 << 30, n)).astype(np.int32)
    else:
        x = np.sort(rng.integers(-1 << 30, 1 << 30, n))[::-1].astype(np.int32).copy()
    for kk, desc in ((1000, False), (4096, True), (7, False)):
        k, i, _ = run(rsx, x, off, kk, desc)
        check(x, off, kk, k, i, desc)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_float_specials(rsx, dtype):
    rng = np.random.default_rng(41)
    off = offsets_from([100, 3000, 9000, 1 << 17], start=1)
    x = special(dtype, int(off[-1]), rng)
    for desc in (False, True):
        k, i, _ = run(rsx, x, off, 1000, desc)
        check(x, off, 1000, k, i, desc)


@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_reported_once(rsx, bad):
    rng = np.random.default_rng(43)
    n = 60000
    x = random_bits(np.uint32, n, rng)
    if bad == "decreasing":
        off = np.array([0, 100, 20000, 5000], dtype=np.uint64)                # segment 2 = [20000, 5000)
    else:
        off = np.array([0, 100, 20000, n + 1], dtype=np.uint64)               # segment 2 ends past n
    eng = rsx.Engine(np.uint32, n)
    k, i, _ = run(rsx, x, off, 64, eng=eng)                                  # guard bands checked inside
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "segment 2 " in str(ei.value)
    eng.sync()                                                               # reported once
    check(x, off, 64, k, i)                                                  # the bad row keeps the sentinel
    good = np.array([0, 3, 5000, 5001, 30000, n], dtype=np.uint64)
    k, i, _ = run(rsx, x, good, 64, eng=eng)
    eng.sync()
    check(x, good, 64, k, i)


def test_deterministic(rsx):
    rng = np.random.default_rng(47)
    off = offsets_from([1 << 21, 5000, 200, 1 << 19], start=0)
    x = rng.integers(0, 50, int(off[-1])).astype(np.uint64)                  # many ties
    eng = rsx.Engine(np.uint64, x.size, descending=True)
    k1, i1, _ = run(rsx, x, off, 1000, eng=eng)
    k2, i2, _ = run(rsx, x, off, 1000, eng=eng)
    assert k1.tobytes() == k2.tobytes() and i1.tobytes() == i2.tobytes()
    check(x, off, 1000, k1, i1, True)


@pytest.mark.parametrize("dtype", ["int32", "int64", "float32", "float64"])
@pytest.mark.parametrize("largest", [True, False], ids=["largest", "smallest"])
def test_topk_matches_torch(rsx, dtype, largest):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(5)
    for shape, kk in (((64, 1 << 17), 50), ((4096, 300), 32), ((3, 20000), 4096), ((7,), 3)):
        if dtype.startswith("float"):
            x = t.randn(shape, device="cuda", generator=g, dtype=getattr(t, dtype))
            x.view(-1)[::11] = 0.5                                           # ties
            x.view(-1)[::97] = float("inf")
            x.view(-1)[5::101] = float("nan")
        else:
            x = t.randint(-50, 50, shape, device="cuda", generator=g, dtype=getattr(t, dtype))
        v, i = rsx.topk(x, kk, largest=largest)
        wv, _ = t.topk(x, kk, largest=largest)
        _, si = t.sort(x, dim=-1, descending=largest, stable=True)
        assert i.dtype == t.int64 and v.shape == wv.shape and i.shape == wv.shape
        assert t.equal(v.nan_to_num(), wv.nan_to_num()) and t.equal(v.isnan(), wv.isnan())
        assert t.equal(i, si[..., :kk])


def test_topk_dims_layouts_stream(rsx):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(7)
    x = t.randint(-1000, 1000, (5, 3000, 6), device="cuda", generator=g, dtype=t.int32)
    for dim in (0, 1, -1):
        v, i = rsx.topk(x, 4, dim=dim, sorted=False)
        _, si = t.sort(x, dim=dim, descending=True, stable=True)
        wv, _ = t.topk(x, 4, dim=dim)
        assert t.equal(v, wv) and t.equal(i, si.narrow(dim % 3, 0, 4))
    xt = x[:, :, 2].t()                                                      # non-contiguous
    v, i = rsx.topk(xt, 3, largest=False)
    _, si = t.sort(xt, dim=-1, stable=True)
    assert t.equal(v, t.topk(xt, 3, largest=False)[0]) and t.equal(i, si[:, :3])
    xs = x[:, ::2, 1]                                                        # strided rows of 1500
    v, i = rsx.topk(xs, 100)
    _, si = t.sort(xs, dim=-1, descending=True, stable=True)
    assert t.equal(v, t.topk(xs, 100)[0]) and t.equal(i, si[:, :100])
    v, i = rsx.topk(x, 0)
    assert v.shape == (5, 3000, 0) and i.shape == (5, 3000, 0)
    with pytest.raises(ValueError):
        rsx.topk(x, 7)                                                       # k > size
    for bad in (t.float16, t.bfloat16, t.bool):
        with pytest.raises(TypeError):
            rsx.topk(t.zeros(10, dtype=bad, device="cuda"), 2)
    # work runs on the current torch stream: an engine of that stream, the result ordered after work queued there
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        y = x.float() * 2
        v2, i2 = rsx.topk(y, 5)
    side.synchronize()
    assert t.equal(v2, t.topk(x.float() * 2, 5)[0])
    assert side.cuda_stream in {key[1] for key in rsx._SEG_ENGINES}


def test_segmented_topk_helper(rsx):
    t = _torch()
    rng = np.random.default_rng(53)
    x = random_bits(np.float32, 30001, rng)
    x = x[np.isfinite(x)]
    off = offsets_from([100, 0, 1, 7000, 3000, 5], start=1)
    keys = t.from_numpy(x).cuda()[1:]                                        # misaligned view: copied first
    offsets = t.from_numpy(off.astype(np.int64)).cuda()
    v, i = rsx.segmented_topk(keys, offsets, 50, largest=True)
    xs = x[1:]
    wk, wi, written = topk_oracle(xs, off, 50, descending=True)
    assert v.shape == (6, 50) and i.dtype == t.int64
    assert np.array_equal(v.cpu().numpy().view(np.uint32), np.where(written, wk, 0))
    assert np.array_equal(i.cpu().numpy(), np.where(written, wi.astype(np.int64), -1))
