"""Weighted select (rsx_segmented_weighted_select, radix_sort_amd.segmented_weighted_select / top_p / weighted_quantile / weighted_median)
on the GPU.

The referee is tests/_wselect_ref.py: the stable argsort of the order-mapped keys, the mass function in numpy, a uint64 cumsum and
searchsorted, compared bit for bit: keys, positions, ranks, masses and totals.  The outputs start out holding a sentinel that must
survive in every slot the call may not write (targets without an answer, rows of invalid segments) and sit inside guard bands that must
come back untouched.  Lengths reach every path: empty and one-key segments, the three LDS classes (<= 256, <= 1024, <= 4096 keys) and
the select chain over the tiles of larger segments.  Every layout here runs the chain with one tile per group and at most one item per
workgroup in every kernel; groups shared by several large segments, the grid strides and segments of more than 1024 tiles are the
business of tests/test_gpu_wselect_paths.py.
"""
import numpy as np
import pytest

from _wselect_ref import MASS_ONE, kind_of, mass_np, random_targets, wselect_oracle
from test_gpu_float_keys import UINT, random_bits, special
from test_gpu_segmented import DTYPES, _torch, dev, offsets_from

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xC3
LENGTHS = [0, 1, 2, 6, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 1, 0, 3, 9000, 5000, 7, 1,
           1 << 19, 12345]


def _band(t, nbytes, elem, shift):
    g = GUARD + shift
    buf = dev(t, np.concatenate([np.full(g, 0x5A, dtype=np.uint8), np.full(nbytes, FILL, dtype=np.uint8), np.full(GUARD * elem, 0xA5, dtype=np.uint8)]))
    return buf, g


def _unband(buf, g, nbytes, what):
    b = buf.cpu().numpy().view(np.uint8)
    assert np.all(b[:g] == 0x5A) and np.all(b[g + nbytes:] == 0xA5), f"{what} guard band written"
    return b[g:g + nbytes].copy()


def run(rsx, x, off, weights, targets, fraction=False, descending=False, weight_exp=0, eng=None, out_shift=0):
    """One rsx_segmented_weighted_select through the Engine API, outputs inside guard bands and pre-filled with the sentinel.
    Returns (keys [S, R] unsigned words, pos [S, R] uint32, rank [S, R] uint32, mass [S, R] uint64, total [S] uint64, engine)."""
    t = _torch()
    n = x.size
    nseg = len(off) - 1
    tt = np.ascontiguousarray(np.asarray(targets, dtype=np.float64 if fraction else np.uint64).reshape(nseg, -1))
    R = tt.shape[1]
    ks = x.dtype.itemsize
    u = UINT[x.dtype]
    k_in = dev(t, x)
    w_in = None if weights is None else dev(t, weights)
    o = dev(t, np.asarray(off, dtype=np.uint64))
    t_in = dev(t, tt)
    kind = kind_of(x if weights is None else weights)
    k_buf, gk = _band(t, nseg * R * ks, ks, out_shift * ks)
    i_buf, gi = _band(t, nseg * R * 4, 4, out_shift * 4)
    r_buf, gr = _band(t, nseg * R * 4, 4, out_shift * 4)
    m_buf, gm = _band(t, nseg * R * 8, 8, out_shift * 8)
    s_buf, gs = _band(t, nseg * 8, 8, out_shift * 8)
    if eng is None:
        eng = rsx.Engine(x.dtype, max(n, 1), descending=descending)
    eng.segmented_weighted_select(k_in.data_ptr(), None if w_in is None else w_in.data_ptr(), n, o.data_ptr(), nseg, t_in.data_ptr(), R,
                                  rsx.WSELECT_FRACTION if fraction else 0, kind, weight_exp, k_buf.data_ptr() + gk, i_buf.data_ptr() + gi,
                                  r_buf.data_ptr() + gr, m_buf.data_ptr() + gm, s_buf.data_ptr() + gs)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    return (_unband(k_buf, gk, nseg * R * ks, "key").view(u).reshape(nseg, R), _unband(i_buf, gi, nseg * R * 4, "index").view(np.uint32).reshape(nseg, R),
            _unband(r_buf, gr, nseg * R * 4, "rank").view(np.uint32).reshape(nseg, R), _unband(m_buf, gm, nseg * R * 8, "mass").view(np.uint64).reshape(nseg, R),
            _unband(s_buf, gs, nseg * 8, "total").view(np.uint64), eng)


def _fill(dtype):
    return np.frombuffer(bytes([FILL]) * np.dtype(dtype).itemsize, dtype=dtype)[0]


def check(got, x, off, weights, targets, fraction=False, descending=False, weight_exp=0):
    wk, wi, wr, wm, written, total, valid = wselect_oracle(x, off, weights, targets, fraction, descending, weight_exp)
    gk, gi, gr, gm, gt = got[:5]
    for name, g, w, mask in (("keys", gk, wk, written), ("positions", gi, wi, written), ("ranks", gr, wr, written), ("masses", gm, wm, written),
                             ("totals", gt, total, valid)):
        bad = np.argwhere(g != np.where(mask, w, _fill(g.dtype)))
        assert bad.size == 0, f"{name} differ at {bad[:8].tolist()} (of {len(bad)}): got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"
    return written


def make_weights(kind, n, rng):
    """Random weights of one kind with the values that weigh nothing mixed in."""
    if kind == 0:
        w = rng.integers(0, 1000, n).astype(np.uint32)
        w[rng.integers(0, n, n // 5)] = 0
        w[rng.integers(0, n, max(n // 50, 1))] = 0xFFFFFFFF
        return w
    w = (rng.random(n) * 1.5).astype(np.float32 if kind == 1 else np.float64)
    w[rng.integers(0, n, n // 7)] = 0.0
    w[rng.integers(0, n, n // 9)] = -0.25
    w[rng.integers(0, n, n // 11)] = np.nan
    w[rng.integers(0, n, max(n // 50, 1))] = 3.0           # above 2^weight_exp: saturates
    return w


def edge_targets(total, R, rng):
    tt = random_targets(total, R, rng)
    for s in range(len(total)):                            # the edge targets of every other segment, in rotating order
        if s % 2 == 0:
            edge = [0, 1, int(total[s]), int(total[s]) + 1]
            tt[s] = [edge[(s // 2 + q) % 4] for q in range(R)]
    return tt


def edge_fractions(nseg, R, rng):
    fr = rng.random((nseg, R))
    edge = [0.0, 1.0, np.nan, 0.5, -1.0, 2.0, 1e-12, 1 - 1e-12]
    for s in range(nseg):
        if s % 2 == 0:
            fr[s] = [edge[(s // 2 + q) % len(edge)] for q in range(R)]
    return fr


def totals_of(x, off, weights, weight_exp=0):
    m = mass_np(x if weights is None else weights, weight_exp)
    return np.array([int(m[int(a):int(b)].sum()) if a <= b <= x.size else 0 for a, b in zip(off[:-1], off[1:])], dtype=np.uint64)


@pytest.mark.parametrize("R", [1, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_kinds_directions_targets(rsx, dtype, descending, R):
    """All six key types x both directions x R; the weight kind cycles so that every (key width, weight kind) pair occurs; absolute and
    fraction form; for float keys also the keys as their own weights."""
    rng = np.random.default_rng(DTYPES.index(dtype) * 16 + descending * 8 + R)
    off = offsets_from(LENGTHS, start=3)
    n = int(off[-1]) + 5
    x = random_bits(dtype, n, rng)
    x[rng.integers(0, n, n // 3)] = x[rng.integers(0, n, n // 3)]           # ties
    kind = (DTYPES.index(dtype) + R + descending) % 3
    wexp = 0 if kind == 0 else [0, -1, 3][R % 3]
    w = make_weights(kind, n, rng)
    total = totals_of(x, off, w, wexp)
    shift = 1 if R == 3 else 0                                               # R = 3: outputs element-aligned only
    tt = edge_targets(total, R, rng)
    got = run(rsx, x, off, w, tt, False, descending, wexp, out_shift=shift)
    written = check(got, x, off, w, tt, False, descending, wexp)
    assert written.any() and not written.all()
    fr = edge_fractions(len(total), R, rng)
    got = run(rsx, x, off, w, fr, True, descending, wexp, eng=got[5], out_shift=shift)
    check(got, x, off, w, fr, True, descending, wexp)
    if np.dtype(dtype).kind == "f":                                          # the keys are the weights
        p = np.ldexp(rng.random(n), -rng.integers(0, 20, n)).astype(dtype)
        p[rng.integers(0, n, n // 4)] = p[rng.integers(0, n, n // 4)]
        p[rng.integers(0, n, n // 10)] = 0.0
        p[rng.integers(0, n, n // 100)] = -p[rng.integers(0, n, n // 100)]
        p[rng.integers(0, n, 50)] = np.nan
        got = run(rsx, p, off, None, fr, True, descending, 0, eng=got[5])
        check(got, p, off, None, fr, True, descending, 0)
        tt = edge_targets(totals_of(p, off, None), R, rng)
        got = run(rsx, p, off, None, tt, False, descending, 0, eng=got[5])
        check(got, p, off, None, tt, False, descending, 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_every_edge_target_on_every_length(rsx, dtype, descending):
    """Every length of LENGTHS gets every edge target by construction, in one R = 4 call per form: 0, 1, total and total + 1, and the
    fractions 0, 1, NaN and 0.5 — with separate weights of a cycling kind, and for float keys with the keys as their own weights."""
    rng = np.random.default_rng(500 + DTYPES.index(dtype) * 2 + descending)
    off = offsets_from(LENGTHS, start=3)
    n = int(off[-1]) + 5
    nseg = len(LENGTHS)
    x = random_bits(dtype, n, rng)
    x[rng.integers(0, n, n // 3)] = x[rng.integers(0, n, n // 3)]           # ties
    kind = (DTYPES.index(dtype) + descending) % 3
    wexp = 0 if kind == 0 else 1
    cases = [(x, make_weights(kind, n, rng), wexp)]
    if np.dtype(dtype).kind == "f":
        p = np.ldexp(rng.random(n), -rng.integers(0, 20, n)).astype(dtype)
        p[rng.integers(0, n, n // 10)] = 0.0
        cases.append((p, None, 0))
    fr = np.tile(np.array([0.0, 1.0, np.nan, 0.5]), (nseg, 1))
    eng = None
    firsts = off[:-1][np.array(LENGTHS) > 0].astype(np.int64)
    for keys, w, e in cases:
        (keys if w is None else w)[firsts] = 5 if kind == 0 and w is not None else 0.75      # every non-empty segment has mass: its edges have answers
        total = totals_of(keys, off, w, e)
        assert (total[np.array(LENGTHS) > 0] > 0).all()
        tt = np.stack([np.zeros_like(total), np.ones_like(total), total, total + np.uint64(1)], axis=1)
        got = run(rsx, keys, off, w, tt, False, descending, e, eng=eng)
        eng = got[5]
        written = check(got, keys, off, w, tt, False, descending, e)
        has = total > 0
        assert not written[:, 0].any() and not written[:, 3].any() and (written[:, 1] == has).all() and (written[:, 2] == has).all()
        got = run(rsx, keys, off, w, fr, True, descending, e, eng=eng)
        written = check(got, keys, off, w, fr, True, descending, e)
        assert not written[:, 2].any() and all((written[:, q] == has).all() for q in (0, 1, 3))
        assert (got[2][has, 1] >= got[2][has, 3]).all() and (got[2][has, 3] >= got[2][has, 0]).all()      # ranks of f = 1 >= 0.5 >= 0


@pytest.mark.parametrize("case", ["all_equal", "three"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["u32", "f32", "f64"])
def test_ties_decide(rsx, case, kind):
    """All keys equal, and three distinct keys, with random weights: the crossing lies purely in the tie phase, across tiles."""
    rng = np.random.default_rng(31 + kind)
    lens = [70000, 4097, 300, (1 << 18) + 11, 1025]
    off = offsets_from(lens, start=2)
    n = int(off[-1]) + 3
    dtype = [np.int32, np.uint64, np.float32][kind]
    x = np.full(n, 77, dtype=dtype) if case == "all_equal" else rng.integers(0, 3, n).astype(dtype)
    w = make_weights(kind, n, rng)
    total = totals_of(x, off, w)
    for desc in (False, True):
        for R in (4, 1):
            tt = random_targets(total, R, rng)
            tt[:, 0] = np.maximum(total // np.uint64(2), np.uint64(1))       # a crossing in the middle tiles
            got = run(rsx, x, off, w, tt, False, desc)
            written = check(got, x, off, w, tt, False, desc)
            assert written[:, 0].all()
        fr = rng.random((len(lens), 3))
        got = run(rsx, x, off, w, fr, True, desc)
        check(got, x, off, w, fr, True, desc)


def test_zero_mass(rsx):
    """A segment of all-zero weights writes only total = 0; zero-mass elements before the answer count in the rank and are never the answer."""
    rng = np.random.default_rng(37)
    lens = [5000, 300, 20000, 1, 6000, 1, 0]
    off = offsets_from(lens, start=0)
    n = int(off[-1])
    x = rng.integers(0, 50, n).astype(np.int32)
    w = rng.integers(0, 4, n).astype(np.uint32)
    w[0:5000] = 0                                                             # large, all zero
    w[5000:5300] = 0                                                          # small, all zero
    w[25300] = 0                                                              # one key, no mass
    seg = slice(5300, 25300)
    w[seg] = np.where(x[seg] < 25, 0, w[seg])                                 # the smaller half of the keys weighs nothing
    tt = np.array([[1, 2], [1, 1], [1, 7], [1, 1], [1, 3], [1, 2], [1, 1]], dtype=np.uint64)
    got = run(rsx, x, off, w, tt)
    written = check(got, x, off, w, tt)
    assert not written[0].any() and not written[1].any() and not written[3].any() and not written[6].any() and written[2].all()
    gk, gi, gr = got[0], got[1], got[2]
    below = int(np.count_nonzero(x[seg] < 25))
    assert int(gr[2, 0]) >= below and int(gk[2, 0]) >= 25 and w[5300 + int(gi[2, 0])] > 0
    fr = np.array([[0.0, 1.0]] * 7)
    got = run(rsx, x, off, w, fr, True)
    written = check(got, x, off, w, fr, True)
    assert not written[0].any() and written[2].all()
    assert w[5300 + int(got[1][2, 0])] > 0 and w[5300 + int(got[1][2, 1])] > 0     # first and last element WITH mass


@pytest.mark.parametrize("keys", ["random", "all_equal"])
def test_64_bit_carries(rsx, keys):
    """One segment of 2^19 elements of mass 2^32 - 1 each: targets on both sides of multiples of 2^32.  A 32-bit accumulator anywhere in the
    chain — histogram bins, group partials, the pick's scan, tie masses per tile, the tile walk, the locate — fails this."""
    rng = np.random.default_rng(41)
    n = 1 << 19
    x = rng.integers(0, 1 << 12, n).astype(np.uint32) if keys == "random" else np.full(n, 5, dtype=np.uint32)
    w = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    off = np.array([0, n], dtype=np.uint64)
    total = n * 0xFFFFFFFF
    eng = None
    for k in (1, 4097, 1 << 18, n - 2):
        base = k << 32
        tt = np.array([[base - 1, base, base + 1, base - k]], dtype=np.uint64)      # base - k = k * (2^32 - 1): exactly k elements
        got = run(rsx, x, off, w, tt, eng=eng)
        eng = got[5]
        written = check(got, x, off, w, tt)
        assert written.all() and int(got[4][0]) == total
        assert got[2][0].tolist() == [k if k > 1 else 0, k, k, k - 1]        # the smallest r with (r + 1) * (2^32 - 1) >= T
    tt = np.array([[total, total + 1, total - 1, 1]], dtype=np.uint64)
    got = run(rsx, x, off, w, tt, eng=eng)
    written = check(got, x, off, w, tt)
    assert written[0].tolist() == [True, False, True, True] and int(got[2][0, 0]) == n - 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_float_specials(rsx, dtype):
    """special() keys (NaNs of both signs, infinities, zeros, denormals) with separate weights: NaN and negative WEIGHTS weigh nothing,
    weights above 2^weight_exp saturate."""
    rng = np.random.default_rng(43)
    off = offsets_from([100, 3000, 9000, 1 << 17], start=1)
    n = int(off[-1])
    x = special(dtype, n, rng)
    for kind, wexp in ((1, -1), (2, 0), (1, 1)):
        w = make_weights(kind, n, rng)
        assert int((mass_np(w, wexp) == MASS_ONE).sum()) > 0 and np.isnan(w).any() and (w < 0).any()
        total = totals_of(x, off, w, wexp)
        for desc in (False, True):
            tt = random_targets(total, 4, rng)
            got = run(rsx, x, off, w, tt, False, desc, wexp)
            check(got, x, off, w, tt, False, desc, wexp)
    fr = rng.random((4, 2))
    for desc in (False, True):                                               # and the specials as their own weights
        got = run(rsx, x, off, None, fr, True, desc)
        check(got, x, off, None, fr, True, desc)


def dyadic_rows(rows, cols, rng, dtype=np.float32):
    """Probabilities that are multiples of 2^-24 and sum to 1 in every row: every partial sum is exact in float64 and as a mass."""
    cuts = np.sort(rng.integers(0, (1 << 24) + 1, (rows, cols - 1)), axis=1)
    parts = np.diff(np.concatenate([np.zeros((rows, 1), dtype=np.int64), cuts, np.full((rows, 1), 1 << 24)], axis=1), axis=1)
    return (parts / float(1 << 24)).astype(dtype)


@pytest.mark.parametrize("shape", [(12, 50257), (64, 4096), (3, 1 << 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_top_p_equals_the_sorting_chain(rsx, shape):
    """top_p against the library's own chain — sort_rows descending, float64 cumsum, searchsorted — on dyadic rows: equality on every row,
    in count and threshold; and compact_rows(bound=threshold) keeps the nucleus."""
    t = _torch()
    rng = np.random.default_rng(47)
    rows, cols = shape
    probs = t.from_numpy(dyadic_rows(rows, cols, rng)).cuda()
    p = t.from_numpy(rng.integers(1, 1025, rows) / 1024.0).cuda()
    p[0] = 1.0
    thr, count, kept = rsx.top_p(probs, p)
    sv, _ = rsx.sort_rows(probs, descending=True)
    cdf = t.cumsum(sv.to(t.float64), dim=-1)
    want = t.searchsorted(cdf, p.reshape(rows, 1)).reshape(rows)
    assert count.dtype == t.int64 and kept.dtype == t.float64 and thr.shape == (rows,)
    assert t.equal(count, want + 1)
    assert t.equal(thr, sv.gather(1, want.reshape(rows, 1)).reshape(rows))
    assert t.equal(kept, cdf.gather(1, want.reshape(rows, 1)).reshape(rows))
    thr2, count2, _ = rsx.top_p(probs, 0.9)
    want2 = t.searchsorted(cdf, t.full((rows, 1), 0.9, dtype=t.float64, device="cuda")).reshape(rows)
    assert t.equal(count2, want2 + 1) and t.equal(thr2, sv.gather(1, want2.reshape(rows, 1)).reshape(rows))
    nucleus = probs >= thr2.reshape(rows, 1)                                 # the follow-up: ties of the threshold beyond count come with it
    assert bool((nucleus.sum(dim=1) >= count2).all())
    v, c = rsx.top_p(probs.t().contiguous(), 0.9, dim=0)[:2]                 # rows along dim 0
    assert t.equal(v, thr2) and t.equal(c, count2)
    one = t.zeros((2, 300), device="cuda")
    one[0, 7] = 1.0                                                          # one-hot: exact; and a row without mass
    thr3, count3, kept3 = rsx.top_p(one, 0.5)
    assert thr3.tolist() == [1.0, 0.0] and count3.tolist() == [1, 0] and kept3[0].item() == 1.0 and t.isnan(kept3[1]).item()


def test_weighted_quantile_integer_weights_equal_kthvalue_of_the_repeated_row(rsx):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(53)
    for dt, L in ((t.int32, 9000), (t.float32, 3000), (t.int64, 70000), (t.float64, 257)):
        x = t.randint(-40, 40, (L,), device="cuda", generator=g).to(dt)
        w = t.randint(0, 6, (L,), device="cuda", generator=g, dtype=t.int32)
        rep = rsx.repeat_interleave(x, w)
        total = int(w.sum().item())
        qs = [0.0, 0.1, 0.5, 1 / 3, 0.99, 1.0]                               # 6: two engine calls
        v, i = rsx.weighted_quantile(x, w, qs)
        assert v.shape == (6,) and i.dtype == t.int64
        for j, q in enumerate(qs):
            T = min(max(int(np.ceil(float(total) * q)), 1), total)
            assert v[j].item() == rsx.kthvalue(rep, T)[0].item(), (dt, q)
            assert x[i[j]].item() == v[j].item() and w[i[j]].item() > 0
        assert rsx.weighted_median(x, w)[0].item() == v[2].item()
    # float weights: the scale comes from weight_max (read back once when not given), rows along a dim
    x = t.randn((5, 4000, 3), device="cuda", generator=g)
    w = t.rand((5, 4000, 3), device="cuda", generator=g) * 100
    v, i = rsx.weighted_quantile(x, w, 0.25, dim=1)
    v2, i2 = rsx.weighted_quantile(x, w, 0.25, dim=1, weight_max=float(w.max().item()))
    assert v.shape == (5, 3) and t.equal(v, v2) and t.equal(i, i2) and t.equal(x.gather(1, i.unsqueeze(1)).squeeze(1), v)
    xs, order = t.sort(x, dim=1, stable=True)
    cw = t.cumsum(w.gather(1, order).double(), dim=1)
    # The float64 chain names the same element unless its running weight passes within the quantisation of the crossing: a weight loses
    # less than 2^(7 - 31) (weight_max <= 128), 4000 of them less than 2.4e-4, against steps of about 50 — so at most one rank apart.
    near = (cw >= 0.25 * cw[:, -1:, :]).double().argmax(dim=1)
    got_rank = (order == i.unsqueeze(1)).double().argmax(dim=1)
    assert (got_rank - near).abs().max().item() <= 1
    for bad in (t.float16, t.bfloat16, t.bool):
        with pytest.raises(TypeError):
            rsx.top_p(t.zeros(10, dtype=bad, device="cuda"), 0.5)
        with pytest.raises(TypeError):
            rsx.weighted_median(t.zeros(10, device="cuda"), t.zeros(10, dtype=bad, device="cuda"))
        with pytest.raises(TypeError):
            rsx.weighted_median(t.zeros(10, dtype=bad, device="cuda"), t.ones(10, device="cuda"))


def test_segmented_helper(rsx):
    t = _torch()
    rng = np.random.default_rng(59)
    x = random_bits(np.float32, 30001, rng)
    w = make_weights(2, 30001, rng)
    off = offsets_from([100, 0, 1, 7000, 3000, 5], start=1)
    keys = t.from_numpy(x).cuda()[1:]                                        # misaligned views: copied first
    wts = t.from_numpy(w).cuda()[1:]
    offsets = t.from_numpy(off.astype(np.int64)).cuda()
    xs, ws = x[1:], w[1:]
    total = totals_of(xs, off, ws)
    for R in (1, 4, 9):                                                      # 9: three engine calls
        tt = random_targets(total, R, rng)
        for desc in (False, True):
            v, i, r, m, tot = rsx.segmented_weighted_select(keys, offsets, wts, targets=t.from_numpy(tt.astype(np.int64)).cuda(), descending=desc)
            wk, wi, wr, wm, written, wt, _ = wselect_oracle(xs, off, ws, tt, False, desc)
            assert v.shape == (6, R) and i.dtype == t.int64 and r.dtype == t.int64 and tot.shape == (6,)
            assert np.array_equal(v.cpu().numpy().view(np.uint32), np.where(written, wk, 0))
            assert np.array_equal(i.cpu().numpy(), np.where(written, wi.astype(np.int64), -1))
            assert np.array_equal(r.cpu().numpy(), np.where(written, wr.astype(np.int64), -1))
            assert np.array_equal(m.cpu().numpy().view(np.uint64), np.where(written, wm, 0)) and np.array_equal(tot.cpu().numpy().view(np.uint64), wt)
    fr = rng.random(6)
    v, i, r, m, tot = rsx.segmented_weighted_select(keys, offsets, fractions=t.from_numpy(fr).cuda())     # fractions [S], keys as weights
    wk, wi, wr, wm, written, wt, _ = wselect_oracle(xs, off, None, fr, True)
    assert v.shape == (6, 1) and np.array_equal(i.cpu().numpy(), np.where(written, wi.astype(np.int64), -1))
    with pytest.raises(ValueError):
        rsx.segmented_weighted_select(keys, offsets, wts)                    # neither targets nor fractions
    with pytest.raises(ValueError):
        rsx.segmented_weighted_select(keys, offsets, t.ones(30000, dtype=t.int32, device="cuda"), fractions=t.from_numpy(fr).cuda(), weight_exp=1)
    with pytest.raises(TypeError):
        rsx.segmented_weighted_select(keys.to(t.int32), offsets, fractions=t.from_numpy(fr).cuda())       # integer keys are no weights


def test_bits_equal_across_engines_stream_and_graph(rsx):
    """Two engines of different capacity, a side stream, and a graph replay after one eager call: equal input, equal bits."""
    t = _torch()
    rng = np.random.default_rng(61)
    lens = [100000, 5000, 1, 0, 150000, 300]
    off = offsets_from(lens, start=0)
    n, nseg, R = 300000, len(lens), 4
    x = random_bits(np.float32, n, rng)
    x[::3] = x[0]
    w = make_weights(1, n, rng)
    fr = rng.random((nseg, R))
    first = run(rsx, x, off, w, fr, True, eng=rsx.Engine(np.float32, n))
    check(first, x, off, w, fr, True)
    second = run(rsx, x, off, w, fr, True, eng=rsx.Engine(np.float32, 1 << 22))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:5], second[:5]))

    stream = t.cuda.Stream()
    eng = rsx.Engine(np.float32, n)
    eng.set_stream(stream.cuda_stream)
    keys, wts = dev(t, x), dev(t, w)
    offs, frs = dev(t, off), dev(t, fr)
    out = [t.zeros((nseg, R), dtype=d, device="cuda") for d in (t.int32, t.int32, t.int32, t.int64)] + [t.zeros(nseg, dtype=t.int64, device="cuda")]

    def call():
        eng.segmented_weighted_select(keys.data_ptr(), wts.data_ptr(), n, offs.data_ptr(), nseg, frs.data_ptr(), R, rsx.WSELECT_FRACTION, 1, 0,
                                      *[o.data_ptr() for o in out])

    def same():
        got = [o.cpu().numpy() for o in out]
        return (got[0].view(np.uint32).tobytes() == first[0].tobytes() and got[1].view(np.uint32).tobytes() == first[1].tobytes()
                and got[2].view(np.uint32).tobytes() == first[2].tobytes() and got[3].view(np.uint64).tobytes() == first[3].tobytes()
                and got[4].view(np.uint64).tobytes() == first[4].tobytes())

    def reset():                                                             # the sentinel's bits, so that unwritten slots compare equal
        for o in out[:3]:
            o.fill_(0xC3C3C3C3 - (1 << 32))
        for o in out[3:]:
            o.fill_(0xC3C3C3C3C3C3C3C3 - (1 << 64))
        t.cuda.synchronize()

    reset()
    call()                                                                   # eager on the side stream; scratch grows here
    stream.synchronize()
    assert same()
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=stream):
        call()
    reset()
    graph.replay()
    t.cuda.synchronize()
    assert same()
    eng.sync()


@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_reported_once_under_this_calls_name(rsx, bad):
    rng = np.random.default_rng(67)
    n = 60000
    x = random_bits(np.uint32, n, rng)
    w = make_weights(0, n, rng)
    if bad == "decreasing":
        off = np.array([0, 100, 20000, 5000], dtype=np.uint64)                # segment 2 = [20000, 5000)
    else:
        off = np.array([0, 100, 20000, n + 1], dtype=np.uint64)               # segment 2 ends past n
    tt = np.array([[1, 50], [10000, 1], [1, 2]], dtype=np.uint64)
    eng = rsx.Engine(np.uint32, n)
    got = run(rsx, x, off, w, tt, eng=eng)                                   # guard bands checked inside
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "segment 2 " in str(ei.value) and "rsx_segmented_weighted_select" in str(ei.value)
    eng.sync()                                                               # reported once
    written = check(got, x, off, w, tt)                                      # the bad row keeps the sentinel, its total included
    assert written[:2].all() and not written[2].any()
    good = np.array([0, 3, 5000, 5001, 30000, n], dtype=np.uint64)
    tt = random_targets(totals_of(x, good, w), 2, rng)
    got = run(rsx, x, good, w, tt, eng=eng)
    eng.sync()                                                               # the engine is usable, and nothing is pending
    check(got, x, good, w, tt)


def test_refusals(rsx):
    t = _torch()
    n = 1 << 14
    eng = rsx.Engine(np.uint32, n)
    feng = rsx.Engine(np.float32, n)
    x = t.zeros(n, dtype=t.int32, device="cuda")
    w = t.ones(n, dtype=t.float32, device="cuda")
    off = t.tensor([0, n], dtype=t.int64, device="cuda")
    tg = t.ones(16, dtype=t.int64, device="cuda")
    out = [t.full((16,), 7, dtype=d, device="cuda") for d in (t.int32, t.int32, t.int32, t.int64, t.int64)]
    o = [b.data_ptr() for b in out]

    def call(e=eng, keys=x.data_ptr(), wts=w.data_ptr(), nn=n, R=4, flags=0, kind=1, wexp=0, outs=o):
        e.segmented_weighted_select(keys, wts, nn, off.data_ptr(), 1, tg.data_ptr(), R, flags, kind, wexp, *outs)

    with pytest.raises(rsx.RadixSortError) as ei:                            # R = 5
        call(R=5)
    assert ei.value.status == 4 and "call again" in str(ei.value)
    call(R=0)                                                                # R == 0: nothing
    with pytest.raises(rsx.RadixSortError) as ei:                            # NULL weights on an integer engine
        call(wts=None)
    assert ei.value.status == 1
    with pytest.raises(rsx.RadixSortError) as ei:                            # NULL weights, float engine, the wrong float kind
        call(e=feng, wts=None, kind=2)
    assert ei.value.status == 1
    with pytest.raises(rsx.RadixSortError) as ei:                            # misaligned keys
        call(keys=x.data_ptr() + 4, nn=100)
    assert ei.value.status == 1
    with pytest.raises(rsx.RadixSortError) as ei:                            # an output overlaps the input
        call(outs=[x.data_ptr() + 64] + o[1:])
    assert ei.value.status == 1
    with pytest.raises(rsx.RadixSortError):                                  # an output overlaps the weights
        call(outs=o[:3] + [w.data_ptr(), o[4]])
    with pytest.raises(rsx.RadixSortError):                                  # two outputs overlap
        call(outs=[o[0], o[0] + 8] + o[2:])
    with pytest.raises(rsx.RadixSortError):                                  # misaligned mass output
        call(outs=o[:3] + [o[3] + 4, o[4]])
    with pytest.raises(rsx.RadixSortError):                                  # an unknown flag
        call(flags=1)
    with pytest.raises(rsx.RadixSortError):                                  # weight_exp with raw masses
        call(kind=0, wexp=1)
    with pytest.raises(rsx.RadixSortError):                                  # an unknown weight kind
        call(kind=3)
    with pytest.raises(rsx.RadixSortError) as ei:                            # beyond capacity
        call(nn=n + 1)
    assert ei.value.status == 7
    eng.sync()
    feng.sync()
    assert all(bool((b == 7).all()) for b in out)                            # nothing was written by any of them
    call(outs=o[:2] + [None, None, None])                                    # the optional outputs may be absent
    eng.sync()
    assert out[0][0].item() == 0 and out[1][0].item() == 0 and bool((out[2] == 7).all())
