"""The segmented rank (rsx_segmented_rank, radix_sort_amd.segmented_rank and rankdata) on the GPU.

The referee is tests/_rank_ref.py; every comparison is exact integer equality with it, entry for entry: there is no tolerance anywhere.
Both outputs are pre-filled with the family's sentinel — a position outside [off[0], off[S]) must still hold it — and followed by guard
bands, with a few bytes in front so that they start aligned to their element only.
Every engine a test creates is closed by the test: an engine left to the garbage collector (a pytest.raises block keeps its frame in a
reference cycle) would be freed at an arbitrary later moment, possibly inside another test's stream capture.
"""
import numpy as np
import pytest

import _rank_ref as R
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, FILL32, GUARD

pytestmark = pytest.mark.gpu

GUARD_BYTE = 0xA5
FRONT = 4
KEY_DTYPES = ["uint32", "int32", "uint64", "int64", "float32", "float64"]
EDGE_LENGTHS = [0, 1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4095, 4096]          # every class shape and both of its edges
LARGE_LENGTHS = [4097, 8192, 8193, 3 * 4096 + 5]
# empty, one-key, small and large segments; off[0] != 0; large segments that start off the 4096 grid
MIXED_LENGTHS = [0, 1, 2, 260, 0, 1200, 3500, 30000, 1, 4097, 700, 9000, 4096, 0]
MIXED_START, MIXED_TAIL = 37, 50


def layout(lengths, start=0, tail=0):
    off = np.concatenate([[start], start + np.cumsum(lengths)]).astype(np.uint64)
    return int(off[-1]) + tail, off


def random_keys(rng, dt, n, values=8):
    """keys from an alphabet of `values` values, the fourth one as frequent as all others together: long tie groups"""
    dt = np.dtype(dt)
    if dt.kind == "f":
        alphabet = (rng.standard_normal(values) * 4).astype(dt)
    else:
        alphabet = rng.integers(-1000 if dt.kind == "i" else 0, 1000, values).astype(dt)
    p = np.full(values, 0.5 / (values - 1))
    p[3] = 0.5
    return alphabet[rng.choice(values, n, p=p)]


def _band(t, nbytes):
    buf = dev(t, np.concatenate([np.full(FRONT + nbytes, FILL, dtype=np.uint8), np.full(GUARD, GUARD_BYTE, dtype=np.uint8)]))
    assert buf.data_ptr() % 16 == 0
    return buf


def _unband(buf, nbytes, what):
    raw = buf.cpu().numpy().view(np.uint8)
    assert np.all(raw[-GUARD:] == GUARD_BYTE), f"guard band behind the {what} written"
    assert np.all(raw[:FRONT] == FILL), f"bytes before the {what} written"
    return raw[FRONT:FRONT + nbytes].copy().view(np.uint32)


def run(rsx, eng, x, off, method, want_ties=True):
    """One rsx_segmented_rank through the Engine API.  Returns (ranks [n] uint32, ties [n] uint32 or None), the sentinel where nothing was
    written."""
    t = _torch()
    n = x.size
    nseg = 1 if off is None else len(off) - 1
    k = dev(t, x) if n else dev(t, np.zeros(4, dtype=x.dtype))
    o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
    r_buf, t_buf = _band(t, n * 4), _band(t, n * 4)
    eng.segmented_rank(k.data_ptr(), n, None if o is None else o.data_ptr(), nseg, method, r_buf.data_ptr() + FRONT,
                       t_buf.data_ptr() + FRONT if want_ties else None)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    ranks, ties = _unband(r_buf, n * 4, "ranks"), _unband(t_buf, n * 4, "ties")
    assert want_ties or np.all(ties == FILL32), "a NULL d_ties_out: the buffer was not passed"
    return ranks, ties if want_ties else None


def check(got, want, method, what=""):
    ranks, ties = got
    wr, wt, _ = want
    for name, g, w in (("ranks", ranks, wr[method]), ("ties", ties, wt)):
        if g is None:
            continue
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what} method {method}: {name} differ at {bad[:6].tolist()} (of {len(bad)}): got {g[bad[:6]].tolist()}, want {w[bad[:6]].tolist()}"


def run_check_all(rsx, eng, x, off, descending=False, what="", methods=range(5)):
    """every method with the tie counts, and (alternating) without"""
    want = R.rank_oracle(x, off, descending, fill=FILL32)
    for method in methods:
        check(run(rsx, eng, x, off, method), want, method, what)
        check(run(rsx, eng, x, off, method, want_ties=False), want, method, what + " (no ties)")
    return want


def engine(rsx, dt, cap, descending=False):
    return rsx.Engine(np.dtype(dt), cap, payload=True, descending=descending)


# -- 1. the shapes ----------------------------------------------------------------------------------------------------------------------------------

def test_hand_case(rsx):
    eng = engine(rsx, np.int32, 4096)
    x = np.array([30, 10, 20, 10, 30, 30, 7], dtype=np.int32)
    off = [0, 6]
    assert run(rsx, eng, x, off, rsx.RANK_ORDINAL)[0].tolist() == [3, 0, 2, 1, 4, 5, FILL32]
    assert run(rsx, eng, x, off, rsx.RANK_MIN)[0].tolist() == [3, 0, 2, 0, 3, 3, FILL32]
    assert run(rsx, eng, x, off, rsx.RANK_MAX)[0].tolist() == [5, 1, 2, 1, 5, 5, FILL32]
    assert run(rsx, eng, x, off, rsx.RANK_DENSE)[0].tolist() == [2, 0, 1, 0, 2, 2, FILL32]
    ranks, ties = run(rsx, eng, x, off, rsx.RANK_AVERAGE)
    assert ranks.tolist() == [8, 1, 4, 1, 8, 8, FILL32] and ties.tolist() == [3, 2, 1, 2, 3, 3, FILL32]
    eng.sync()
    eng.close()


def test_class_edges_in_one_call(rsx):
    rng = np.random.default_rng(1)
    n, off = layout(EDGE_LENGTHS, start=5, tail=9)
    x = random_keys(rng, np.uint32, n)
    eng = engine(rsx, np.uint32, 1 << 15)
    run_check_all(rsx, eng, x, off, what="class edges")
    eng.sync()
    eng.close()


def test_class_edges_separately(rsx):
    rng = np.random.default_rng(2)
    eng = engine(rsx, np.uint64, 8192)
    for L in EDGE_LENGTHS:
        n, off = layout([L], start=3, tail=2)
        x = random_keys(rng, np.uint64, n)
        run_check_all(rsx, eng, x, off, what=f"one segment of {L}", methods=(rsx.RANK_AVERAGE, rsx.RANK_DENSE))
    eng.sync()
    eng.close()


@pytest.mark.parametrize("L", LARGE_LENGTHS)
def test_large_segments(rsx, L):
    rng = np.random.default_rng(L)
    n, off = layout([L, 5, L], start=11, tail=3)                                 # the second one starts off the grid
    x = random_keys(rng, np.uint32, n)
    eng = engine(rsx, np.uint32, 1 << 15)
    run_check_all(rsx, eng, x, off, what=f"large {L}")
    eng.sync()
    eng.close()


def mixed_case(rng, dt):
    n, off = layout(MIXED_LENGTHS, MIXED_START, MIXED_TAIL)
    return n, off, random_keys(rng, dt, n)


def test_mixed_call_with_groups_across_tiles(rsx):
    rng = np.random.default_rng(4)
    n, off, x = mixed_case(rng, np.uint32)
    assert int(off[0]) != 0 and any(int(a) % 4096 and int(b - a) > 4096 for a, b in zip(off[:-1], off[1:]))
    facts = [R.tile_facts(a, s) for a, s in R.sorted_keys_layout(x, off)]
    assert any(c for c, _ in facts) and any(h for _, h in facts), "the input must have a group crossing a 4096 boundary and a tile without a head"
    eng = engine(rsx, np.uint32, 1 << 16)
    run_check_all(rsx, eng, x, off, what="mixed")
    eng.sync()
    eng.close()


def test_equal_and_increasing_large_segments(rsx):
    n, off = layout([3 * 4096 + 5, 9000, 100], start=1, tail=1)
    x = np.zeros(n, dtype=np.int64)
    x[:int(off[1])] = -5                                                         # 12 293 equal keys
    x[int(off[1]):int(off[2])] = np.arange(9000) * 3 - 9000                      # strictly increasing
    x[int(off[2]):] = 1
    eng = engine(rsx, np.int64, 1 << 15)
    want = run_check_all(rsx, eng, x, off, what="equal / increasing")
    assert np.all(want[1][1:int(off[1])] == 3 * 4096 + 5) and np.all(want[1][int(off[1]):int(off[2])] == 1)
    run_check_all(rsx, eng, x[::-1].copy(), (n - off[::-1]).astype(np.uint64), what="reversed")      # strictly decreasing input
    eng.sync()
    eng.close()


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dt", KEY_DTYPES)
def test_key_kinds_and_directions(rsx, dt, descending):
    rng = np.random.default_rng(KEY_DTYPES.index(dt) * 2 + descending)
    n, off, x = mixed_case(rng, dt)
    if np.dtype(dt).kind != "f":                                                 # the extremes of the type among the keys
        info = np.iinfo(dt)
        x[rng.integers(0, n, 40)] = info.min
        x[rng.integers(0, n, 40)] = info.max
    eng = engine(rsx, dt, 1 << 16, descending)
    run_check_all(rsx, eng, x, off, descending, what=f"{dt} descending={descending}", methods=(rsx.RANK_AVERAGE, rsx.RANK_ORDINAL, rsx.RANK_DENSE))
    eng.sync()
    eng.close()


@pytest.mark.parametrize("descending", [False, True])
def test_float_specials(rsx, descending):
    rng = np.random.default_rng(6)
    n, off, _ = mixed_case(rng, np.float32)
    nan_neg = np.array([0xFFC00000, 0xFFC00001], dtype=np.uint32).view(np.float32)
    nan_pos = np.array([0x7FC00000, 0x7FC00001], dtype=np.uint32).view(np.float32)
    alphabet = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -1.5], dtype=np.float32), nan_neg, nan_pos])
    x = alphabet[rng.integers(0, len(alphabet), n)]
    eng = engine(rsx, np.float32, 1 << 16, descending)
    want = run_check_all(rsx, eng, x, off, descending, what="float specials")
    # -0.0 and +0.0 do not tie, NaNs with equal bits do: in the 30000-key segment every one of the ten values forms one group
    a, b = int(off[7]), int(off[8])
    assert len(np.unique(want[0][R.DENSE][a:b])) == len(alphabet)
    eng.sync()
    eng.close()


@pytest.mark.parametrize("n", [1, 5, 4096, 4097, 10000])
def test_flat_form(rsx, n):
    rng = np.random.default_rng(n)
    x = random_keys(rng, np.int32, n)
    eng = engine(rsx, np.int32, 1 << 14)
    run_check_all(rsx, eng, x, None, what=f"flat {n}")
    eng.sync()
    eng.close()


# -- 2. against the library's own sort and torch ---------------------------------------------------------------------------------------------------

def test_ordinal_is_the_inverse_of_the_sorts_payload(rsx):
    t = _torch()
    rng = np.random.default_rng(8)
    n, off, x = mixed_case(rng, np.int32)
    keys = dev(t, x)
    offsets = t.from_numpy(off.astype(np.int64)).cuda()
    iota = t.arange(n, dtype=t.int32, device="cuda")
    _, perm = rsx.segmented_sort(keys, offsets, iota)
    got = rsx.segmented_rank(keys, offsets, method="ordinal")
    lo, hi = int(off[0]), int(off[-1])
    seg = t.searchsorted(offsets, t.arange(n, device="cuda"), right=True) - 1    # the segment of every position in [lo, hi)
    want = t.zeros(n, dtype=t.int64, device="cuda")
    idx = t.arange(lo, hi, device="cuda")
    want[perm[lo:hi].to(t.int64)] = idx - offsets[seg[lo:hi]]
    assert got.dtype == t.int64 and bool((got == want).all())
    t.cuda.synchronize()


def test_ordinal_equals_double_argsort(rsx):
    t = _torch()
    gen = t.Generator(device="cuda").manual_seed(9)
    for rows, cols in ((7, 300), (3, 5000)):
        x = t.randint(-20, 20, (rows, cols), dtype=t.int32, device="cuda", generator=gen)
        want = t.argsort(t.argsort(x, dim=-1, stable=True), dim=-1, stable=True)
        got = rsx.rankdata(x, method="ordinal") - 1
        assert got.dtype == t.int64 and bool((got == want).all())
        wantd = t.argsort(t.argsort(x, dim=-1, stable=True, descending=True), dim=-1, stable=True)
        assert bool((rsx.rankdata(x, method="ordinal", descending=True) - 1 == wantd).all())
    t.cuda.synchronize()


# -- 3. the helpers -------------------------------------------------------------------------------------------------------------------------------

def _rankdata_ref(x, method, axis, descending=False):
    """1-based, float64 for the average, along `axis` (None: flattened)"""
    code = R.METHODS[method]
    if axis is None:
        ranks, _ = R.rank_segment(x.reshape(-1), descending)
        out = ranks[code].reshape(x.shape)
    else:
        moved = np.moveaxis(x, axis, -1)
        flat = np.ascontiguousarray(moved).reshape(-1, moved.shape[-1])
        out = np.moveaxis(np.stack([R.rank_segment(row, descending)[0][code] for row in flat]).reshape(moved.shape), -1, axis)
    return out.astype(np.float64) / 2 + 1 if method == "average" else out.astype(np.int64) + 1


def test_rankdata_along_dims(rsx):
    t = _torch()
    rng = np.random.default_rng(10)
    x = rng.integers(0, 6, (5, 7, 9)).astype(np.float32)
    xd = t.from_numpy(x).cuda()
    for dim in (0, -1, 1):
        for method in R.METHODS:
            got = rsx.rankdata(xd, method=method, dim=dim)
            want = _rankdata_ref(x, method, dim)
            assert got.shape == xd.shape and got.dtype == (t.float64 if method == "average" else t.int64)
            assert np.array_equal(got.cpu().numpy(), want), (dim, method)
    got = rsx.rankdata(xd.transpose(0, 2), method="min", dim=1, descending=True)             # a non-contiguous view
    assert np.array_equal(got.cpu().numpy(), _rankdata_ref(np.ascontiguousarray(x.transpose(2, 1, 0)), "min", 1, True))
    t.cuda.synchronize()


def test_rankdata_flattened_and_pct(rsx):
    t = _torch()
    rng = np.random.default_rng(11)
    x = rng.integers(-50, 50, (100, 100)).astype(np.int64)                       # 10 000 keys: the flat chain
    xd = t.from_numpy(x).cuda()
    for method in R.METHODS:
        got = rsx.rankdata(xd, method=method, dim=None)
        assert got.shape == xd.shape and np.array_equal(got.cpu().numpy(), _rankdata_ref(x, method, None)), method
    got = rsx.rankdata(xd, method="max", dim=-1, pct=True)
    assert got.dtype == t.float64 and np.array_equal(got.cpu().numpy(), _rankdata_ref(x, "max", -1).astype(np.float64) / 100)
    got = rsx.rankdata(xd, dim=None, pct=True)
    assert np.array_equal(got.cpu().numpy(), _rankdata_ref(x, "average", None) / 10000)
    ranks, ties = rsx.segmented_rank(xd.reshape(-1), t.tensor([0, 10, 10, 9000], device="cuda"), method="average", return_ties=True)
    wr, wt, _ = R.rank_oracle(x.reshape(-1), [0, 10, 10, 9000])
    assert ranks.dtype == t.float64 and ties.dtype == t.int64
    assert np.array_equal(ranks.cpu().numpy(), wr[R.AVERAGE] / 2) and np.array_equal(ties.cpu().numpy(), wt.astype(np.int64))
    assert rsx.rankdata(xd[:0], dim=-1).shape == (0, 100) and rsx.rankdata(xd[:, :0], dim=None).shape == (100, 0)
    t.cuda.synchronize()


# -- 4. bad offsets, refusals ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_reported_once(rsx, bad):
    rng = np.random.default_rng(23)
    n = 40000
    x = random_keys(rng, np.uint32, n)
    off = np.array([0, 100, 5000, 4000 if bad == "decreasing" else n + 1, n], dtype=np.uint64)       # segment 2 is the first bad one
    eng = engine(rsx, np.uint32, 1 << 16)
    ranks, ties = run(rsx, eng, x, off, rsx.RANK_AVERAGE)                        # guard bands checked inside
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "rsx_segmented_rank" in str(ei.value) and "segment 2 " in str(ei.value)
    eng.sync()                                                                   # reported once
    assert np.all(ranks == FILL32) and np.all(ties == FILL32)
    good = np.array([0, 3, 5000, 5001, n], dtype=np.uint64)                      # the engine stays usable: the next call is right
    run_check_all(rsx, eng, x, good, what="after bad offsets", methods=(rsx.RANK_AVERAGE,))
    eng.sync()
    eng.close()


def test_refusals(rsx):
    t = _torch()
    n = 100
    k = dev(t, np.ones(n + 4, dtype=np.uint32))
    o = dev(t, np.array([0, 50, n], dtype=np.uint64))
    rout, tout = dev(t, np.zeros(n + 4, dtype=np.uint32)), dev(t, np.zeros(n + 4, dtype=np.uint32))
    eng, plain = engine(rsx, np.uint32, 4096), rsx.Engine(np.uint32, 4096)

    def refused(status, text, e, *args):
        with pytest.raises(rsx.RadixSortError) as ei:
            e.segmented_rank(*args)
        assert ei.value.status == status and "rsx_segmented_rank" in str(ei.value) and text in str(ei.value), str(ei.value)

    base = lambda **kw: tuple({**dict(d_keys=k.data_ptr(), n=n, d_offsets=o.data_ptr(), num_segments=2, method=rsx.RANK_AVERAGE, rout=rout.data_ptr(),
                                      tout=tout.data_ptr()), **kw}.values())
    refused(4, "method", eng, *base(method=5))
    refused(1, "has_payload = 1", plain, *base())                                                   # an engine without payload
    refused(1, "capacity", eng, *base(n=4097))
    refused(1, "keys must be a 16-byte aligned", eng, *base(d_keys=k.data_ptr() + 4))
    refused(1, "keys must be a 16-byte aligned", eng, *base(d_keys=None))
    refused(1, "rank output", eng, *base(rout=None))
    refused(1, "rank output", eng, *base(rout=rout.data_ptr() + 2))
    refused(1, "ties output", eng, *base(tout=tout.data_ptr() + 1))
    refused(1, "offsets must be an 8-byte aligned", eng, *base(d_offsets=o.data_ptr() + 4))
    refused(1, "overlaps an input", eng, *base(rout=k.data_ptr()))                                    # overlapping buffers
    refused(1, "overlaps an input", eng, *base(tout=o.data_ptr()))
    refused(1, "two outputs overlap", eng, *base(tout=rout.data_ptr() + 8))
    lib = rsx.load_library()                                                                          # flags and the engine: below the Engine API
    assert lib.rsx_segmented_rank(eng._h, k.data_ptr(), n, o.data_ptr(), 2, 1, 0, rout.data_ptr(), None) == 4
    assert b"flags" in lib.rsx_last_error() and b"rsx_segmented_rank" in lib.rsx_last_error()
    assert lib.rsx_segmented_rank(None, k.data_ptr(), n, o.data_ptr(), 2, 0, 0, rout.data_ptr(), None) == 4
    assert b"null engine" in lib.rsx_last_error()
    # accepted and empty: n == 0, no segments
    eng.segmented_rank(*base(n=0))
    eng.segmented_rank(*base(num_segments=0))
    eng.sync()
    assert bool((rout == 0).all()) and bool((tout == 0).all())
    eng.close()
    plain.close()


# -- 5. reproducibility, engine state ------------------------------------------------------------------------------------------------------------

def test_reproducible_across_engines_streams_and_replays(rsx):
    t = _torch()
    rng = np.random.default_rng(70)
    n, off, x = mixed_case(rng, np.float32)
    kd, od = dev(t, x), dev(t, off)
    method = rsx.RANK_AVERAGE
    want = R.rank_oracle(x, off, True, fill=FILL32)
    results = []
    for i, cap in enumerate((1 << 16, 1 << 20)):
        side = t.cuda.Stream()
        eng = engine(rsx, np.float32, cap, descending=True)
        eng.set_stream(side.cuda_stream)
        rout, tout = dev(t, np.full(n * 4, FILL, dtype=np.uint8)), dev(t, np.full(n * 4, FILL, dtype=np.uint8))
        call = lambda: eng.segmented_rank(kd.data_ptr(), n, od.data_ptr(), len(off) - 1, method, rout.data_ptr(), tout.data_ptr())
        result = lambda: (rout.cpu().numpy().view(np.uint32).copy(), tout.cpu().numpy().view(np.uint32).copy())
        call()                                                                   # eager: the first call of an engine allocates its scratch
        eng.sync()
        results.append(result())
        check(results[-1], want, method, f"capacity {cap}")
        if i == 1:                                                               # a linear capture on the side stream: no parallel branches
            graph = t.cuda.CUDAGraph()
            with t.cuda.graph(graph, stream=side):
                call()
            for rep in range(2):
                x2 = random_keys(rng, np.float32, n)
                kd.copy_(dev(t, x2))                                             # rewritten in place
                for buf in (rout, tout):
                    buf.fill_(FILL - 256)
                t.cuda.synchronize()
                graph.replay()
                t.cuda.synchronize()
                check(result(), R.rank_oracle(x2, off, True, fill=FILL32), method, f"replay {rep}")
            del graph
        eng.sync()
        eng.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(results[0], results[1]))


def test_rank_after_a_sort_on_the_same_engine(rsx):
    t = _torch()
    rng = np.random.default_rng(12)
    n, off, x = mixed_case(rng, np.uint64)
    eng = engine(rsx, np.uint64, 1 << 16)
    other = rng.integers(0, 1 << 60, n).astype(np.uint64)
    k, o, p = dev(t, other), dev(t, off), dev(t, np.arange(n, dtype=np.uint32))
    k_out, p_out = dev(t, other), dev(t, np.zeros(n, dtype=np.uint32))
    eng.segmented_sort(k.data_ptr(), n, o.data_ptr(), len(off) - 1, k_out.data_ptr(), p.data_ptr(), p_out.data_ptr())
    run_check_all(rsx, eng, x, off, what="after a segmented sort", methods=(rsx.RANK_AVERAGE, rsx.RANK_ORDINAL))
    run_check_all(rsx, eng, x[:9000], None, what="flat after segmented", methods=(rsx.RANK_MIN,))
    run_check_all(rsx, eng, x, off, what="segmented after flat", methods=(rsx.RANK_MAX,))
    eng.sync()
    eng.close()
