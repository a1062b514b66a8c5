"""Segmented expand (rsx_segmented_expand, radix_sort_amd.segmented_expand / segment_ids / repeat_interleave / gather_ranges ...) on the GPU.

The referee is tests/_expand_ref.py (np.repeat and plain loops).  Every comparison is exact, values by their bits.  The outputs start out
holding a sentinel and lie between guard bands, so that a position outside [off[0], off[S]) that was written shows.  Every engine here has
capacity 4096 unless a test says otherwise: the call is not bound by it.  The layouts are the smallest that reach each path of
expand_tile_kernel; tests/test_expand.py proves from the offsets alone that they do.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import _expand_ref as R
from _expand_ref import TILE, expand_oracle, offsets_from
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, GUARD

pytestmark = pytest.mark.gpu

CAP = 4096
UWORD = {4: np.uint32, 8: np.uint64}
OUTPUTS = ("values", "segment", "rank")


def engine(rsx, stream=None, capacity=CAP, dtype=np.uint32, **kw):
    eng = rsx.Engine(dtype, capacity, **kw)
    if stream is not None:
        eng.set_stream(stream)
    return eng


def banded(t, nbytes, shift_bytes):
    """a device buffer: guard | shift | nbytes of sentinel | guard; returns (tensor, byte offset of the payload)"""
    pre = GUARD + shift_bytes
    return dev(t, np.concatenate([np.full(pre, 0x5A, dtype=np.uint8), np.full(nbytes, FILL, dtype=np.uint8), np.full(GUARD, 0xA5, dtype=np.uint8)])), pre


def unband(buf, pre, nbytes, what):
    b = buf.cpu().numpy().view(np.uint8)
    assert np.all(b[:pre] == 0x5A), f"{what}: bytes before the output written"
    assert np.all(b[pre + nbytes:] == 0xA5), f"{what}: guard band written"
    return b[pre:pre + nbytes].copy()


def run(rsx, off, n, values=None, starts=None, want=OUTPUTS, eng=None, shifts=(0, 0, 0, 0), sync=True):
    """One rsx_segmented_expand through the Engine API.  values: unsigned words (the opaque bits), one per segment or, with starts, the
    source of the ranged gather.  shifts: the value input and the three outputs lie that many ELEMENTS past a 16-byte aligned address.
    Returns ({output name: host array of n words}, engine)."""
    t = _torch()
    nseg = len(off) - 1
    vb = 4 if values is None else values.dtype.itemsize
    o = dev(t, np.asarray(off, dtype=np.uint64))
    st = None if starts is None else dev(t, np.asarray(starts, dtype=np.uint64))
    v_in = None
    if values is not None and "values" in want:
        v_in = dev(t, np.concatenate([np.full(shifts[0] * vb, 0x5A, dtype=np.uint8), values.view(np.uint8), np.full(GUARD, 0xA5, dtype=np.uint8)]))
        assert v_in.data_ptr() % 16 == 0
    bufs = {}
    for k, name in enumerate(OUTPUTS):
        if name in want and (name != "values" or values is not None):
            eb = vb if name == "values" else 4
            bufs[name] = banded(t, n * eb, shifts[k + 1] * eb) + (eb,)
            assert bufs[name][0].data_ptr() % 16 == 0 and GUARD % 16 == 0
    ptr = lambda name: bufs[name][0].data_ptr() + bufs[name][1] if name in bufs else None
    if eng is None:
        eng = engine(rsx)
    eng.segmented_expand(None if v_in is None else v_in.data_ptr() + shifts[0] * vb, 0 if values is None else values.size, vb, o.data_ptr(), nseg, n,
                         None if st is None else st.data_ptr(), ptr("values"), ptr("segment"), ptr("rank"))
    if sync:
        t.cuda.synchronize()      # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    out = {name: unband(buf, pre, n * eb, name).view(UWORD[eb]) for name, (buf, pre, eb) in bufs.items()}
    return out, eng


def check(out, off, n, values=None, starts=None, what=""):
    vout, sout, rout, _ = expand_oracle(off, n, values, starts)
    for name, ref in (("values", vout), ("segment", sout), ("rank", rout)):
        if name not in out:
            continue
        bad = np.flatnonzero(out[name] != ref)
        assert bad.size == 0, f"{what} {name}: positions {bad[:8].tolist()} (of {bad.size}): {out[name][bad[:8]].tolist()} != {ref[bad[:8]].tolist()}"


def words(rng, count, vb):
    return rng.integers(0, 1 << (8 * vb), count, dtype=UWORD[vb], endpoint=False)


def random_starts(rng, off, num_values):
    lens = np.diff(np.asarray(off).astype(np.int64))
    return np.array([rng.integers(0, num_values - k + 1) for k in lens], dtype=np.uint64)


def both_forms(rsx, off, n, rng, eng, what, vbs=(4, 8), **kw):
    """the fill form and the gather form, all three outputs, for the value widths"""
    nseg = len(off) - 1
    for vb in vbs:
        vals = words(rng, nseg, vb)
        out, _ = run(rsx, off, n, vals, eng=eng, **kw)
        check(out, off, n, vals, what=f"{what} fill {vb}")
        longest = int(np.diff(np.asarray(off).astype(np.int64)).max()) if nseg else 0
        src = words(rng, longest + 37, vb)
        starts = random_starts(rng, off, src.size)
        out, _ = run(rsx, off, n, src, starts, eng=eng, **kw)
        check(out, off, n, src, starts, what=f"{what} gather {vb}")


# -- layouts ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_layouts(rsx, name):
    rng = np.random.default_rng(len(name))
    n, off = R.LAYOUTS[name][0]()
    eng = engine(rsx)
    both_forms(rsx, off, n, rng, eng, name)
    eng.sync()


@pytest.mark.parametrize("name", list(R.BIG_LAYOUTS))
def test_big_layouts(rsx, name):
    """2^24 + 4099 elements in 4099 segments (two tiles per workgroup); 2^20 + 4099 segments, mostly empty"""
    rng = np.random.default_rng(4)
    n, off = R.BIG_LAYOUTS[name][0]()
    eng = engine(rsx)
    both_forms(rsx, off, n, rng, eng, name, vbs=(4,) if name == "multi tile" else (8,))
    eng.sync()


def test_nothing_to_do(rsx):
    """n == 0 and S == 0 launch nothing; all segments empty writes nothing"""
    t = _torch()
    eng = engine(rsx)
    vals = np.arange(3, dtype=np.uint32)
    out, _ = run(rsx, np.zeros(4, dtype=np.uint64), 0, vals, eng=eng)
    assert all(v.size == 0 for v in out.values())
    out, _ = run(rsx, np.array([7], dtype=np.uint64), 100, np.zeros(0, dtype=np.uint32), want=("segment", "rank"), eng=eng)
    assert all(np.all(v == 0xC3C3C3C3) for v in out.values())
    buf = t.full((64,), -7, dtype=t.int32, device="cuda")
    eng.segmented_expand(None, 0, 4, None, 0, 64, None, None, buf.data_ptr(), None)          # S == 0: not even the offsets are needed
    out, _ = run(rsx, np.array([5, 5, 5], dtype=np.uint64), 100, vals[:2], eng=eng)
    assert all(np.all(v == 0xC3C3C3C3) for v in out.values())
    eng.sync()
    assert bool((buf == -7).all())


# -- pointers off 16-byte alignment -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vb", [4, 8])
def test_misaligned_pointers(rsx, vb):
    """every input and output 1, 2 and 3 elements past a 16-byte boundary, together and one at a time, on ragged ends inside tiles"""
    rng = np.random.default_rng(12 + vb)
    n, off = R.layout_ragged_ends()
    nseg = len(off) - 1
    vals = words(rng, nseg, vb)
    src = words(rng, 5000, vb)
    starts = random_starts(rng, off, src.size) | np.uint64(1)     # odd starts
    starts = np.minimum(starts, (src.size - np.diff(off.astype(np.int64))).astype(np.uint64))
    eng = engine(rsx)
    for shifts in ((1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 1, 2, 3), (3, 2, 1, 0), (1, 0, 0, 0), (0, 3, 0, 0), (0, 0, 1, 0), (0, 0, 0, 2)):
        out, _ = run(rsx, off, n, vals, eng=eng, shifts=shifts)
        check(out, off, n, vals, what=f"fill {shifts}")
        out, _ = run(rsx, off, n, src, starts, eng=eng, shifts=shifts)
        check(out, off, n, src, starts, what=f"gather {shifts}")
    n2, off2 = R.layout_one(3 * TILE + 5)                          # the pure fill path
    for shifts in ((1, 1, 1, 1), (0, 3, 2, 1)):
        out, _ = run(rsx, off2, n2, vals[:1], eng=eng, shifts=shifts)
        check(out, off2, n2, vals[:1], what=f"fill tiles {shifts}")
        src2 = words(rng, n2 + 9, vb)
        out, _ = run(rsx, off2, n2, src2, [3], eng=eng, shifts=shifts)
        check(out, off2, n2, src2, [3], what=f"gather tiles {shifts}")
    eng.sync()


# -- outputs and forms --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gather", [False, True], ids=["fill", "gather"])
def test_every_subset_of_the_outputs(rsx, gather):
    rng = np.random.default_rng(31)
    n, off = R.layout_zipf(total=1 << 15, seed=8)
    nseg = len(off) - 1
    eng = engine(rsx)
    for vb in (4, 8):
        vals = words(rng, 30000 if gather else nseg, vb)
        starts = random_starts(rng, off, vals.size) if gather else None
        for r in (1, 2, 3):
            for want in itertools.combinations(OUTPUTS, r):
                out, _ = run(rsx, off, n, vals, starts, want=want, eng=eng)
                assert set(out) == set(want)
                check(out, off, n, vals, starts, what=str(want))
    eng.sync()


def test_gather_starts_overlap_descend_and_are_odd(rsx):
    rng = np.random.default_rng(41)
    lens = [5000, 3, 0, 4097, 1, 0, 0, 777, 4096, 2]
    off = offsets_from(lens, start=2)
    n = int(off[-1]) + 1
    eng = engine(rsx)
    for vb in (4, 8):
        src = words(rng, 6001, vb)
        cases = {"overlapping": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9], "descending": [1001, 900, 800, 700, 600, 500, 400, 300, 200, 100],
                 "odd": [1, 5997, 6001, 1903, 5999, 3, 6001, 5223, 1905, 5999], "same": [77] * 10, "to the end": [6001 - k for k in lens]}
        for name, starts in cases.items():
            assert R.valid(off, n, starts, src.size) is None
            out, _ = run(rsx, off, n, src, starts, eng=eng)
            check(out, off, n, src, starts, what=name)
    eng.sync()


# -- round trips through the engine -------------------------------------------------------------------------------------------------------

def test_expand_undoes_run_length_encoding(rsx):
    """expand of segmented_unique(consecutive)'s keys and run offsets gives the input back bit for bit"""
    t = _torch()
    rng = np.random.default_rng(51)
    n = 3 * TILE + 123
    for dt in (np.uint32, np.uint64):
        x = np.repeat(words(rng, 400, np.dtype(dt).itemsize) >> np.array(3, dtype=dt), rng.integers(1, 60, 400))[:n]
        n = x.size
        xd = dev(t, x)
        keys = t.zeros(n, dtype=xd.dtype, device="cuda")
        runoff = t.zeros(2, dtype=t.int64, device="cuda")
        counts = t.zeros(n, dtype=t.int32, device="cuda")
        eng = engine(rsx, dtype=dt, capacity=n)
        eng.segmented_unique(xd.data_ptr(), n, None, 1, keys.data_ptr(), runoff.data_ptr(), counts.data_ptr(), None, None, consecutive=True)
        eng.sync()
        runs = int(runoff[1])
        assert 300 < runs <= 400
        off = t.zeros(runs + 1, dtype=t.int64, device="cuda")
        off[1:] = t.cumsum(counts[:runs].to(t.int64), 0)
        back = t.full((n,), -1, dtype=xd.dtype, device="cuda")
        eng.segmented_expand(keys.data_ptr(), runs, x.dtype.itemsize, off.data_ptr(), runs, n, None, back.data_ptr(), None, None)
        eng.sync()
        assert t.equal(back, xd)
        assert t.equal(rsx.repeat_interleave(keys[:runs], counts[:runs].to(t.int64), output_size=n), xd)


def test_segment_ids_then_bincount_gives_the_lengths(rsx):
    t = _torch()
    n, off_h = R.layout_zipf(total=1 << 16, seed=3)
    off = dev(t, off_h)
    ids = rsx.segment_ids(off - int(off_h[0]), n=int(off_h[-1] - off_h[0]))
    assert ids.dtype == t.int64
    got = rsx.bincount(ids.to(t.int32), num_bins=len(off_h) - 1)
    assert t.equal(got, off[1:] - off[:-1])
    assert t.equal(rsx.segment_ids(off - int(off_h[0])), ids)                     # n read back from offsets[-1]
    rk = rsx.segment_ranks(off, n=n)
    seg, rank = R.owners(off_h)
    assert np.array_equal(rk.cpu().numpy()[int(off_h[0]):int(off_h[-1])], rank) and int(rk[:int(off_h[0])].abs().sum()) == 0


def test_broadcast_of_segment_max_equals_the_scan_at_the_last_element(rsx):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(9)
    lens = [1, 0, 5000, 17, 0, 4096, 300, 1, 0]
    off_h = offsets_from(lens)
    off = dev(t, off_h)
    n = int(off_h[-1])
    for dt in (t.float32, t.int64, t.float64, t.int32):
        v = (t.randn(n, device="cuda", generator=g, dtype=t.float64) * 1000).to(dt)
        spread = rsx.broadcast_segments(rsx.segmented_reduce(v, off, "max"), off, n=n)
        running = rsx.segmented_scan(v, off, "max")
        seg, rank = R.owners(off_h)
        last = t.from_numpy(off_h.astype(np.int64)[1:][seg] - 1).cuda()
        assert spread.dtype == dt and t.equal(spread, running[last])


# -- bad input --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", ["decreasing", "past_n", "start"])
def test_bad_input_writes_nothing_and_is_reported_once(rsx, bad):
    rng = np.random.default_rng(23)
    n = 40000
    off = np.array([0, 100, 5000, 4000 if bad == "decreasing" else (n + 1 if bad == "past_n" else 9000), n, n], dtype=np.uint64)      # segment 2 is the first bad one
    src = words(rng, n, 4)
    starts = np.array([0, 0, n - 3999 if bad == "start" else 0, 0, n + 1 if bad == "start" else 0], dtype=np.uint64)
    vals = words(rng, 5, 4)
    eng = engine(rsx)
    if bad == "start":
        assert R.valid(off, n) is None and R.valid(off, n, starts, n) == 2
        out, _ = run(rsx, off, n, src, starts, eng=eng)
    else:
        assert R.valid(off, n) == 2
        out, _ = run(rsx, off, n, vals, eng=eng)
    assert all(np.all(v == 0xC3C3C3C3) for v in out.values()), "a call with bad input wrote something"
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "rsx_segmented_expand" in str(ei.value) and "segment 2 " in str(ei.value)
    eng.sync()                                                     # reported once
    good = np.array([0, 3, 5000, 5001, 30000, n], dtype=np.uint64)
    out, _ = run(rsx, good, n, vals, eng=eng)                      # the engine stays usable
    check(out, good, n, vals, what="after bad input")
    if bad == "start":                                             # the same offsets with starts that fit, and without starts
        out, _ = run(rsx, off, n, src, np.array([0, 0, n - 4000, 0, n], dtype=np.uint64), eng=eng)
        check(out, off, n, src, [0, 0, n - 4000, 0, n], what="starts that just fit")
    eng.sync()


# -- streams, engines, capture ------------------------------------------------------------------------------------------------------------

def test_streams_engines_and_sort_state(rsx):
    """equal input, equal bits: twice on one engine, engines of another capacity, key kind and payload, a side stream; n far above the
    capacity; and the sort result of the engine stays"""
    t = _torch()
    rng = np.random.default_rng(99)
    n, off = R.layout_zipf(total=1 << 17, seed=11)
    vals = words(rng, len(off) - 1, 8)
    eng = engine(rsx)
    x = rng.integers(0, 1 << 32, CAP, dtype=np.uint32)
    eng.upload(x)
    eng.sort()
    a, _ = run(rsx, off, n, vals, eng=eng)
    check(a, off, n, vals, what="first")
    b, _ = run(rsx, off, n, vals, eng=eng)
    c, _ = run(rsx, off, n, vals, eng=engine(rsx, capacity=1 << 20, dtype=np.float64, payload=True))
    side = t.cuda.Stream()
    d, eng2 = run(rsx, off, n, vals, eng=engine(rsx, stream=side.cuda_stream, dtype=np.int64))
    eng2.sync()
    for other, what in ((b, "second call"), (c, "float64 payload engine of another capacity"), (d, "side stream")):
        assert all(np.array_equal(a[k], other[k]) for k in OUTPUTS), what
    assert n > 30 * CAP and eng.geometry().num_keys == CAP
    assert np.array_equal(eng.download(), np.sort(x))


def test_capture_and_replay(rsx):
    """one captured call (one linear stream) is replayed twice after values, starts and offsets were changed in place"""
    t = _torch()
    rng = np.random.default_rng(70)
    lens = [5, 0, 4096, 1, 700, 0, 0, 4500, 33, 2]
    nseg = len(lens)
    n = sum(lens) + 9
    side = t.cuda.Stream()
    eng = engine(rsx, stream=side.cuda_stream)
    off = offsets_from(lens, start=4)
    src = words(rng, 6000, 8)
    starts = random_starts(rng, off, src.size)
    od, sd, vd = dev(t, off), dev(t, starts), dev(t, src)
    outs = [dev(t, np.full(n * eb, FILL, dtype=np.uint8)) for eb in (8, 4, 4)]

    def call():
        eng.segmented_expand(vd.data_ptr(), src.size, 8, od.data_ptr(), nseg, n, sd.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())

    def result():
        return {"values": outs[0].cpu().numpy().view(np.uint64), "segment": outs[1].cpu().numpy().view(np.uint32), "rank": outs[2].cpu().numpy().view(np.uint32)}

    call()                                                         # eager: sizes the scratch of this n
    eng.sync()
    check(result(), off, n, src, starts, what="eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for rep in range(2):
        off = offsets_from([int(v) for v in rng.permutation(lens)], start=rep)      # same segment count, ends within n
        src = words(rng, 6000, 8)
        starts = random_starts(rng, off, src.size)
        vd.copy_(t.from_numpy(src.view(np.int64)))
        od.copy_(t.from_numpy(off.view(np.int64)))
        sd.copy_(t.from_numpy(starts.view(np.int64)))
        for o in outs:
            o.fill_(FILL - 256)
        t.cuda.synchronize()
        graph.replay()
        t.cuda.synchronize()
        check(result(), off, n, src, starts, what=f"replay {rep}")
    del graph
    eng.sync()


# -- the argument rules -------------------------------------------------------------------------------------------------------------------

def test_refusals(rsx):
    """every argument rule of the contract, one change at a time from a valid call, with the message"""
    t = _torch()
    n = 3 * TILE
    eng = rsx.Engine(np.uint32, n, payload=True)
    vals = t.ones(2 * n + 4, dtype=t.int32, device="cuda")
    vout = t.full((n + 4,), -7, dtype=t.int32, device="cuda")
    sout = t.full((n + 4,), -7, dtype=t.int32, device="cuda")
    rout = t.full((n + 4,), -7, dtype=t.int32, device="cuda")
    off = t.tensor([0, n, n, n], dtype=t.int64, device="cuda")
    starts = t.tensor([0, 5, 5, 0], dtype=t.int64, device="cuda")
    lib = rsx.load_library()
    P = C.c_void_p
    p = lambda x: None if x is None else P(x)
    base = dict(e=eng._h, d_values=vals.data_ptr(), num_values=3, value_bytes=4, d_offsets=off.data_ptr(), num_segments=3, n=n, d_starts=None, flags=0,
                d_values_out=vout.data_ptr(), d_segment_out=sout.data_ptr(), d_rank_out=rout.data_ptr())

    def call(**kw):
        a = {**base, **kw}
        return lib.rsx_segmented_expand(a["e"], p(a["d_values"]), a["num_values"], a["value_bytes"], p(a["d_offsets"]), a["num_segments"], a["n"],
                                        p(a["d_starts"]), a["flags"], p(a["d_values_out"]), p(a["d_segment_out"]), p(a["d_rank_out"]))

    gather = dict(flags=rsx.EXPAND_GATHER, d_starts=starts.data_ptr(), num_values=2 * n)
    refused = [
        (4, "null engine", dict(e=None)),
        (4, "unknown flag bits", dict(flags=1)), (4, "unknown flag bits", dict(flags=32)), (4, "unknown flag bits", dict(flags=128)),
        (4, "unknown flag bits", {**gather, "flags": 64 | (1 << 31)}),
        (4, "value_bytes must be 4 or 8", dict(value_bytes=2)), (4, "value_bytes must be 4 or 8", dict(value_bytes=0)), (4, "value_bytes must be 4 or 8", dict(value_bytes=16)),
        (4, "d_starts must be given if and only if", dict(flags=rsx.EXPAND_GATHER)), (4, "d_starts must be given if and only if", dict(d_starts=starts.data_ptr())),
        (4, "both be NULL or both be given", dict(d_values=None)), (4, "both be NULL or both be given", dict(d_values_out=None)),
        (4, "at least one output", dict(d_values=None, d_values_out=None, d_segment_out=None, d_rank_out=None)),
        (4, "num_values must equal num_segments", dict(num_values=2)), (4, "num_values must equal num_segments", dict(num_values=4)),
        (4, "at most 2^32 - 2 segments", dict(num_segments=0xFFFFFFFF, num_values=0xFFFFFFFF)),
        (4, "at most 2^31 elements", dict(n=(1 << 31) + 1)),
        (1, "offsets must be", dict(d_offsets=None)), (1, "offsets must be", dict(d_offsets=off.data_ptr() + 4)),
        (1, "starts must be", {**gather, "d_starts": starts.data_ptr() + 4}),
        (1, "aligned to the value size", dict(d_values=vals.data_ptr() + 2)), (1, "aligned to the value size", dict(d_values_out=vout.data_ptr() + 2)),
        (1, "aligned to the value size", dict(value_bytes=8, d_values=vals.data_ptr() + 4)), (1, "aligned to the value size", dict(value_bytes=8, d_values_out=vout.data_ptr() + 4)),
        (1, "4-byte aligned", dict(d_segment_out=sout.data_ptr() + 2)), (1, "4-byte aligned", dict(d_rank_out=rout.data_ptr() + 1)),
        (1, "two outputs overlap", dict(d_rank_out=sout.data_ptr() + 4 * (n - 1))), (1, "two outputs overlap", dict(d_segment_out=vout.data_ptr())),
        (1, "an output overlaps an input", dict(d_values_out=vals.data_ptr() + 8)), (1, "an output overlaps an input", dict(d_segment_out=off.data_ptr())),
        (1, "an output overlaps an input", {**gather, "d_rank_out": starts.data_ptr()}),
        (1, "an output overlaps an input", {**gather, "d_values_out": vals.data_ptr() + 4 * (2 * n - 1)}),
        (1, "the engine's own buffers", dict(d_values_out=eng.result_device()[0])), (1, "the engine's own buffers", dict(d_values=eng.result_device()[0])),
        (1, "the engine's own buffers", dict(d_segment_out=eng.result_device()[1])),
    ]
    for status, text, kw in refused:
        assert call(**kw) == status, kw
        msg = lib.rsx_last_error().decode()
        assert msg.startswith("rsx_segmented_expand: ") and text in msg, (kw, msg)
    assert call(num_segments=0, num_values=0) == 0 and call(n=0) == 0                # nothing to do: nothing is launched
    eng.sync()
    assert all(bool((b == -7).all()) for b in (vout, sout, rout)), "a refused call wrote something"
    assert call() == 0                                                           # and the call these were variations of works,
    eng.sync()
    assert bool((vout[:n] == 1).all()) and bool((sout[:n] == 0).all()) and rout[:n].tolist() == list(range(n))
    assert all(bool((b[n:] == -7).all()) for b in (vout, sout, rout))
    assert call(**gather) == 0                                                   # in gather form,
    assert call(d_values=None, d_values_out=None, d_rank_out=None) == 0          # with one output and no values,
    assert call(**{**gather, "d_values": None, "d_values_out": None}) == 0       # and with starts that are only checked
    eng.sync()
    with pytest.raises(rsx.RadixSortError) as ei:                                # the Engine method carries the same text
        eng.segmented_expand(None, 0, 4, off.data_ptr(), 3, n)
    assert "at least one output" in str(ei.value)


# -- the torch helpers ------------------------------------------------------------------------------------------------------------------

def test_repeat_interleave_matches_torch(rsx):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(5)
    rep = t.randint(0, 9, (700,), device="cuda", generator=g)
    rep[100] = 5000
    total = int(rep.sum())
    assert t.equal(rsx.repeat_interleave(rep), t.repeat_interleave(rep))                                   # form 1
    assert t.equal(rsx.repeat_interleave(rep, output_size=total), t.repeat_interleave(rep, output_size=total))
    assert t.equal(rsx.repeat_interleave(rep.to(t.int32)), t.repeat_interleave(rep.to(t.int32)))
    for dt in (t.float32, t.int64, t.float64, t.bfloat16, t.bool):
        x = (t.randn(700, device="cuda", generator=g) * 100).to(dt)
        for kw in ({}, {"output_size": total}):
            got = rsx.repeat_interleave(x, rep, **kw)
            assert got.dtype == dt and t.equal(got, t.repeat_interleave(x, rep, **kw)), (dt, kw)           # form 3
        got = rsx.repeat_interleave(x, 3)
        assert t.equal(got, t.repeat_interleave(x, 3)) and t.equal(rsx.repeat_interleave(x, 3, output_size=2100), got)      # form 2
        assert rsx.repeat_interleave(x, 0).numel() == 0
        y = (t.randn(5, 700, device="cuda", generator=g) * 100).to(dt)                                 # 2-D
        assert t.equal(rsx.repeat_interleave(y, 2), t.repeat_interleave(y, 2))                             # flattened
        assert t.equal(rsx.repeat_interleave(y, rep, dim=1), t.repeat_interleave(y, rep, dim=1))
        assert t.equal(rsx.repeat_interleave(y, rep, dim=-1, output_size=total), t.repeat_interleave(y, rep, dim=1, output_size=total))
        assert t.equal(rsx.repeat_interleave(y, 3, dim=0), t.repeat_interleave(y, 3, dim=0))
        assert t.equal(rsx.repeat_interleave(y.t(), rep[:5], dim=1), t.repeat_interleave(y.t(), rep[:5], dim=1))      # non-contiguous
    with pytest.raises(ValueError):
        rsx.repeat_interleave(x, rep[:10])
    bad = rep.clone()
    bad[3] = -2                                                                                            # negative repeats: bad offsets
    with pytest.raises(rsx.RadixSortError) as ei:
        rsx.repeat_interleave(x.float(), bad, output_size=total)
        t.cuda.synchronize()
        rsx.segment_ids(t.tensor([0, 4], device="cuda"), n=4)                                              # ... reported at the next call
    assert "rsx_segmented_expand" in str(ei.value)


def test_pack_rows_and_gather_ranges(rsx):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(6)
    B, W = 300, 70
    for dt in (t.float32, t.int64, t.float16):
        x = (t.randn(B, W, device="cuda", generator=g) * 100).to(dt)
        lengths = t.randint(0, W + 1, (B,), device="cuda", generator=g)
        lengths[7], lengths[8] = 0, W
        vals, off = rsx.pack_rows(x, lengths)
        mask = t.arange(W, device="cuda")[None, :] < lengths[:, None]
        assert t.equal(vals, x[mask]) and t.equal(off[1:], t.cumsum(lengths, 0)) and int(off[0]) == 0
        src = (t.randn(5000, device="cuda", generator=g) * 100).to(dt)
        starts = t.randint(0, 4000, (40,), device="cuda", generator=g)
        lens = t.randint(0, 1000, (40,), device="cuda", generator=g)
        lens[5] = 0
        got, goff = rsx.gather_ranges(src, starts, lens)
        want = t.cat([src[int(a):int(a) + int(k)] for a, k in zip(starts.tolist(), lens.tolist())])
        assert t.equal(got, want) and goff.tolist() == [0] + np.cumsum(lens.tolist()).tolist()
    with pytest.raises(rsx.RadixSortError):                                                                # a slice that runs off the end
        rsx.gather_ranges(src, t.tensor([4999], device="cuda"), t.tensor([2], device="cuda"))
        t.cuda.synchronize()
        rsx.segment_ids(t.tensor([0, 4], device="cuda"), n=4)


def test_segmented_expand_helper_and_no_synchronisation_when_sizes_are_given(rsx):
    """the helpers run on the current stream and, with n / output_size given, read nothing back: they can be captured in a graph"""
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(7)
    lens = [3, 0, 4097, 1, 0, 250]
    off_h = offsets_from(lens, start=2)
    n = int(off_h[-1]) + 3
    seg, rank = R.owners(off_h)
    off = dev(t, off_h)
    v = t.randn(len(lens), device="cuda", generator=g)
    vals, ids, rk = rsx.segmented_expand(off, v, n=n, return_segment=True, return_rank=True)
    lo, hi = int(off_h[0]), int(off_h[-1])
    assert t.equal(vals[lo:hi], v[t.from_numpy(seg).cuda()]) and np.array_equal(ids.cpu().numpy()[lo:hi], seg) and np.array_equal(rk.cpu().numpy()[lo:hi], rank)
    assert float(vals[:lo].abs().sum()) == 0 and float(vals[hi:].abs().sum()) == 0 and vals.numel() == n
    assert t.equal(rsx.segmented_expand(off, v), vals[:hi])                                                # n read back
    rows = t.randn(len(lens), 3, device="cuda", generator=g).to(t.bfloat16)                                 # rows per segment: index_select
    assert t.equal(rsx.broadcast_segments(rows, off - lo, n=hi - lo), rows[t.from_numpy(seg).cuda()])
    src = t.randn(9000, device="cuda", generator=g, dtype=t.float64)
    starts = t.tensor([5, 4, 3, 2, 1, 0], device="cuda")
    got = rsx.segmented_expand(off, src, n=n, starts=starts)
    assert t.equal(got[lo:hi], src[starts[t.from_numpy(seg).cuda()] + t.from_numpy(rank).cuda()])

    side = t.cuda.Stream()
    rep = t.tensor(lens, device="cuda")
    x = t.randn(len(lens), device="cuda", generator=g)
    total = sum(lens)
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        rsx.repeat_interleave(x, rep, output_size=total)                                                   # eager on this stream: sizes its engine's scratch
        rsx.segment_ids(off, n=n)
    side.synchronize()
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):                                                                 # a read-back would fail the capture
        y = rsx.repeat_interleave(x, rep, output_size=total)
        ids2 = rsx.segment_ids(off, n=n)
    for k in range(2):
        x.copy_(t.randn(len(lens), device="cuda", generator=g))
        rep.copy_(t.tensor(lens[k:] + lens[:k], device="cuda"))
        t.cuda.synchronize()
        graph.replay()
        t.cuda.synchronize()
        assert t.equal(y, t.repeat_interleave(x, rep)) and t.equal(ids2, ids)
    del graph
