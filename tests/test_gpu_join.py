"""Segmented join (rsx_segmented_join, radix_sort_amd.segmented_join / join_sorted / isin_sorted) on the GPU.

The referee is tests/_join_ref.py (np.searchsorted, np.repeat).  Every comparison is exact: indices, offsets and key bits.  The row buffers
start out holding a sentinel and lie between guard bands, so that a row at or past min(P, out_capacity) that was written shows.  Every
engine here has capacity 4096: the call is not bound by it.  The layouts are the smallest that reach each path of the kernels;
tests/test_join.py proves from the data alone that they do.
"""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest

import _join_ref as R
from _join_ref import ANTI, INNER, LEFT, SEMI, TILE
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, GUARD

pytestmark = pytest.mark.gpu

CAP = 4096
UWORD = {4: np.uint32, 8: np.uint64}
OUTPUTS = ("keys", "ia", "ib")
SENT32 = 0xC3C3C3C3
NONE32 = 0xFFFFFFFF


def engine(rsx, dtype, stream=None, **kw):
    eng = rsx.Engine(dtype, CAP, **kw)
    if stream is not None:
        eng.set_stream(stream)
    return eng


def banded(t, nbytes, shift_bytes):
    pre = GUARD + shift_bytes
    return dev(t, np.concatenate([np.full(pre, 0x5A, dtype=np.uint8), np.full(nbytes, FILL, dtype=np.uint8), np.full(GUARD, 0xA5, dtype=np.uint8)])), pre


def unband(buf, pre, nbytes, what):
    b = buf.cpu().numpy().view(np.uint8)
    assert np.all(b[:pre] == 0x5A), f"{what}: bytes before the output written"
    assert np.all(b[pre + nbytes:] == 0xA5), f"{what}: guard band written"
    return b[pre:pre + nbytes].copy()


def run(rsx, a, aoff, b, boff, op, cap=None, want=OUTPUTS, eng=None, shifts=(0, 0, 0), descending=False, rows=None, sync=True, **engine_kw):
    """One rsx_segmented_join through the Engine API.  cap: out_capacity (None: the true total, from the referee); rows: elements of each
    row buffer (default cap).  shifts: the three outputs lie that many ELEMENTS past a 16-byte aligned address.  want == (): count only.
    Returns ({name: host array of `rows` words}, out_offsets, engine)."""
    t = _torch()
    kb = a.dtype.itemsize
    nseg = 1 if aoff is None else len(aoff) - 1
    if cap is None:
        cap = int(R.join_oracle(a, aoff, b, boff, op, descending)[3][-1])
    rows = cap if rows is None else rows
    want = tuple(w for w in want if not (w == "ib" and op == ANTI))
    da, db = dev(t, a), dev(t, b)
    dao, dbo = (None, None) if aoff is None else (dev(t, np.asarray(aoff, dtype=np.uint64)), dev(t, np.asarray(boff, dtype=np.uint64)))
    ooff = dev(t, np.full(nseg + 1, 0xC3C3C3C3C3C3C3C3, dtype=np.uint64))
    bufs = {}
    for k, name in enumerate(OUTPUTS):
        if name in want:
            eb = kb if name == "keys" else 4
            bufs[name] = banded(t, rows * eb, shifts[k] * eb) + (eb,)
            assert bufs[name][0].data_ptr() % 16 == 0 and GUARD % 16 == 0
    ptr = lambda name: bufs[name][0].data_ptr() + bufs[name][1] if name in bufs else None
    if eng is None:
        eng = engine(rsx, a.dtype, descending=descending, **engine_kw)
    eng.segmented_join(da.data_ptr() if a.size else None, a.size, None if dao is None else dao.data_ptr(), db.data_ptr() if b.size else None, b.size,
                       None if dbo is None else dbo.data_ptr(), nseg, op, cap, ooff.data_ptr(), d_a_index_out=ptr("ia"), d_b_index_out=ptr("ib"),
                       d_keys_out=ptr("keys"))
    if sync:
        t.cuda.synchronize()      # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    out = {name: unband(buf, pre, rows * eb, name).view(UWORD[eb]) for name, (buf, pre, eb) in bufs.items()}
    return out, ooff.cpu().numpy().view(np.uint64), eng


def reference(a, aoff, b, boff, op, descending=False):
    ia, ib, keys, ooff = R.join_oracle(a, aoff, b, boff, op, descending)
    return {"ia": ia.astype(np.uint32), "ib": np.where(ib < 0, NONE32, ib).astype(np.uint32), "keys": keys.view(UWORD[a.dtype.itemsize])}, ooff


def check(out, ooff, ref, ref_off, cap=None, what=""):
    """the offsets are the true ones; rows below min(P, cap) are the referee's; everything behind still holds the sentinel"""
    assert np.array_equal(ooff, ref_off), f"{what} offsets: {ooff[:6].tolist()} != {ref_off[:6].tolist()}"
    P = int(ref_off[-1])
    w = P if cap is None else min(P, cap)
    for name, got in out.items():
        bad = np.flatnonzero(got[:w] != ref[name][:w])
        assert bad.size == 0, f"{what} {name}: rows {bad[:8].tolist()} (of {bad.size}): {got[bad[:8]].tolist()} != {ref[name][bad[:8]].tolist()}"
        sent = np.frombuffer(bytes([FILL]) * got.dtype.itemsize, dtype=got.dtype)[0]
        assert np.all(got[w:] == sent), f"{what} {name}: a row at or past min(P, capacity) = {w} was written"


def run_and_check(rsx, a, aoff, b, boff, op, what, descending=False, extra=5, **kw):
    ref, ref_off = reference(a, aoff, b, boff, op, descending)
    P = int(ref_off[-1])
    out, ooff, eng = run(rsx, a, aoff, b, boff, op, cap=P + extra, descending=descending, **kw)
    check(out, ooff, ref, ref_off, P + extra, what)
    return eng


# -- the matrix ---------------------------------------------------------------------------------------------------------------------------

RAGGED = R.layout_ragged()


@pytest.mark.parametrize("how", list(R.KINDS))
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_matrix(rsx, dtype, descending, how):
    a, aoff, b, boff = R.typed(*RAGGED, dtype, descending)
    run_and_check(rsx, a, aoff, b, boff, R.KINDS[how], f"{dtype} {descending} {how}", descending).sync()


@pytest.mark.parametrize("shape", [(5000, 3), (3, 10000), (4096, 1), (1, 8193), (4097, 4097)])
def test_all_keys_equal(rsx, shape):
    a, _, b, _ = R.layout_all_equal(*shape)
    kinds = (INNER,) if shape == (4097, 4097) else (INNER, LEFT, SEMI, ANTI)
    for op in kinds:
        run_and_check(rsx, a, None, b, None, op, f"{shape} {op}").sync()


@pytest.mark.parametrize("P", R.TOTALS)
def test_tile_edge_totals(rsx, P):
    a, _, b, _ = R.layout_total(P)
    for op in (INNER, SEMI):
        run_and_check(rsx, a, None, b, None, op, f"P={P} {op}").sync()


@pytest.mark.parametrize("na", R.ONE_PARTNER)
def test_tile_edge_sizes_with_one_partner_each(rsx, na):
    a, _, b, _ = R.layout_one_partner(na)
    for op in (INNER, LEFT, ANTI):
        run_and_check(rsx, a, None, b, None, op, f"na={na} {op}").sync()
    run_and_check(rsx, a.astype(np.uint64), None, b.astype(np.uint64), None, INNER, f"na={na} uint64").sync()


@pytest.mark.parametrize("how", ["inner", "left"])
def test_sparse_matches(rsx, how):
    a, _, b, _ = R.layout_sparse()
    run_and_check(rsx, a, None, b, None, R.KINDS[how], "sparse " + how).sync()


@pytest.mark.parametrize("name", ["many segments", "zipf"])
def test_many_segments(rsx, name):
    a, aoff, b, boff = R.LAYOUTS[name][0]()
    for op in (INNER, LEFT):
        run_and_check(rsx, a, aoff, b, boff, op, f"{name} {op}").sync()
    a64, b64 = a.astype(np.int64) - 20, b.astype(np.int64) - 20
    run_and_check(rsx, a64, aoff, b64, boff, SEMI, f"{name} int64 semi").sync()


def test_empty_sides(rsx):
    """na == 0: zero offsets, no rows; nb == 0: INNER and SEMI nothing, LEFT and ANTI every A row"""
    z = np.zeros(0, dtype=np.uint32)
    a = np.arange(5000, dtype=np.uint32)
    for op in (INNER, LEFT, SEMI, ANTI):
        out, ooff, eng = run(rsx, z, None, a, None, op, cap=16)
        assert ooff.tolist() == [0, 0] and all(np.all(v == SENT32) for v in out.values())
        eng.sync()
        eng = run_and_check(rsx, a, None, z, None, op, f"nb == 0 {op}")
        eng.sync()
        off = np.array([0, 0, 5000, 5000], dtype=np.uint64)
        run_and_check(rsx, a, off, z, np.zeros(4, dtype=np.uint64), op, f"nb == 0 segments {op}").sync()


# -- 64-bit counting ----------------------------------------------------------------------------------------------------------------------

def test_64_bit_counting(rsx):
    a, b = np.full(65537, 9, dtype=np.uint32), np.full(65536, 9, dtype=np.uint32)
    big = (1 << 32) + 65536
    out, ooff, eng = run(rsx, a, None, b, None, INNER, cap=0, want=())                    # count only
    assert ooff.tolist() == [0, big]
    out, ooff, _ = run(rsx, a, None, b, None, INNER, cap=8192, rows=8192 + 100, eng=eng)
    assert ooff.tolist() == [0, big]
    assert np.all(out["ia"][:8192] == 0) and np.array_equal(out["ib"][:8192], np.arange(8192)) and np.all(out["keys"][:8192] == 9)
    assert all(np.all(v[8192:] == SENT32) for v in out.values())
    a2, b2 = np.concatenate([a, a]), np.concatenate([b, b])
    aoff, boff = np.array([0, 65537, 2 * 65537], dtype=np.uint64), np.array([0, 65536, 2 * 65536], dtype=np.uint64)
    out, ooff, _ = run(rsx, a2, aoff, b2, boff, INNER, cap=0, want=(), eng=eng)
    assert ooff.tolist() == [0, big, 2 * big]
    eng.sync()


# -- capacity, output selection, alignment ------------------------------------------------------------------------------------------------

def test_capacity(rsx):
    a, aoff, b, boff = R.layout_many_segments()
    for op in (INNER, LEFT):
        ref, ref_off = reference(a, aoff, b, boff, op)
        P = int(ref_off[-1])
        eng = engine(rsx, a.dtype)
        out, counted, _ = run(rsx, a, aoff, b, boff, op, cap=0, want=(), eng=eng)
        assert np.array_equal(counted, ref_off)
        for cap in (P, P - 1, 1, P + TILE + 3):
            out, ooff, _ = run(rsx, a, aoff, b, boff, op, cap=cap, rows=max(cap, P) + 7, eng=eng)
            check(out, ooff, ref, ref_off, cap, f"{op} capacity {cap}")
        eng.sync()


@pytest.mark.parametrize("payload", [False, True])
def test_output_selection(rsx, payload):
    a, aoff, b, boff = R.typed(*RAGGED, "int32", False)
    ref, ref_off = reference(a, aoff, b, boff, LEFT)
    eng = engine(rsx, a.dtype, payload=payload)
    for k in (1, 2, 3):
        for want in itertools.combinations(OUTPUTS, k):
            out, ooff, _ = run(rsx, a, aoff, b, boff, LEFT, want=want, eng=eng)
            assert set(out) == set(want)
            check(out, ooff, ref, ref_off, what=str(want))
    eng.sync()


@pytest.mark.parametrize("dtype", ["uint32", "uint64"])
def test_every_residue_of_16_bytes(rsx, dtype):
    a, aoff, b, boff = R.typed(*R.layout_many_segments(), dtype, False)
    ref, ref_off = reference(a, aoff, b, boff, INNER)
    eng = engine(rsx, a.dtype)
    per = 16 // np.dtype(dtype).itemsize
    for s in range(4):
        out, ooff, _ = run(rsx, a, aoff, b, boff, INNER, eng=eng, shifts=(s % per, s, (s + 1) % 4))
        check(out, ooff, ref, ref_off, what=f"shift {s}")
    eng.sync()


# -- the argument rules -------------------------------------------------------------------------------------------------------------------

def test_refusals(rsx):
    """every argument rule of the contract, one change at a time from a valid call, with the message"""
    t = _torch()
    n = 3 * TILE
    eng = rsx.Engine(np.uint32, n, payload=True)
    a = t.arange(n + 8, dtype=t.int32, device="cuda")
    b = t.arange(n + 8, dtype=t.int32, device="cuda")
    ko, ia, ib = (t.full((n + 8,), -7, dtype=t.int32, device="cuda") for _ in range(3))
    aoff = t.tensor([0, n, n, n], dtype=t.int64, device="cuda")
    boff = t.tensor([0, 5, 5, n], dtype=t.int64, device="cuda")
    ooff = t.full((5,), -7, dtype=t.int64, device="cuda")
    lib = rsx.load_library()
    p = lambda x: None if x is None else C.c_void_p(x)
    base = dict(e=eng._h, d_a=a.data_ptr(), na=n, aoff=aoff.data_ptr(), d_b=b.data_ptr(), nb=n, boff=boff.data_ptr(), nseg=3, op=0, flags=0, cap=n, ko=ko.data_ptr(),
                ia=ia.data_ptr(), ib=ib.data_ptr(), ooff=ooff.data_ptr())

    def call(**kw):
        g = {**base, **kw}
        return lib.rsx_segmented_join(g["e"], p(g["d_a"]), g["na"], p(g["aoff"]), p(g["d_b"]), g["nb"], p(g["boff"]), g["nseg"], g["op"], g["flags"], g["cap"],
                                      p(g["ko"]), p(g["ia"]), p(g["ib"]), p(g["ooff"]))

    refused = [
        (4, "null engine", dict(e=None)),
        (4, "unknown op", dict(op=4)), (4, "unknown op", dict(op=1 << 31)),
        (4, "flags must be 0", dict(flags=1)), (4, "flags must be 0", dict(flags=64)),
        (4, "one offsets array without the other", dict(aoff=None)), (4, "one offsets array without the other", dict(boff=None)),
        (4, "at most 2^31 keys", dict(na=(1 << 31) + 1)), (4, "at most 2^31 keys", dict(nb=(1 << 31) + 1)),
        (4, "at most 2^32 - 2 segments", dict(nseg=0xFFFFFFFF)),
        (4, "out_capacity above 2^34", dict(cap=(1 << 34) + 1)),
        (4, "RSX_JOIN_ANTI", dict(op=3)),
        (1, "d_out_offsets is required", dict(ooff=None)),
        (1, "16-byte aligned", dict(d_a=None)), (1, "16-byte aligned", dict(d_b=None)), (1, "16-byte aligned", dict(d_a=a.data_ptr() + 4)),
        (1, "16-byte aligned", dict(d_b=b.data_ptr() + 8)),
        (1, "aligned to their element size", dict(ia=ia.data_ptr() + 2)), (1, "aligned to their element size", dict(ib=ib.data_ptr() + 1)),
        (1, "aligned to their element size", dict(ko=ko.data_ptr() + 2)),
        (1, "offsets must be", dict(aoff=aoff.data_ptr() + 4)), (1, "offsets must be", dict(boff=boff.data_ptr() + 4)), (1, "offsets must be", dict(ooff=ooff.data_ptr() + 4)),
        (1, "two outputs overlap", dict(ib=ia.data_ptr() + 4 * (n - 1))), (1, "two outputs overlap", dict(ko=ia.data_ptr())),
        (1, "an output overlaps an input", dict(ia=a.data_ptr() + 16)), (1, "an output overlaps an input", dict(ko=b.data_ptr() + 4 * (n - 1))),
        (1, "an output overlaps an input", dict(ooff=aoff.data_ptr())), (1, "an output overlaps an input", dict(ib=boff.data_ptr(), cap=4)),
        (1, "the engine's own buffers", dict(ia=eng.result_device()[0])), (1, "the engine's own buffers", dict(d_a=eng.result_device()[0])),
        (1, "the engine's own buffers", dict(ooff=eng.result_device()[1])),
    ]
    for status, text, kw in refused:
        assert call(**kw) == status, kw
        msg = lib.rsx_last_error().decode()
        assert msg.startswith("rsx_segmented_join: ") and text in msg, (kw, msg)
    eng64 = rsx.Engine(np.uint64, CAP)
    assert lib.rsx_segmented_join(eng64._h, p(a.data_ptr()), 8, None, p(b.data_ptr()), 8, None, 1, 0, 0, 8, p(ko.data_ptr() + 4), None, None, p(ooff.data_ptr())) == 1
    eng.sync()
    assert all(bool((x == -7).all()) for x in (ko, ia, ib, ooff)), "a refused call wrote something"
    assert call() == 0                                                           # and the call these were variations of works,
    eng.sync()
    assert ooff.tolist()[:4] == [0, 5, 5, 5] and ia[:5].tolist() == ib[:5].tolist() == ko[:5].tolist() == [0, 1, 2, 3, 4] and bool((ia[5:] == -7).all())
    assert call(op=3, ib=None) == 0 and call(ko=None, ia=None, ib=None, cap=1 << 60) == 0      # ANTI without B indices; count only ignores the capacity
    eng.sync()
    with pytest.raises(rsx.RadixSortError) as ei:                                # the Engine method carries the same text
        eng.segmented_join(a.data_ptr(), n, None, b.data_ptr(), n, None, 1, 7, 0, ooff.data_ptr())
    assert "unknown op" in str(ei.value)


@pytest.mark.parametrize("case", ["a_decreasing", "b_past_nb", "b_only"])
def test_bad_offsets(rsx, case):
    a, aoff, b, boff = R.layout_many_segments()
    aoff, boff = aoff.copy(), boff.copy()
    if case == "a_decreasing":
        aoff[100] = aoff[99] - 1                                                 # (segments have at least 3 keys: segment 98 stays valid)
        first = 99
    elif case == "b_past_nb":
        boff[-1] = b.size + 1
        first = len(boff) - 2
    else:
        boff[2000] = boff[2001] + 1
        first = 2000
    eng = engine(rsx, a.dtype)
    out, ooff, _ = run(rsx, a, aoff, b, boff, LEFT, cap=1000, eng=eng)
    assert np.all(ooff == 0) and all(np.all(v == SENT32) for v in out.values())
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert "rsx_segmented_join: segment %d " % first in str(ei.value)
    eng.sync()                                                                   # reported once
    a, aoff, b, boff = R.layout_many_segments()
    run_and_check(rsx, a, aoff, b, boff, LEFT, "after bad offsets", eng=eng).sync()       # and the next call is clean


# -- the engine ---------------------------------------------------------------------------------------------------------------------------

def test_sort_state_untouched_and_sizes_beyond_the_capacity(rsx):
    t = _torch()
    rng = np.random.default_rng(3)
    eng = rsx.Engine(np.uint32, CAP)
    x = rng.integers(0, 1 << 32, CAP, dtype=np.uint32)
    xd = dev(t, x)
    eng.sort_from(xd.data_ptr(), CAP)
    a, aoff, b, boff = RAGGED
    assert a.size > 10 * CAP and b.size > 10 * CAP
    ref_off = reference(a, aoff, b, boff, LEFT)[1]
    assert int(ref_off[-1]) > 10 * CAP
    run_and_check(rsx, a, aoff, b, boff, LEFT, "on an engine that holds a sort's result", eng=eng)
    assert eng.geometry().num_keys == CAP
    out = t.zeros(CAP, dtype=t.int32, device="cuda")
    eng.copy_result(out.data_ptr())
    eng.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.sort(x))


def test_two_engines_on_two_streams_give_identical_bits(rsx):
    t = _torch()
    a, aoff, b, boff = R.typed(*RAGGED, "float32", True)
    outs = []
    for _ in range(2):
        s = t.cuda.Stream()
        eng = engine(rsx, a.dtype, stream=s.cuda_stream, descending=True)
        out, ooff, _ = run(rsx, a, aoff, b, boff, LEFT, eng=eng, descending=True)
        eng.sync()
        outs.append((out, ooff))
    assert np.array_equal(outs[0][1], outs[1][1]) and all(np.array_equal(outs[0][0][k], outs[1][0][k]) for k in OUTPUTS)
    ref, ref_off = reference(a, aoff, b, boff, LEFT, True)
    check(outs[0][0], outs[0][1], ref, ref_off, what="two engines")


def test_capture_and_replay(rsx):
    """one captured call (one linear stream) is replayed twice after the keys and the offsets were changed in place"""
    t = _torch()
    rng = np.random.default_rng(70)
    la, lb = [5, 0, 4096, 1, 700, 0, 0, 4500, 33, 2], [0, 3, 4000, 1, 900, 0, 7, 4100, 40, 2]
    na, nb, rows = sum(la), sum(lb), 60000
    side = t.cuda.Stream()
    eng = engine(rsx, np.uint32, stream=side.cuda_stream)

    def data():
        pa, pb = [int(v) for v in rng.permutation(la)], [int(v) for v in rng.permutation(lb)]
        a = np.concatenate([np.sort(rng.integers(0, 1500, x, dtype=np.uint32)) for x in pa])
        b = np.concatenate([np.sort(rng.integers(0, 1500, y, dtype=np.uint32)) for y in pb])
        return a, R.offsets_from(pa), b, R.offsets_from(pb)

    a, aoff, b, boff = data()
    da, dao, db, dbo = dev(t, a), dev(t, aoff), dev(t, b), dev(t, boff)
    outs = [dev(t, np.full(rows * 4, FILL, dtype=np.uint8)) for _ in range(3)]
    ooff = dev(t, np.zeros(len(la) + 1, dtype=np.uint64))

    def call():
        eng.segmented_join(da.data_ptr(), na, dao.data_ptr(), db.data_ptr(), nb, dbo.data_ptr(), len(la), INNER, rows, ooff.data_ptr(), d_a_index_out=outs[1].data_ptr(),
                           d_b_index_out=outs[2].data_ptr(), d_keys_out=outs[0].data_ptr())

    def result():
        return {name: o.cpu().numpy().view(np.uint32) for name, o in zip(OUTPUTS, outs)}, ooff.cpu().numpy().view(np.uint64)

    call()                                                         # eager: sizes the scratch
    eng.sync()
    check(*result(), *reference(a, aoff, b, boff, INNER), rows, "eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for rep in range(2):
        a, aoff, b, boff = data()
        for d, h in ((da, a), (dao, aoff), (db, b), (dbo, boff)):
            d.copy_(t.from_numpy(h.view({4: np.int32, 8: np.int64}[h.dtype.itemsize])))
        for o in outs:
            o.fill_(FILL - 256)
        t.cuda.synchronize()
        graph.replay()
        t.cuda.synchronize()
        check(*result(), *reference(a, aoff, b, boff, INNER), rows, f"replay {rep}")
    del graph
    eng.sync()


# -- unsorted inputs ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True])
def test_unsorted_inputs_keep_the_invariants(rsx, ragged):
    rng = np.random.default_rng(11)
    if ragged:
        la, lb = rng.integers(0, 300, 200), rng.integers(0, 300, 200)
        aoff, boff = R.offsets_from(la), R.offsets_from(lb)
    else:
        la, lb, aoff, boff = [9000], [7000], None, None
    a = rng.integers(0, 40, int(np.sum(la)), dtype=np.uint32)
    b = rng.integers(0, 40, int(np.sum(lb)), dtype=np.uint32)
    for op in (INNER, LEFT, SEMI, ANTI):
        _, counted, eng = run(rsx, a, aoff, b, boff, op, cap=0, want=())
        assert np.all(np.diff(counted.astype(np.int64)) >= 0) and counted[0] == 0                       # the offsets are non-decreasing
        P = int(counted[-1])
        for cap in (P, P // 2):
            out, ooff, _ = run(rsx, a, aoff, b, boff, op, cap=cap, rows=P + 500, eng=eng)           # (no access leaves the buffers: the guard bands)
            assert np.array_equal(ooff, counted)
            for name, v in out.items():
                assert np.all(v[cap:] == SENT32), f"{name}: written past min(P, capacity)"
            seg = np.repeat(np.arange(len(la)), np.diff(ooff.astype(np.int64)))[:cap]
            assert np.all(out["ia"][:cap] < np.asarray(la)[seg])                                      # (also: every row below the capacity is written)
            assert np.all(out["keys"][:cap] < 40)
            if op != ANTI:
                ibv = out["ib"][:cap]
                assert np.all((ibv < np.asarray(lb)[seg]) | (ibv == NONE32))
        eng.sync()


# -- the torch helpers --------------------------------------------------------------------------------------------------------------------

def test_join_sorted_matches_the_outer_comparison(rsx):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(5)
    for dt in (t.int32, t.int64, t.float32, t.float64):
        a = t.sort(t.randint(-40, 40, (300,), device="cuda", generator=g).to(dt)).values
        b = t.sort(t.randint(-40, 40, (200,), device="cuda", generator=g).to(dt)).values
        ia, ib = rsx.join_sorted(a, b)
        want = t.nonzero(a[:, None] == b[None, :])
        assert ia.dtype == ib.dtype == t.int64 and t.equal(ia, want[:, 0]) and t.equal(ib, want[:, 1])
        ad, bd = a.flip(0).contiguous(), b.flip(0).contiguous()
        ia, ib = rsx.join_sorted(ad, bd, descending=True)
        want = t.nonzero(ad[:, None] == bd[None, :])
        assert t.equal(ia, want[:, 0]) and t.equal(ib, want[:, 1])
    a2 = t.sort(t.randint(0, 30, (7, 50), device="cuda", generator=g), dim=1).values
    b2 = t.sort(t.randint(0, 30, (7, 40), device="cuda", generator=g), dim=1).values
    ia, ib, ro = rsx.join_sorted(a2, b2)
    want = t.nonzero(a2[:, :, None] == b2[:, None, :])
    assert t.equal(ia, want[:, 1]) and t.equal(ib, want[:, 2]) and ro.tolist() == [0] + np.cumsum(np.bincount(want[:, 0].cpu().numpy(), minlength=7)).tolist()
    ia, ib, oo, keys = rsx.segmented_join(a2.reshape(-1), t.arange(8, device="cuda") * 50, b2.reshape(-1), t.arange(8, device="cuda") * 40, return_keys=True)
    assert t.equal(ia, want[:, 1]) and t.equal(oo, ro) and t.equal(keys, a2[want[:, 0], want[:, 1]])
    ia, ib = rsx.join_sorted(a[1:], b[3:])                               # misaligned views are copied
    assert t.equal(ia, t.nonzero(a[1:, None] == b[None, 3:])[:, 0])


def test_isin_and_left(rsx):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(6)
    a = t.sort(t.randint(0, 3000, (9000,), device="cuda", generator=g)).values
    b = t.sort(t.randint(0, 3000, (1500,), device="cuda", generator=g)).values
    assert t.equal(rsx.isin_sorted(a, b), t.isin(a, b)) and t.equal(rsx.isin_sorted(a, b, invert=True), ~t.isin(a, b))
    a2 = t.sort(t.randint(0, 60, (33, 70), device="cuda", generator=g).to(t.int32), dim=1).values
    b2 = t.sort(t.randint(0, 60, (33, 20), device="cuda", generator=g).to(t.int32), dim=1).values
    want = (a2[:, :, None] == b2[:, None, :]).any(dim=2)
    assert t.equal(rsx.isin_sorted(a2, b2), want) and t.equal(rsx.isin_sorted(a2, b2, invert=True), ~want)
    ia, ib = rsx.join_sorted(a, b, how="left")
    ah, bh = a.cpu().numpy(), b.cpu().numpy()
    lo, hi = np.searchsorted(bh, ah, "left"), np.searchsorted(bh, ah, "right")
    rows = [(i, j) for i in range(ah.size) for j in (range(lo[i], hi[i]) if hi[i] > lo[i] else [-1])]
    assert ia.tolist() == [r[0] for r in rows] and ib.tolist() == [r[1] for r in rows]
    ia, ib = rsx.join_sorted(a, b, how="anti")
    assert ib is None and t.equal(ia, t.nonzero(~t.isin(a, b)).reshape(-1))
    ia, ib = rsx.join_sorted(a, b, how="semi")
    assert t.equal(ia, t.nonzero(t.isin(a, b)).reshape(-1)) and t.equal(ib, t.from_numpy(lo[hi > lo]).cuda())


def test_capacity_int_does_not_synchronise_and_helper_errors(rsx):
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(7)
    a = t.sort(t.randint(0, 500, (5000,), device="cuda", generator=g)).values
    b = t.sort(t.randint(0, 500, (700,), device="cuda", generator=g)).values
    want = t.nonzero(a[:, None] == b[None, :])
    P = want.shape[0]
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        rsx.segmented_join(a, None, b, None, capacity=P + 10)                      # eager on this stream: sizes its engine's scratch
        rsx.isin_sorted(a, b)
    side.synchronize()
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):                                         # a host synchronisation would raise in here
        ia, ib, oo = rsx.segmented_join(a, None, b, None, capacity=P + 10)
        sa, sb, so = rsx.segmented_join(a, None, b, None, capacity=100)
        mask = rsx.isin_sorted(a, b)
    graph.replay()
    t.cuda.synchronize()
    assert oo.tolist() == [0, P] and so.tolist() == [0, P] and ia.numel() == P + 10 and sa.numel() == 100
    assert t.equal(ia[:P], want[:, 0]) and t.equal(ib[:P], want[:, 1]) and bool((ia[P:] == -1).all()) and bool((ib[P:] == -1).all())
    assert t.equal(sa, want[:100, 0]) and t.equal(sb, want[:100, 1]) and t.equal(mask, t.isin(a, b))
    del graph
    with pytest.raises(TypeError):
        rsx.join_sorted(a, b.to(t.int32))
    for bad in (a.to(t.bfloat16), a.to(t.float16), a > 3):
        with pytest.raises(TypeError):
            rsx.join_sorted(bad, bad)
    with pytest.raises(ValueError):
        rsx.join_sorted(a.cpu(), b)
    with pytest.raises(ValueError):
        rsx.join_sorted(a, b, how="outer")
    with pytest.raises(ValueError):
        rsx.segmented_join(a, t.tensor([0, 5000], device="cuda"), b, None)
    with pytest.raises(ValueError):
        rsx.join_sorted(a, b, capacity=-1)
    with pytest.raises(ValueError):
        rsx.join_sorted(a.reshape(50, 100), b)
    with pytest.raises(rsx.RadixSortError):                                        # bad offsets surface at the read-back
        rsx.segmented_join(a, t.tensor([0, 6000], device="cuda"), b, t.tensor([0, 700], device="cuda"))


# -- equal to the composition it replaces -------------------------------------------------------------------------------------------------

def test_inner_equals_the_composition(rsx):
    """search lower + search right + cumsum + segmented_expand + arithmetic, the class tools/join_bench.py times, entry for entry"""
    t = _torch()
    spec = importlib.util.spec_from_file_location("join_bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "join_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for dtype, descending in (("int32", False), ("float64", True)):
        a, aoff, b, boff = R.typed(*RAGGED, dtype, descending)
        ref, ref_off = reference(a, aoff, b, boff, INNER, descending)
        P = int(ref_off[-1])
        out, ooff, eng = run(rsx, a, aoff, b, boff, INNER, descending=descending)
        eng.sync()
        stream = t.cuda.current_stream()
        comp = bench.Composition(dev(t, a).view(getattr(t, dtype)), dev(t, aoff), dev(t, b).view(getattr(t, dtype)), dev(t, boff), descending, P, stream.cuda_stream)
        comp.run()
        t.cuda.synchronize()
        assert np.array_equal(comp.ia.cpu().numpy().view(np.uint32), out["ia"]) and np.array_equal(comp.ib.cpu().numpy().view(np.uint32), out["ib"])
        assert np.array_equal(comp.out_offsets.cpu().numpy().view(np.uint64), ooff)
        comp.close()
