"""Set operations on sorted segments (rsx_segmented_set_op, radix_sort_amd.segmented_set_op / intersect_sorted / ...) on the GPU.

The referee is tests/_setop_ref.py; every comparison is exact equality of bits with setop_oracle: the call moves bits, there is no tolerance
anywhere.  Every output starts out holding the family's sentinel, which must survive from koff[S] on, and ends in a guard band.  The
output buffers have exactly the size the call asks for: na elements for intersection and difference, na + nb for the other two.  Keys
outside [aoff[0], aoff[S]) and [boff[0], boff[S]) are random, so that reading one changes an answer.  Every engine here has capacity 4096:
the call is not bound by it.
"""
import ctypes as C

import numpy as np
import pytest

import _merge_ref as M
import _setop_ref as R
from _merge_ref import sorted_segments
from _search_ref import UINT, sort_engine_order
from _setop_ref import OPS, capacity, setop_oracle
from test_gpu_merge import CAP, GUARD_BYTE, filled, gather, payloads
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, FILL32, FILL64, GUARD
from test_merge import ragged_inputs
from test_search import HEADER_DTYPES as DTYPES
from test_search import random_keys

pytestmark = pytest.mark.gpu

ALL = ("keys", "index", "match")


def run(rsx, a, aoff, b, boff, op, pa=None, pb=None, descending=False, eng=None, want=ALL, payload_engine=False):
    """One rsx_segmented_set_op through the Engine API.  Every output is pre-filled with the sentinel and followed by a guard band; the
    match output exists for the intersection only.  Returns ({name: host array of the whole output}, engine)."""
    t = _torch()
    na, nb, ks = a.size, b.size, a.dtype.itemsize
    nseg = 1 if aoff is None else len(aoff) - 1
    ad, bd = dev(t, a), dev(t, b)
    ao = None if aoff is None else dev(t, np.asarray(aoff, dtype=np.uint64))
    bo = None if boff is None else dev(t, np.asarray(boff, dtype=np.uint64))
    pad = None if pa is None else dev(t, np.asarray(pa, dtype=np.uint32))
    pbd = None if pb is None else dev(t, np.asarray(pb, dtype=np.uint32))
    n = capacity(op, na, nb)
    kout = filled(t, n * ks) if "keys" in want else None
    iout = filled(t, n * 4) if "index" in want else None
    mout = filled(t, n * 4) if "match" in want and op == R.INTERSECTION else None
    pout = filled(t, n * 4) if pa is not None else None
    koff = filled(t, (nseg + 1) * 8)
    if eng is None:
        eng = rsx.Engine(a.dtype, CAP, payload=payload_engine, descending=descending)
    ptr = lambda x: None if x is None else x.data_ptr()
    eng.segmented_set_op(ptr(ad) if na else None, na, ptr(ao), ptr(bd) if nb else None, nb, ptr(bo), nseg, op, ptr(kout), ptr(koff), ptr(iout), ptr(mout),
                         d_a_payload=ptr(pad), d_b_payload=ptr(pbd), d_payload_out=ptr(pout))
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    got = {}
    for name, buf, size in (("keys", kout, ks), ("index", iout, 4), ("match", mout, 4), ("payload", pout, 4), ("koff", koff, 8)):
        if buf is None:
            continue
        raw = buf.cpu().numpy().view(np.uint8)
        assert np.all(raw[-GUARD:] == GUARD_BYTE), f"{name}: guard band written"
        got[name] = raw[:-GUARD].copy().view({4: np.uint32, 8: np.uint64}[size])
    return got, eng


def check(got, a, aoff, b, boff, op, descending=False, pa=None, pb=None, what="", ref=None):
    """exact equality with the referee in [0, koff[S]), the sentinel from there on"""
    rk, ri, rm, rkoff = setop_oracle(a, aoff, b, boff, op, descending) if ref is None else ref
    u = UINT[a.dtype.itemsize]
    total, n = int(rkoff[-1]), capacity(op, a.size, b.size)
    what = f"{what} [{R.OP_NAMES[op]}]"
    assert np.array_equal(got["koff"].astype(np.int64), rkoff), f"{what}: kept offsets differ: {got['koff'][:8].tolist()} != {rkoff[:8].tolist()}"
    fill = lambda dt, tail: np.full(tail, FILL64 & ((1 << (8 * np.dtype(dt).itemsize)) - 1), dtype=dt)
    wants = {"keys": np.concatenate([rk.view(u), fill(u, n - total)]), "index": np.concatenate([ri.astype(np.uint32), fill(np.uint32, n - total)])}
    if rm is not None:
        wants["match"] = np.concatenate([rm.astype(np.uint32), fill(np.uint32, n - total)])
    if pa is not None:
        ao, bo = (np.array([0, a.size]), np.array([0, b.size])) if aoff is None else (np.asarray(aoff).astype(np.int64), np.asarray(boff).astype(np.int64))
        wants["payload"] = np.concatenate([gather(ri, rkoff, ao, bo, np.asarray(pa, dtype=np.uint32), np.asarray(pb, dtype=np.uint32)), fill(np.uint32, n - total)])
    for name, want in wants.items():
        if name in got:
            bad = np.flatnonzero(got[name] != want)
            assert bad.size == 0, f"{what}: {name} differ at {bad[:8].tolist()} (of {bad.size}): {got[name][bad[:8]].tolist()} != {want[bad[:8]].tolist()}"
    return rk, ri, rm, rkoff


def run_check(rsx, a, aoff, b, boff, op, what="", ref=None, **kw):
    got, eng = run(rsx, a, aoff, b, boff, op, **kw)
    check(got, a, aoff, b, boff, op, kw.get("descending", False), kw.get("pa"), kw.get("pb"), what, ref)
    return got, eng


# -- 1. the ragged layout: six dtypes x both directions x four ops ----------------------------------------------------------------------------

@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_ragged_matrix(rsx, dt, descending):
    rng = np.random.default_rng(100 + DTYPES.index(dt) * 2 + descending)
    a, aoff, b, boff = ragged_inputs(dt, rng, descending)
    assert aoff[0] == 3 and boff[0] == 7 and aoff[-1] < a.size and boff[-1] < b.size
    pa, pb = payloads(a.size, b.size, rng)
    eng = rsx.Engine(dt, CAP, descending=descending)
    for op in OPS:
        run_check(rsx, a, aoff, b, boff, op, f"{np.dtype(dt).name} descending={descending}", pa=pa, pb=pb, descending=descending, eng=eng)
    eng.sync()


# -- 2. runs longer than a tile ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("na,nb", [(9000, 5000), (5000, 9000), (4096, 4096), (1, 8193), (8193, 1)])
def test_all_keys_equal(rsx, na, nb):
    """one run crosses two tile boundaries with m > n, m < n and m = n: the run starts reach back past the staged range and the probes
    leave it on either side"""
    for dt in (np.uint32, np.float64):
        a, b = np.full(na, 7, dtype=dt), np.full(nb, 7, dtype=dt)
        eng = rsx.Engine(dt, CAP)
        pa, pb = payloads(na, nb, np.random.default_rng(na))
        for op in OPS:
            got, _ = run_check(rsx, a, None, b, None, op, f"all equal {na} + {nb}", eng=eng, pa=pa, pb=pb)
            assert int(got["koff"][1]) == R.expected_count(op, na, nb)
        eng.sync()


def test_256_distinct_values(rsx):
    rng = np.random.default_rng(21)
    na, nb = 20000, 30000
    for dt, descending in ((np.uint32, False), (np.int64, True)):
        a = sort_engine_order(rng.integers(0, 256, na).astype(dt), descending)
        b = sort_engine_order(rng.integers(0, 256, nb).astype(dt), descending)
        pa, pb = payloads(na, nb, rng)
        eng = rsx.Engine(dt, CAP, descending=descending)
        for op in OPS:
            run_check(rsx, a, None, b, None, op, "256 distinct values", pa=pa, pb=pb, descending=descending, eng=eng)
        eng.sync()


# -- 3. disjoint, interleaved, identical and empty inputs -------------------------------------------------------------------------------------

def test_disjoint_interleaved_identical_and_single(rsx):
    n = 10000
    lo, hi = np.arange(n, dtype=np.uint32), np.arange(n, 2 * n + 5, dtype=np.uint32)
    eng = rsx.Engine(np.uint32, CAP)
    for op in OPS:
        run_check(rsx, lo, None, hi, None, op, "all of A before all of B", eng=eng)
        run_check(rsx, hi, None, lo, None, op, "all of B before all of A", eng=eng)
        run_check(rsx, 2 * lo, None, 2 * lo + 1, None, op, "strictly alternating", eng=eng)
        got, _ = run_check(rsx, lo, None, lo.copy(), None, op, "identical", eng=eng)
        if op in (R.INTERSECTION, R.UNION):                                      # the intersection of identical inputs is A
            assert int(got["koff"][1]) == n and np.array_equal(got["keys"][:n], lo) and np.array_equal(got["index"][:n], lo)
        else:
            assert int(got["koff"][1]) == 0
        for place in (0, n // 2, n - 1, n):                                      # one key against 10000: first, middle, last place, behind the end
            one = np.array([place], dtype=np.uint32)
            run_check(rsx, one, None, lo, None, op, f"A of length 1 at {place}", eng=eng)
            run_check(rsx, lo, None, one, None, op, f"B of length 1 at {place}", eng=eng)
        got, _ = run_check(rsx, lo, None, lo[:0], None, op, "B empty", eng=eng)
        assert int(got["koff"][1]) == (0 if op == R.INTERSECTION else n)        # union, difference, symmetric difference give A back
        run_check(rsx, lo[:0], None, lo, None, op, "A empty", eng=eng)
        got, _ = run(rsx, lo[:0], None, lo[:0], None, op, eng=eng)             # na + nb == 0: nothing is launched, nothing is written
        assert np.all(got["koff"] == FILL64)
    eng.sync()


# -- 4. many small segments -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["small", "medium"])
def test_many_segments(rsx, layout):
    rng = np.random.default_rng(400 if layout == "small" else 401)             # (the layouts tests/test_merge.py looks at)
    na, aoff, nb, boff = M.small_segments_layout(rng) if layout == "small" else M.medium_segments_layout(rng)
    assert layout != "small" or (np.any(np.diff(aoff) == 0) and np.any(np.diff(boff) == 0))          # empty segments on either side
    for dt, descending in ((np.uint32, False), (np.float64, True)):
        a = sorted_segments(random_keys(dt, na, rng, narrow=True), aoff, descending)
        b = sorted_segments(random_keys(dt, nb, rng, narrow=True), boff, descending)
        pa, pb = payloads(na, nb, rng)
        eng = rsx.Engine(dt, CAP, descending=descending)
        for op in OPS:
            run_check(rsx, a, aoff, b, boff, op, f"{layout} segments", pa=pa, pb=pb, descending=descending, eng=eng)
        eng.sync()


# -- 5. output selection ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("payload_engine", [False, True], ids=["plain_engine", "payload_engine"])
def test_output_selection(rsx, payload_engine):
    rng = np.random.default_rng(500)
    a, aoff, b, boff = ragged_inputs(np.int64, rng)
    pa, pb = payloads(a.size, b.size, rng)
    eng = rsx.Engine(np.int64, CAP, payload=payload_engine)
    for op in (R.INTERSECTION, R.SYMMETRIC_DIFFERENCE):
        ref = setop_oracle(a, aoff, b, boff, op)
        for want in ((), ("keys",), ("index",), ("match",), ("keys", "index"), ("keys", "match"), ("index", "match")):
            got, _ = run_check(rsx, a, aoff, b, boff, op, f"{want} alone", ref=ref, eng=eng, want=want)       # () is count only: the same offsets
            assert set(got) == {"koff"} | {w for w in want if w != "match" or op == R.INTERSECTION}
        got, _ = run_check(rsx, a, aoff, b, boff, op, "everything", ref=ref, eng=eng, pa=pa, pb=pb)
        assert set(got) >= {"keys", "index", "koff", "payload"}
        got, _ = run_check(rsx, a, aoff, b, boff, op, "payload alone", ref=ref, eng=eng, pa=pa, pb=pb, want=())
        assert set(got) == {"payload", "koff"}
    eng.sync()


# -- 6. two tiles per workgroup ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("segments", [1, 4096])
def test_two_tiles_per_workgroup(rsx, segments):
    """the smallest na + nb above 4096 x 16 x CUs; keys only, intersection and union"""
    rng = np.random.default_rng(600 + segments)
    cus = _torch().cuda.get_device_properties(0).multi_processor_count
    total = M.TILE * 16 * cus + 1
    na = total // 2
    nb = total - na
    assert -(-(na + nb) // M.TILE) > 16 * cus
    a, b = rng.integers(0, 1 << 23, na).astype(np.uint32), rng.integers(0, 1 << 23, nb).astype(np.uint32)          # about a third of the keys shared
    if segments == 1:
        aoff = boff = None
        a, b = np.sort(a), np.sort(b)
    else:
        cut = lambda n: np.concatenate([[0], np.sort(rng.integers(0, n + 1, segments - 1)), [n]]).astype(np.int64)
        aoff, boff = cut(na), cut(nb)
        a, b = sorted_segments(a, aoff), sorted_segments(b, boff)
    eng = rsx.Engine(np.uint32, CAP)
    for op in (R.INTERSECTION, R.UNION):
        run_check(rsx, a, aoff, b, boff, op, f"{segments} segment(s), two tiles a workgroup", eng=eng, want=("keys",))
    eng.sync()


# -- 7. alignment -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [np.uint32, np.uint64], ids=["uint32", "uint64"])
def test_every_residue_of_16_bytes(rsx, dt):
    t = _torch()
    rng = np.random.default_rng(700)
    width = 16 // np.dtype(dt).itemsize
    eng = rsx.Engine(dt, CAP)
    for sa in range(width):
        for sb in range(width):
            aoff, boff = np.array([sa, sa + 5000, sa + 5003]), np.array([sb, sb + 5000, sb + 9001])
            a = sorted_segments(random_keys(dt, sa + 5003 + 2, rng, narrow=True), aoff)
            b = sorted_segments(random_keys(dt, sb + 9001 + 2, rng, narrow=True), boff)
            pa, pb = payloads(a.size, b.size, rng)
            for op in (R.INTERSECTION, R.SYMMETRIC_DIFFERENCE):
                run_check(rsx, a, aoff, b, boff, op, f"aoff[0] = {sa}, boff[0] = {sb}", eng=eng, pa=pa, pb=pb)
    x = t.zeros(64, dtype=t.int64, device="cuda")
    out = t.zeros(64, dtype=t.int64, device="cuda")
    size = np.dtype(dt).itemsize
    for da, db in ((size, 0), (0, size)):                                        # a misaligned d_a / d_b is refused
        with pytest.raises(rsx.RadixSortError) as ei:
            eng.segmented_set_op(x.data_ptr() + da, 8, None, x.data_ptr() + 128 + db, 8, None, 1, R.UNION, out.data_ptr(), out.data_ptr() + 256)
        assert ei.value.status == 1 and "rsx_segmented_set_op" in str(ei.value)
    eng.sync()


# -- 8. refusals ------------------------------------------------------------------------------------------------------------------------------

def test_refusals(rsx):
    t = _torch()
    n = 1000
    eng = rsx.Engine(np.uint32, n)
    x = t.zeros(n + 4, dtype=t.int32, device="cuda")
    eng.sort_from(x.data_ptr(), n)                                               # the engine's result buffer is then one of its own
    eng.sync()
    assert eng.result_device()[0] != 0
    a, b = t.arange(n, dtype=t.int32, device="cuda"), t.arange(n, dtype=t.int32, device="cuda")
    pa, pb = t.zeros(n + 4, dtype=t.int32, device="cuda"), t.zeros(n + 4, dtype=t.int32, device="cuda")
    kout, pout, iout, mout = (t.full((2 * n + 4,), -7, dtype=t.int32, device="cuda") for _ in range(4))
    aoff, boff = t.tensor([0, n, n], dtype=t.int64, device="cuda"), t.tensor([0, n, n], dtype=t.int64, device="cuda")
    koff = t.full((4,), -7, dtype=t.int64, device="cuda")
    base = dict(d_a=a.data_ptr(), na=n, d_a_offsets=aoff.data_ptr(), d_b=b.data_ptr(), nb=n, d_b_offsets=boff.data_ptr(), num_segments=1,
                op=R.INTERSECTION, d_keys_out=kout.data_ptr(), d_index_out=iout.data_ptr(), d_match_out=mout.data_ptr(), d_out_offsets=koff.data_ptr(),
                d_a_payload=pa.data_ptr(), d_b_payload=pb.data_ptr(), d_payload_out=pout.data_ptr())
    ok = lambda **kw: eng.segmented_set_op(**{**base, **kw})
    refused = [
        (4, dict(op=4)), (4, dict(op=1 << 31)),                                  # four ops are defined
        (4, dict(flags=1)), (4, dict(flags=1 << 31)),                            # no flag bit is defined
        (4, dict(op=R.UNION)), (4, dict(op=R.DIFFERENCE)), (4, dict(op=R.SYMMETRIC_DIFFERENCE)),      # a match output with another op
        (4, dict(d_a_offsets=None)), (4, dict(d_b_offsets=None)),                # one offsets array without the other
        (4, dict(na=(1 << 31) + 1)), (4, dict(na=1 << 30, nb=(1 << 30) + 1)),    # beyond 2^31 (pointers only: nothing is launched)
        (4, dict(num_segments=(1 << 32) - 1)),
        (4, dict(d_a_payload=None)), (4, dict(d_b_payload=None)), (4, dict(d_payload_out=None)),      # payloads: all or none
        (4, dict(d_a_payload=None, d_b_payload=None)),
        (1, dict(d_out_offsets=None)),                                           # the kept offsets are required
        (1, dict(d_a=None)), (1, dict(d_b=None)),
        (1, dict(d_a=a.data_ptr() + 4)), (1, dict(d_b=b.data_ptr() + 8)),        # not 16-byte aligned
        (1, dict(d_a_payload=pa.data_ptr() + 2)), (1, dict(d_payload_out=pout.data_ptr() + 2)),
        (1, dict(d_keys_out=kout.data_ptr() + 2)), (1, dict(d_index_out=iout.data_ptr() + 2)), (1, dict(d_match_out=mout.data_ptr() + 1)),
        (1, dict(d_a_offsets=aoff.data_ptr() + 4)), (1, dict(d_b_offsets=boff.data_ptr() + 4)), (1, dict(d_out_offsets=koff.data_ptr() + 4)),
        (1, dict(d_keys_out=a.data_ptr())), (1, dict(d_index_out=b.data_ptr())), (1, dict(d_match_out=a.data_ptr())),      # an output on an input
        (1, dict(d_payload_out=pa.data_ptr())), (1, dict(d_keys_out=pb.data_ptr())),
        (1, dict(d_out_offsets=aoff.data_ptr())), (1, dict(d_out_offsets=boff.data_ptr())),
        (1, dict(d_index_out=kout.data_ptr())), (1, dict(d_match_out=iout.data_ptr() + 4 * (n - 1))),          # two outputs (na elements each)
        (1, dict(d_out_offsets=iout.data_ptr() + 8)),
        (1, dict(op=R.UNION, d_match_out=None, d_payload_out=kout.data_ptr() + 4 * (2 * n - 1))),              # (na + nb elements each)
        (1, dict(d_keys_out=eng.result_device()[0])), (1, dict(d_a=eng.result_device()[0])),         # the engine's own buffers
    ]
    for status, kw in refused:
        with pytest.raises(rsx.RadixSortError) as ei:
            ok(**kw)
        assert ei.value.status == status and "rsx_segmented_set_op" in str(ei.value), kw
    ok(d_match_out=iout.data_ptr() + 4 * n)                                      # an intersection's outputs hold na elements: no overlap
    eng.sync()
    iout.fill_(-7)
    lib = rsx.load_library()
    assert lib.rsx_segmented_set_op(None, C.c_void_p(a.data_ptr()), None, n, None, C.c_void_p(b.data_ptr()), None, n, None, 1, 0, 0, C.c_void_p(kout.data_ptr()),
                                    None, None, None, C.c_void_p(koff.data_ptr())) == 4
    assert b"rsx_segmented_set_op" in lib.rsx_last_error() and b"null engine" in lib.rsx_last_error()
    for buf in (kout, pout, mout, koff):
        buf.fill_(-7)
    # na + nb == 0 and no segments: nothing is launched, nothing is written - the kept offsets included
    ok(na=0, nb=0)
    ok(num_segments=0)
    ok(na=0, nb=0, d_a_offsets=None, d_b_offsets=None)
    eng.sync()
    for buf in (kout, pout, iout, mout, koff):
        assert bool((buf == -7).all()), "a refused call wrote something"
    ok()                                                                         # and the call these were variations of works
    eng.sync()
    assert koff.tolist() == [0, n, -7, -7] and kout[:n].tolist() == list(range(n)) and bool((kout[n:] == -7).all())
    assert iout[:n].tolist() == list(range(n)) and mout[:n].tolist() == list(range(n)) and bool((mout[n:] == -7).all())


# -- 9. bad offsets ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", ["a_decreasing", "b_past_nb", "b_only"])
def test_bad_offsets_reported_once(rsx, bad):
    rng = np.random.default_rng(900)
    na, nb = 30000, 20000
    good_a, good_b = np.array([0, 100, 5000, 9000, na]), np.array([5, 100, 4000, 4000, nb])
    a = sorted_segments(rng.integers(0, 99, na).astype(np.uint32), good_a)
    b = sorted_segments(rng.integers(0, 99, nb).astype(np.uint32), good_b)
    aoff, boff = good_a.copy(), good_b.copy()
    if bad == "a_decreasing":
        aoff[3] = 4000                                                           # segment 2 of A is the first bad one
    elif bad == "b_past_nb":
        boff[3] = nb + 1                                                         # segment 2 of B; segment 3 then decreases
    else:
        aoff[4], boff[3] = na - 1, 3999                                          # B alone: segment 2 (A is valid)
    pa, pb = payloads(na, nb, rng)
    eng = rsx.Engine(np.uint32, CAP)
    op = R.INTERSECTION if bad == "b_only" else R.UNION
    got, _ = run(rsx, a, aoff, b, boff, op, pa=pa, pb=pb, eng=eng)               # guard bands checked inside
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "rsx_segmented_set_op" in str(ei.value) and "segment 2 " in str(ei.value)
    eng.sync()                                                                   # reported once
    assert np.all(got["koff"] == 0)
    for name in set(got) - {"koff"}:
        assert np.all(got[name] == FILL32), name
    run_check(rsx, a, good_a, b, good_b, op, "after bad offsets", eng=eng, pa=pa, pb=pb)       # the engine stays usable
    eng.sync()


# -- 10. call state ---------------------------------------------------------------------------------------------------------------------------

def test_sort_state_is_untouched_and_n_exceeds_capacity(rsx):
    t = _torch()
    rng = np.random.default_rng(1000)
    eng = rsx.Engine(np.uint32, CAP)
    x = rng.integers(0, 1 << 32, CAP, dtype=np.uint32)
    xd = dev(t, x)
    eng.sort_from(xd.data_ptr(), CAP)
    a = np.sort(rng.integers(0, 1 << 14, 2 * CAP - 3).astype(np.uint32))
    b = np.sort(rng.integers(0, 1 << 14, CAP + 3).astype(np.uint32))
    for op in OPS:
        run_check(rsx, a, None, b, None, op, "3 x capacity keys on an engine that holds a sort's result", eng=eng)
    assert eng.geometry().num_keys == CAP
    out = t.zeros(CAP, dtype=t.int32, device="cuda")
    t.cuda.synchronize()                                                         # (the engine copies on its own stream)
    eng.copy_result(out.data_ptr())
    eng.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.sort(x))


# -- 11. streams and capture ------------------------------------------------------------------------------------------------------------------

def test_two_engines_two_streams_identical_bits(rsx):
    t = _torch()
    rng = np.random.default_rng(1100)
    a, aoff, b, boff = ragged_inputs(np.float32, rng, True)
    pa, pb = payloads(a.size, b.size, rng)
    res = []
    for s in (t.cuda.Stream(), t.cuda.Stream()):
        eng = rsx.Engine(np.float32, CAP, descending=True)
        eng.set_stream(s.cuda_stream)
        got, _ = run(rsx, a, aoff, b, boff, R.INTERSECTION, pa=pa, pb=pb, descending=True, eng=eng)
        eng.sync()
        res.append(got)
    check(res[0], a, aoff, b, boff, R.INTERSECTION, True, pa, pb, "stream 0")
    for name in res[0]:
        assert np.array_equal(res[0][name], res[1][name]), name


def test_capture_and_replay(rsx):
    """every launch is sized from na, nb and the segment count: one captured call (a linear chain) is replayed after the keys have changed"""
    t = _torch()
    rng = np.random.default_rng(1101)
    dt = np.int32
    op = R.SYMMETRIC_DIFFERENCE
    a, aoff, b, boff = ragged_inputs(dt, rng)
    na, nb, nseg = a.size, b.size, len(aoff) - 1
    side = t.cuda.Stream()
    eng = rsx.Engine(dt, CAP)
    eng.set_stream(side.cuda_stream)
    ad, bd, ao, bo = dev(t, a), dev(t, b), dev(t, aoff.astype(np.uint64)), dev(t, boff.astype(np.uint64))
    kout, iout, koff = (dev(t, np.full(nbytes, FILL, dtype=np.uint8)) for nbytes in (4 * (na + nb), 4 * (na + nb), 8 * (nseg + 1)))

    def call():
        eng.segmented_set_op(ad.data_ptr(), na, ao.data_ptr(), bd.data_ptr(), nb, bo.data_ptr(), nseg, op, kout.data_ptr(), koff.data_ptr(), iout.data_ptr())

    def result():
        return {"keys": kout.cpu().numpy().view(np.uint32), "index": iout.cpu().numpy().view(np.uint32), "koff": koff.cpu().numpy().view(np.uint64)}

    call()                                                                       # eager: the first call of an engine allocates its scratch
    eng.sync()
    check(result(), a, aoff, b, boff, op, what="eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for rep in range(2):
        a, _, b, _ = ragged_inputs(dt, rng)
        ad.copy_(t.from_numpy(a.view(np.int32)))
        bd.copy_(t.from_numpy(b.view(np.int32)))
        for buf in (kout, iout, koff):
            buf.fill_(FILL - 256)
        graph.replay()
        t.cuda.synchronize()
        check(result(), a, aoff, b, boff, op, what=f"replay {rep}")
    del graph
    eng.sync()


# -- 12. inputs that are not sorted -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["one_segment", "ragged"])
def test_unsorted_inputs_stay_inside_the_buffers(rsx, layout):
    """the contract for inputs that are not sorted: the result is unspecified, but the guard bands are intact (run checks them), the kept
    offsets are non-decreasing, koff[S] is at most the buffer size and the sentinel is intact from koff[S] on"""
    rng = np.random.default_rng(1200)
    if layout == "one_segment":
        na, nb, aoff, boff = 30000, 21000, None, None
    else:
        na, aoff, nb, boff = M.ragged_layout()
    eng = rsx.Engine(np.uint32, CAP)
    for narrow in (False, True):
        a = rng.integers(0, 50 if narrow else 1 << 32, na).astype(np.uint32)
        b = rng.integers(0, 50 if narrow else 1 << 32, nb).astype(np.uint32)
        pa, pb = payloads(na, nb, rng)
        for op in OPS:
            got, _ = run(rsx, a, aoff, b, boff, op, pa=pa, pb=pb, eng=eng)
            koff = got["koff"].astype(np.int64)
            total, n = int(koff[-1]), capacity(op, na, nb)
            assert koff[0] == 0 and np.all(np.diff(koff) >= 0) and total <= n, (op, koff[-3:].tolist(), n)
            for name in set(got) - {"koff"}:
                assert np.all(got[name][total:] == FILL32), (op, name)
            if total:                                                            # [0, koff[S]) is written: a payload is one of the inputs'
                assert np.all(np.isin(got["payload"][:total], np.concatenate([pa, pb])))
    eng.sync()


# -- 13. the torch helpers --------------------------------------------------------------------------------------------------------------------

def test_helpers_equal_torch(rsx):
    t = _torch()
    g = t.Generator().manual_seed(13)
    a = t.unique(t.randint(0, 20000, (9000,), generator=g)).to(t.int32).cuda()
    b = t.unique(t.randint(5000, 30000, (12000,), generator=g)).to(t.int32).cuda()
    common = a[t.isin(a, b)]
    assert common.numel() > 1000
    assert t.equal(rsx.intersect_sorted(a, b), common)
    assert t.equal(rsx.difference_sorted(a, b), a[~t.isin(a, b)])
    assert t.equal(rsx.union_sorted(a, b), t.unique(t.cat([a, b])))
    assert t.equal(rsx.symmetric_difference_sorted(a, b), t.sort(t.cat([a[~t.isin(a, b)], b[~t.isin(b, a)]]))[0])
    vals, idx, mt = rsx.intersect_sorted(a, b, return_index=True, return_match=True)
    assert idx.dtype == t.int64 and t.equal(a[idx], vals) and t.equal(b[mt], vals)
    # descending, non-contiguous and misaligned inputs
    ad, bd = t.flip(a, [0]), t.flip(b, [0])
    assert t.equal(rsx.intersect_sorted(ad[1:], bd[::1], descending=True), t.flip(common, [0])[(1 if bool(t.isin(ad[0], b)) else 0):])


def test_inner_join_is_a_sparse_dot_product(rsx):
    t = _torch()
    g = t.Generator().manual_seed(14)
    dim = 50000
    ia = t.unique(t.randint(0, dim, (6000,), generator=g)).to(t.int64).cuda()
    ib = t.unique(t.randint(0, dim, (9000,), generator=g)).to(t.int64).cuda()
    va = t.randint(-100, 100, (ia.numel(),), generator=g).to(t.int32).cuda()
    vb = t.randint(-100, 100, (ib.numel(),), generator=g).to(t.int32).cuda()
    vals, pay, idx, mt = rsx.intersect_sorted(ia, ib, payload_a=va, payload_b=vb, return_index=True, return_match=True)
    assert t.equal(pay, va[idx])                                                 # the kept elements are A's: their payload came along
    da, db = t.zeros(dim, dtype=t.int64, device="cuda"), t.zeros(dim, dtype=t.int64, device="cuda")
    da[ia], db[ib] = va.to(t.int64), vb.to(t.int64)
    assert int((va[idx].to(t.int64) * vb[mt].to(t.int64)).sum()) == int((da * db).sum()) != 0


def test_rows_follow_sort_rows(rsx):
    t = _torch()
    g = t.Generator().manual_seed(15)
    for dt in (t.float32, t.int64):
        x = t.randint(-40, 40, (37, 300), generator=g).to(dt).cuda()
        y = t.randint(-40, 40, (37, 211), generator=g).to(dt).cuda()
        if dt.is_floating_point:
            x[:, ::7] = -0.0
            y[:, ::5] = float("nan")
            y[:, 1::9] = 0.0
        xs, ys = rsx.sort_rows(x)[0], rsx.sort_rows(y)[0]
        bits = lambda v: v.contiguous().view(t.int32 if v.element_size() == 4 else t.int64).cpu().numpy()
        aoff, boff = np.arange(38) * 300, np.arange(38) * 211
        for fn, op in ((rsx.intersect_sorted, R.INTERSECTION), (rsx.difference_sorted, R.DIFFERENCE), (rsx.union_sorted, R.UNION),
                       (rsx.symmetric_difference_sorted, R.SYMMETRIC_DIFFERENCE)):
            vals, rows, idx = fn(xs, ys, return_index=True)
            rk, ri, _, rkoff = setop_oracle(xs.cpu().numpy().reshape(-1), aoff, ys.cpu().numpy().reshape(-1), boff, op)
            assert rows.dtype == t.int64 and np.array_equal(rows.cpu().numpy(), rkoff)
            assert np.array_equal(bits(vals), rk.view(bits(vals).dtype)) and np.array_equal(idx.cpu().numpy(), ri)


def test_helper_errors(rsx):
    t = _torch()
    a, b = t.arange(10, dtype=t.int32, device="cuda"), t.arange(5, dtype=t.int32, device="cuda")
    off = t.tensor([0, 5], dtype=t.int64, device="cuda")
    with pytest.raises(TypeError):
        rsx.intersect_sorted(a, b.to(t.int64))
    for bad in (t.float16, t.bfloat16, t.bool):
        with pytest.raises(TypeError):
            rsx.union_sorted(a.to(bad), b.to(bad))
    with pytest.raises(ValueError):
        rsx.difference_sorted(a.cpu(), b.cpu())
    with pytest.raises(ValueError):
        rsx.intersect_sorted(a, b, payload_a=a)
    with pytest.raises(ValueError):
        rsx.segmented_set_op(a, off, b, off, "union", payload_b=b)
    with pytest.raises(ValueError):
        rsx.segmented_set_op(a, off, b, None, "union")
    with pytest.raises(ValueError):
        rsx.segmented_set_op(a, None, b, None, "union", return_match=True)
    with pytest.raises(ValueError):
        rsx.segmented_set_op(a, None, b, None, "xor")
    with pytest.raises(ValueError):
        rsx.symmetric_difference_sorted(a.reshape(2, 5), b)
    k, koff = rsx.segmented_set_op(a, None, b, None, rsx.SET_DIFFERENCE)
    assert k.tolist() == [5, 6, 7, 8, 9] and koff.tolist() == [0, 5]
