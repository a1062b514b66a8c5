"""Merge of sorted segments (rsx_segmented_merge, radix_sort_amd.segmented_merge / merge) on the GPU.

The referee is tests/_merge_ref.py; every comparison is exact equality of bits with merge_oracle: the call moves bits, there is no
tolerance anywhere.  Every output starts out holding the family's sentinel, which must survive from ooff[S] on, and ends in a guard band.
Keys outside [aoff[0], aoff[S]) and [boff[0], boff[S]) are random, so that reading one changes an answer.  Every engine here has capacity
4096: the call is not bound by it.  The layouts come from _merge_ref, where tests/test_merge.py checks from the layout alone that each
reaches the path it is named after.
"""
import ctypes as C

import numpy as np
import pytest

import _merge_ref as M
from _merge_ref import merge_oracle, sorted_segments
from _search_ref import UINT, sort_engine_order
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, FILL32, FILL64, GUARD
from test_merge import ragged_inputs
from test_search import HEADER_DTYPES as DTYPES
from test_search import random_keys

pytestmark = pytest.mark.gpu

CAP = 4096
GUARD_BYTE = 0xA5


def filled(t, nbytes):
    return dev(t, np.concatenate([np.full(nbytes, FILL, dtype=np.uint8), np.full(GUARD, GUARD_BYTE, dtype=np.uint8)]))


def run(rsx, a, aoff, b, boff, pa=None, pb=None, descending=False, eng=None, want=("keys", "index", "ooff"), payload_engine=False):
    """One rsx_segmented_merge through the Engine API.  Every output is pre-filled with the sentinel and followed by a guard band.
    Returns ({name: host array of the whole output}, engine)."""
    t = _torch()
    na, nb, ks = a.size, b.size, a.dtype.itemsize
    nseg = 1 if aoff is None else len(aoff) - 1
    ad, bd = dev(t, a), dev(t, b)
    ao = None if aoff is None else dev(t, np.asarray(aoff, dtype=np.uint64))
    bo = None if boff is None else dev(t, np.asarray(boff, dtype=np.uint64))
    pad = None if pa is None else dev(t, np.asarray(pa, dtype=np.uint32))
    pbd = None if pb is None else dev(t, np.asarray(pb, dtype=np.uint32))
    n = na + nb
    kout = filled(t, n * ks) if "keys" in want else None
    iout = filled(t, n * 4) if "index" in want else None
    pout = filled(t, n * 4) if pa is not None else None
    ooff = filled(t, (nseg + 1) * 8) if "ooff" in want else None
    if eng is None:
        eng = rsx.Engine(a.dtype, CAP, payload=payload_engine, descending=descending)
    ptr = lambda x: None if x is None else x.data_ptr()
    eng.segmented_merge(ptr(ad) if na else None, na, ptr(ao), ptr(bd) if nb else None, nb, ptr(bo), nseg, ptr(kout), ptr(iout), ptr(ooff),
                        d_a_payload=ptr(pad), d_b_payload=ptr(pbd), d_payload_out=ptr(pout))
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    got = {}
    for name, buf, size in (("keys", kout, ks), ("index", iout, 4), ("payload", pout, 4), ("ooff", ooff, 8)):
        if buf is None:
            continue
        raw = buf.cpu().numpy().view(np.uint8)
        assert np.all(raw[-GUARD:] == GUARD_BYTE), f"{name}: guard band written"
        got[name] = raw[:-GUARD].copy().view({4: np.uint32, 8: np.uint64}[size])
    return got, eng


def gather(index, ooff, aoff, boff, xa, xb):
    """the elements of xa / xb that the index names: output r of segment s is A_s[j] for j < La, else B_s[j - La]"""
    S = len(ooff) - 1
    seg = np.repeat(np.arange(S), np.diff(ooff))
    la = (aoff[1:] - aoff[:-1])[seg]
    from_a = index < la
    pos_a = np.where(from_a, aoff[:-1][seg] + index, 0)
    pos_b = np.where(from_a, 0, boff[:-1][seg] + index - la)
    xa = xa if xa.size else np.zeros(1, dtype=xa.dtype)
    xb = xb if xb.size else np.zeros(1, dtype=xb.dtype)
    return np.where(from_a, xa[pos_a], xb[pos_b])


def check(got, a, aoff, b, boff, descending=False, pa=None, pb=None, what="", ref=None):
    """exact equality with the referee in [0, ooff[S]), the sentinel from there on"""
    rk, ri, rooff = merge_oracle(a, aoff, b, boff, descending) if ref is None else ref
    u = UINT[a.dtype.itemsize]
    total, n = int(rooff[-1]), a.size + b.size
    if "ooff" in got:
        assert np.array_equal(got["ooff"].astype(np.int64), rooff), f"{what}: out offsets differ: {got['ooff'][:8].tolist()} != {rooff[:8].tolist()}"
    fill = lambda dt, tail: np.full(tail, FILL64 & ((1 << (8 * np.dtype(dt).itemsize)) - 1), dtype=dt)
    wants = {"keys": np.concatenate([rk.view(u), fill(u, n - total)]), "index": np.concatenate([ri.astype(np.uint32), fill(np.uint32, n - total)])}
    if pa is not None:
        ao, bo = (np.array([0, a.size]), np.array([0, b.size])) if aoff is None else (np.asarray(aoff).astype(np.int64), np.asarray(boff).astype(np.int64))
        wants["payload"] = np.concatenate([gather(ri, rooff, ao, bo, np.asarray(pa, dtype=np.uint32), np.asarray(pb, dtype=np.uint32)), fill(np.uint32, n - total)])
    for name, want in wants.items():
        if name in got:
            bad = np.flatnonzero(got[name] != want)
            assert bad.size == 0, f"{what}: {name} differ at {bad[:8].tolist()} (of {bad.size}): {got[name][bad[:8]].tolist()} != {want[bad[:8]].tolist()}"
    return rk, ri, rooff


def run_check(rsx, a, aoff, b, boff, what="", ref=None, **kw):
    got, eng = run(rsx, a, aoff, b, boff, **kw)
    check(got, a, aoff, b, boff, kw.get("descending", False), kw.get("pa"), kw.get("pb"), what, ref)
    return got, eng


def payloads(na, nb, rng):
    return rng.integers(0, 1 << 32, na, dtype=np.uint32), rng.integers(0, 1 << 32, nb, dtype=np.uint32)


# -- 1. the ragged layout: six dtypes x both directions ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_ragged_matrix(rsx, dt, descending):
    rng = np.random.default_rng(100 + DTYPES.index(dt) * 2 + descending)
    a, aoff, b, boff = ragged_inputs(dt, rng, descending)
    assert aoff[0] == 3 and boff[0] == 7 and aoff[-1] < a.size and boff[-1] < b.size
    pa, pb = payloads(a.size, b.size, rng)
    _, eng = run_check(rsx, a, aoff, b, boff, f"{np.dtype(dt).name} descending={descending}", pa=pa, pb=pb, descending=descending)
    eng.sync()


# -- 2. ties across tile boundaries -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("na,nb", [(4097, 8191), ((1 << 16) + 3, (1 << 16) - 5), (4097, 100)])
def test_all_keys_equal(rsx, na, nb):
    """a wrong tie rule in the split kernel duplicates or drops elements at a tile boundary: the index says so exactly"""
    for dt in (np.uint32, np.float64):
        a, b = np.full(na, 7, dtype=dt), np.full(nb, 7, dtype=dt)
        got, eng = run_check(rsx, a, None, b, None, f"all equal {na} + {nb}")
        assert np.array_equal(got["index"][:na + nb], np.arange(na + nb, dtype=np.uint32))             # all of A, then all of B
        eng.sync()


def test_256_distinct_values(rsx):
    rng = np.random.default_rng(21)
    n = 1 << 17
    for dt, descending in ((np.uint32, False), (np.int64, True)):
        a = sort_engine_order(rng.integers(0, 256, n).astype(dt), descending)
        b = sort_engine_order(rng.integers(0, 256, n).astype(dt), descending)
        pa, pb = payloads(n, n, rng)
        _, eng = run_check(rsx, a, None, b, None, "256 distinct values", pa=pa, pb=pb, descending=descending)
        eng.sync()


# -- 3. disjoint and interleaved inputs -------------------------------------------------------------------------------------------------------

def test_disjoint_interleaved_identical_and_single(rsx):
    n = 20011
    lo, hi = np.arange(n, dtype=np.uint32), np.arange(n, 2 * n + 5, dtype=np.uint32)
    eng = rsx.Engine(np.uint32, CAP)
    run_check(rsx, lo, None, hi, None, "all of A before all of B", eng=eng)
    run_check(rsx, hi, None, lo, None, "all of B before all of A", eng=eng)
    run_check(rsx, 2 * lo, None, 2 * lo + 1, None, "strictly alternating", eng=eng)
    run_check(rsx, 2 * lo + 1, None, 2 * lo, None, "strictly alternating, B first", eng=eng)
    got, _ = run_check(rsx, lo, None, lo.copy(), None, "identical", eng=eng)
    assert got["index"][:6].tolist() == [0, n, 1, n + 1, 2, n + 2]
    for place in (0, n // 2, n - 1, n):                                        # one key into 20011: first, middle, last place, behind the end
        one = np.array([place], dtype=np.uint32)
        run_check(rsx, one, None, lo, None, f"A of length 1 at {place}", eng=eng)
        run_check(rsx, lo, None, one, None, f"B of length 1 at {place}", eng=eng)
    run_check(rsx, lo, None, lo[:0], None, "B empty: a copy of A", eng=eng)
    run_check(rsx, lo[:0], None, lo, None, "A empty: a copy of B", eng=eng)
    eng.sync()


# -- 4. many small segments -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["small", "medium"])
def test_many_segments(rsx, layout):
    rng = np.random.default_rng(400 if layout == "small" else 401)             # (the layouts tests/test_merge.py looks at)
    na, aoff, nb, boff = M.small_segments_layout(rng) if layout == "small" else M.medium_segments_layout(rng)
    for dt, descending in ((np.uint32, False), (np.float64, True)):
        a = sorted_segments(random_keys(dt, na, rng, narrow=True), aoff, descending)
        b = sorted_segments(random_keys(dt, nb, rng, narrow=True), boff, descending)
        pa, pb = payloads(na, nb, rng)
        _, eng = run_check(rsx, a, aoff, b, boff, f"{layout} segments", pa=pa, pb=pb, descending=descending)
        eng.sync()


# -- 5. output selection ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("payload_engine", [False, True], ids=["plain_engine", "payload_engine"])
def test_output_selection(rsx, payload_engine):
    rng = np.random.default_rng(500)
    a, aoff, b, boff = ragged_inputs(np.int64, rng)
    ref = merge_oracle(a, aoff, b, boff)
    eng = rsx.Engine(np.int64, CAP, payload=payload_engine)
    for want in (("keys",), ("index",), ("ooff",)):
        got, _ = run_check(rsx, a, aoff, b, boff, f"{want} alone", ref=ref, eng=eng, want=want)
        assert set(got) == set(want)
    pa, pb = payloads(a.size, b.size, rng)
    got, _ = run_check(rsx, a, aoff, b, boff, "everything", ref=ref, eng=eng, pa=pa, pb=pb)
    assert set(got) == {"keys", "index", "ooff", "payload"}
    got, _ = run_check(rsx, a, aoff, b, boff, "payload alone", ref=ref, eng=eng, pa=pa, pb=pb, want=())
    assert set(got) == {"payload"}
    eng.sync()


# -- 6. two tiles per workgroup ---------------------------------------------------------------------------------------------------------------

def test_two_tiles_per_workgroup_one_segment(rsx):
    rng = np.random.default_rng(600)
    na, nb = 1 << 23, (1 << 23) + 4096 * 3 + 5
    a = np.sort(rng.integers(0, 1 << 32, na, dtype=np.uint32))
    b = np.sort(rng.integers(0, 1 << 32, nb, dtype=np.uint32))
    eng = rsx.Engine(np.uint32, CAP)
    assert -(-(na + nb) // M.TILE) > 16 * _torch().cuda.get_device_properties(0).multi_processor_count
    run_check(rsx, a, None, b, None, "one segment, two tiles a workgroup", eng=eng)
    eng.sync()


def test_two_tiles_per_workgroup_segments(rsx):
    rng = np.random.default_rng(601)
    cus = _torch().cuda.get_device_properties(0).multi_processor_count
    S = -(-16 * cus * M.TILE * 9 // (8 * 100000))                               # about 9 / 8 of 16 x CUs tiles: 189 segments at 256 CUs
    la, lb = rng.integers(0, 100000, S), rng.integers(0, 100000, S)
    la[[0, 5, 99]], lb[[1, 5, S - 1]] = 0, 0
    aoff = 11 + np.concatenate([[0], np.cumsum(la)]).astype(np.int64)
    boff = 2 + np.concatenate([[0], np.cumsum(lb)]).astype(np.int64)
    na, nb = int(aoff[-1]) + 9, int(boff[-1]) + 9
    a = sorted_segments(rng.integers(0, 1 << 20, na).astype(np.uint32), aoff)
    b = sorted_segments(rng.integers(0, 1 << 20, nb).astype(np.uint32), boff)
    eng = rsx.Engine(np.uint32, CAP)
    assert -(-(na + nb) // M.TILE) > 16 * cus
    pa, pb = payloads(na, nb, rng)
    run_check(rsx, a, aoff, b, boff, "segments of about 10^5, two tiles a workgroup", eng=eng, pa=pa, pb=pb)
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
            a = sorted_segments(random_keys(dt, sa + 5003 + 2, rng), aoff)
            b = sorted_segments(random_keys(dt, sb + 9001 + 2, rng), boff)
            pa, pb = payloads(a.size, b.size, rng)
            run_check(rsx, a, aoff, b, boff, f"aoff[0] = {sa}, boff[0] = {sb}", eng=eng, pa=pa, pb=pb)
    x = t.zeros(64, dtype=t.int64, device="cuda")
    out = t.zeros(64, dtype=t.int64, device="cuda")
    size = np.dtype(dt).itemsize
    for da, db in ((size, 0), (0, size)):                                        # a misaligned d_a / d_b is refused
        with pytest.raises(rsx.RadixSortError) as ei:
            eng.segmented_merge(x.data_ptr() + da, 8, None, x.data_ptr() + 128 + db, 8, None, 1, out.data_ptr())
        assert ei.value.status == 1 and "rsx_segmented_merge" in str(ei.value)
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
    kout, pout, iout = (t.full((2 * n + 4,), -7, dtype=t.int32, device="cuda") for _ in range(3))
    aoff, boff = t.tensor([0, n, n], dtype=t.int64, device="cuda"), t.tensor([0, n, n], dtype=t.int64, device="cuda")
    ooff = t.full((4,), -7, dtype=t.int64, device="cuda")
    base = dict(d_a=a.data_ptr(), na=n, d_a_offsets=aoff.data_ptr(), d_b=b.data_ptr(), nb=n, d_b_offsets=boff.data_ptr(), num_segments=1,
                d_keys_out=kout.data_ptr(), d_index_out=iout.data_ptr(), d_out_offsets=ooff.data_ptr(), d_a_payload=pa.data_ptr(),
                d_b_payload=pb.data_ptr(), d_payload_out=pout.data_ptr())
    ok = lambda **kw: eng.segmented_merge(**{**base, **kw})
    refused = [
        (4, dict(flags=1)), (4, dict(flags=8)), (4, dict(flags=1 << 31)),       # no flag bit is defined
        (4, dict(d_a_offsets=None)), (4, dict(d_b_offsets=None)),                # one offsets array without the other
        (4, dict(na=(1 << 31) + 1)), (4, dict(nb=(1 << 31) + 1)),                # beyond 2^31 (pointers only: nothing is launched)
        (4, dict(na=1 << 30, nb=(1 << 30) + 1)),                                 # together
        (4, dict(num_segments=(1 << 32) - 1)),
        (4, dict(d_keys_out=None, d_index_out=None, d_out_offsets=None, d_a_payload=None, d_b_payload=None, d_payload_out=None)),      # no output
        (4, dict(d_a_payload=None)), (4, dict(d_b_payload=None)), (4, dict(d_payload_out=None)),      # payloads: all or none
        (4, dict(d_a_payload=None, d_b_payload=None)),
        (1, dict(d_a=None)), (1, dict(d_b=None)),
        (1, dict(d_a=a.data_ptr() + 4)), (1, dict(d_b=b.data_ptr() + 8)),        # not 16-byte aligned
        (1, dict(d_a_payload=pa.data_ptr() + 2)), (1, dict(d_b_payload=pb.data_ptr() + 1)), (1, dict(d_payload_out=pout.data_ptr() + 2)),
        (1, dict(d_keys_out=kout.data_ptr() + 2)), (1, dict(d_index_out=iout.data_ptr() + 2)),
        (1, dict(d_a_offsets=aoff.data_ptr() + 4)), (1, dict(d_b_offsets=boff.data_ptr() + 4)), (1, dict(d_out_offsets=ooff.data_ptr() + 4)),
        (1, dict(d_keys_out=a.data_ptr())), (1, dict(d_index_out=b.data_ptr())),                     # an output on an input:
        (1, dict(d_payload_out=pa.data_ptr())), (1, dict(d_keys_out=pb.data_ptr())),                 # (there is no in-place form)
        (1, dict(d_out_offsets=aoff.data_ptr())), (1, dict(d_out_offsets=boff.data_ptr())),
        (1, dict(d_index_out=kout.data_ptr())), (1, dict(d_payload_out=kout.data_ptr() + 4 * (2 * n - 1))),        # two outputs
        (1, dict(d_out_offsets=iout.data_ptr() + 8)),
        (1, dict(d_keys_out=eng.result_device()[0])), (1, dict(d_a=eng.result_device()[0])),         # the engine's own buffers
    ]
    for status, kw in refused:
        with pytest.raises(rsx.RadixSortError) as ei:
            ok(**kw)
        assert ei.value.status == status and "rsx_segmented_merge" in str(ei.value), kw
    lib = rsx.load_library()
    assert lib.rsx_segmented_merge(None, C.c_void_p(a.data_ptr()), None, n, None, C.c_void_p(b.data_ptr()), None, n, None, 1, 0, C.c_void_p(kout.data_ptr()),
                                   None, None, None) == 4
    assert b"rsx_segmented_merge" in lib.rsx_last_error() and b"null engine" in lib.rsx_last_error()
    # na + nb == 0 and no segments: nothing is launched, nothing is written - the out offsets included
    ok(na=0, nb=0)
    ok(num_segments=0)
    ok(na=0, nb=0, d_a_offsets=None, d_b_offsets=None)
    eng.sync()
    for buf in (kout, pout, iout, ooff):
        assert bool((buf == -7).all()), "a refused call wrote something"
    ok()                                                                         # and the call these were variations of works
    eng.sync()
    assert ooff.tolist() == [0, 2 * n, -7, -7] and kout[:2 * n].tolist() == [i // 2 for i in range(2 * n)]
    assert iout[:6].tolist() == [0, n, 1, n + 1, 2, n + 2] and bool((kout[2 * n:] == -7).all())


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
    got, _ = run(rsx, a, aoff, b, boff, pa=pa, pb=pb, eng=eng)                   # guard bands checked inside
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "rsx_segmented_merge" in str(ei.value) and "segment 2 " in str(ei.value)
    eng.sync()                                                                   # reported once
    assert np.all(got["ooff"] == 0)
    for name in ("keys", "index", "payload"):
        assert np.all(got[name] == FILL32), name
    run_check(rsx, a, good_a, b, good_b, "after bad offsets", eng=eng, pa=pa, pb=pb)       # the engine stays usable
    eng.sync()


# -- 10. call state ---------------------------------------------------------------------------------------------------------------------------

def test_sort_state_is_untouched_and_n_exceeds_capacity(rsx):
    t = _torch()
    rng = np.random.default_rng(1000)
    eng = rsx.Engine(np.uint32, CAP)
    x = rng.integers(0, 1 << 32, CAP, dtype=np.uint32)
    xd = dev(t, x)
    eng.sort_from(xd.data_ptr(), CAP)
    a = np.sort(rng.integers(0, 1 << 32, 2 * CAP - 3, dtype=np.uint32))
    b = np.sort(rng.integers(0, 1 << 32, CAP + 3, dtype=np.uint32))
    run_check(rsx, a, None, b, None, "3 x capacity keys on an engine that holds a sort's result", eng=eng)
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
        got, _ = run(rsx, a, aoff, b, boff, pa=pa, pb=pb, descending=True, eng=eng)
        eng.sync()
        res.append(got)
    check(res[0], a, aoff, b, boff, True, pa, pb, "stream 0")
    for name in res[0]:
        assert np.array_equal(res[0][name], res[1][name]), name


def test_capture_and_replay(rsx):
    """every launch is sized from na, nb and the segment count: one captured call (a linear chain) is replayed after the keys have changed"""
    t = _torch()
    rng = np.random.default_rng(1101)
    dt = np.int32
    a, aoff, b, boff = ragged_inputs(dt, rng)
    na, nb, nseg = a.size, b.size, len(aoff) - 1
    side = t.cuda.Stream()
    eng = rsx.Engine(dt, CAP)
    eng.set_stream(side.cuda_stream)
    ad, bd, ao, bo = dev(t, a), dev(t, b), dev(t, aoff.astype(np.uint64)), dev(t, boff.astype(np.uint64))
    kout, iout, ooff = (dev(t, np.full(nbytes, FILL, dtype=np.uint8)) for nbytes in (4 * (na + nb), 4 * (na + nb), 8 * (nseg + 1)))

    def call():
        eng.segmented_merge(ad.data_ptr(), na, ao.data_ptr(), bd.data_ptr(), nb, bo.data_ptr(), nseg, kout.data_ptr(), iout.data_ptr(), ooff.data_ptr())

    def result():
        return {"keys": kout.cpu().numpy().view(np.uint32), "index": iout.cpu().numpy().view(np.uint32), "ooff": ooff.cpu().numpy().view(np.uint64)}

    call()                                                                       # eager: the first call of an engine allocates its scratch
    eng.sync()
    check(result(), a, aoff, b, boff, what="eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for rep in range(2):
        a, _, b, _ = ragged_inputs(dt, rng)
        ad.copy_(t.from_numpy(a.view(np.int32)))
        bd.copy_(t.from_numpy(b.view(np.int32)))
        for buf in (kout, iout, ooff):
            buf.fill_(FILL - 256)
        graph.replay()
        t.cuda.synchronize()
        check(result(), a, aoff, b, boff, what=f"replay {rep}")
    del graph
    eng.sync()


# -- 12. the torch helpers --------------------------------------------------------------------------------------------------------------------

def test_merge_equals_torch_sort_of_the_concatenation(rsx):
    t = _torch()
    g = t.Generator().manual_seed(12)
    for shape_a, shape_b in (((5000,), (333,)), ((7, 33, 50), (7, 33, 77)), ((3, 0), (3, 9))):
        a = t.sort(t.randint(-50, 50, shape_a, generator=g).to(t.float32) / 4 + 0.125, dim=-1, descending=True)[0].cuda()
        b = t.sort(t.randint(-50, 50, shape_b, generator=g).to(t.float32) / 4 + 0.125, dim=-1, descending=True)[0].cuda()
        want, widx = t.sort(t.cat([a, b], -1), dim=-1, stable=True, descending=True)
        got, idx = rsx.merge(a, b, descending=True, return_index=True)
        assert got.shape == want.shape and idx.dtype == t.int64
        assert t.equal(got, want) and t.equal(idx, widx)
        assert t.equal(rsx.merge(a, b, descending=True), want)
    # non-contiguous and misaligned inputs are copied first
    base = t.sort(t.randint(0, 1000, (4, 101), generator=g).to(t.int32), dim=-1)[0].cuda()
    a, b = base[:, 1:61], base[:, 61:]
    assert t.equal(rsx.merge(a, b), t.sort(t.cat([a, b], -1), dim=-1, stable=True)[0])


def test_segmented_merge_with_payloads(rsx):
    t = _torch()
    rng = np.random.default_rng(1200)
    a, aoff, b, boff = ragged_inputs(np.int64, rng)
    pa, pb = payloads(a.size, b.size, rng)
    dv = lambda x: t.from_numpy(x).cuda()
    keys, ooff, pay, idx = rsx.segmented_merge(dv(a), dv(aoff), dv(b), dv(boff), payload_a=dv(pa.view(np.int32)), payload_b=dv(pb.view(np.int32)),
                                               return_index=True)
    rk, ri, rooff = merge_oracle(a, aoff, b, boff)
    total = int(rooff[-1])
    assert keys.numel() == a.size + b.size and idx.dtype == t.int64 and ooff.dtype == t.int64
    assert np.array_equal(ooff.cpu().numpy(), rooff)
    assert np.array_equal(keys.cpu().numpy()[:total], rk) and not keys[total:].any()
    assert np.array_equal(idx.cpu().numpy()[:total], ri) and bool((idx[total:] == -1).all())
    assert np.array_equal(pay.cpu().numpy().view(np.uint32)[:total], gather(ri, rooff, aoff, boff, pa, pb)) and not pay[total:].any()
    res = rsx.segmented_merge(dv(a), dv(aoff), dv(b), dv(boff))
    assert len(res) == 2 and t.equal(res[0], keys)


def test_helper_errors(rsx):
    t = _torch()
    a, b = t.arange(10, dtype=t.int32, device="cuda"), t.arange(5, dtype=t.int32, device="cuda")
    off = t.tensor([0, 5], dtype=t.int64, device="cuda")
    with pytest.raises(TypeError):
        rsx.merge(a, b.to(t.int64))
    for bad in (t.float16, t.bfloat16, t.bool):
        with pytest.raises(TypeError):
            rsx.merge(a.to(bad), b.to(bad))
    with pytest.raises(ValueError):
        rsx.merge(a.cpu(), b.cpu())
    with pytest.raises(ValueError):
        rsx.merge(a, b, payload_a=a)
    with pytest.raises(ValueError):
        rsx.segmented_merge(a, off, b, off, payload_b=b)
    with pytest.raises(ValueError):
        rsx.segmented_merge(a, off, b, None)
    with pytest.raises(ValueError):
        rsx.merge(a.reshape(2, 5), b)


def test_sort_rows_twice_then_merge(rsx):
    t = _torch()
    g = t.Generator().manual_seed(13)
    for dt in (t.float32, t.int64):
        x = t.randint(-1000, 1000, (37, 300), generator=g).to(dt).cuda()
        y = t.randint(-1000, 1000, (37, 211), generator=g).to(dt).cuda()
        if dt.is_floating_point:
            x[:, ::7] = -0.0
            y[:, ::5] = float("nan")
            y[:, 1::9] = 0.0
        merged = rsx.merge(rsx.sort_rows(x)[0], rsx.sort_rows(y)[0])
        want = rsx.sort_rows(t.cat([x, y], -1))[0]
        bits = lambda v: v.contiguous().view(t.int32 if v.element_size() == 4 else t.int64)
        assert t.equal(bits(merged), bits(want))
