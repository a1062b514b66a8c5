"""Search in sorted segments (rsx_segmented_search, radix_sort_amd.searchsorted / bucketize / segmented_searchsorted) on the GPU.

The referee is tests/_search_ref.py; every comparison is exact integer equality with search_oracle.  The output starts out holding a
sentinel that must survive outside [qoff[0], qoff[S]) and ends in a guard band.  Every engine here has capacity 4096: the search is not
bound by it.  Which path a tile takes is computed from the layout by _search_ref.tile_paths, the rule written at the top of rsx_search.hpp.
"""
import ctypes as C
import os

import numpy as np
import pytest

import _search_ref as R
from _search_ref import extremes, neighbours, order_map, sample_positions, search_oracle, sort_engine_order, tile_paths
from test_gpu_segmented import _torch, dev, offsets_from
from test_gpu_unique import FILL, FILL32, GUARD
from test_search import HEADER_DTYPES as DTYPES
from test_search import LENGTHS, drawn_counts, pooled_queries, ragged_case, random_keys

pytestmark = pytest.mark.gpu

CAP = 4096


def engine(rsx, dt, descending=False, stream=None, sampled=True):
    """sampled=False: RSX_SEARCH_SAMPLED=0 (read at rsx_create): tiles inside one long segment bisect global memory from the first level"""
    if not sampled:
        os.environ["RSX_SEARCH_SAMPLED"] = "0"
    try:
        eng = rsx.Engine(dt, CAP, descending=descending)
    finally:
        os.environ.pop("RSX_SEARCH_SAMPLED", None)
    if stream is not None:
        eng.set_stream(stream)
    return eng


def run(rsx, keys, off, queries, qoff, right=False, descending=False, eng=None):
    """One rsx_segmented_search through the Engine API; the output is pre-filled with the sentinel and followed by a guard band.  Returns
    (the uint32 output, engine)."""
    t = _torch()
    n, nq = keys.size, queries.size
    nseg = 1 if off is None else len(off) - 1
    k = dev(t, keys) if n else None
    q = dev(t, queries)
    o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
    qo = None if qoff is None else dev(t, np.asarray(qoff, dtype=np.uint64))
    out = dev(t, np.concatenate([np.full(4 * nq, FILL, dtype=np.uint8), np.full(GUARD, 0xA5, dtype=np.uint8)]))
    if eng is None:
        eng = engine(rsx, keys.dtype, descending)
    eng.segmented_search(None if k is None else k.data_ptr(), n, None if o is None else o.data_ptr(), nseg, q.data_ptr(), nq,
                         None if qo is None else qo.data_ptr(), out.data_ptr(), right=right)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    b = out.cpu().numpy().view(np.uint8)
    assert np.all(b[4 * nq:] == 0xA5), "guard band written"
    return b[:4 * nq].copy().view(np.uint32), eng


def check(got, want, what=""):
    """exact equality with the referee; the sentinel where the referee holds -1 (outside [qoff[0], qoff[S]))"""
    want = np.where(want < 0, FILL32, want).astype(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: differ at {bad[:8].tolist()} (of {bad.size}): {got[bad[:8]].tolist()} != {want[bad[:8]].tolist()}"


def both_sides(rsx, keys, off, queries, qoff, descending=False, eng=None, what=""):
    eng = eng or engine(rsx, keys.dtype, descending)
    res = []
    for right in (False, True):
        got, _ = run(rsx, keys, off, queries, qoff, right, descending, eng)
        check(got, search_oracle(keys, off, queries, qoff, right, descending), f"{what} right={right}")
        res.append(got)
    eng.sync()
    return res


# -- 1. lengths and query counts: the six dtypes x both directions x both sides --------------------------------------------------------------

@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_lengths_and_query_counts(rsx, dt, descending):
    rng = np.random.default_rng(100 + DTYPES.index(dt) * 2 + int(descending))
    keys, off = ragged_case(dt, rng, descending)
    eng = engine(rsx, dt, descending)
    # query counts drawn from the list: tiles inside one segment, ending on a boundary, spanning many
    counts = drawn_counts(rng, len(LENGTHS))
    queries, qoff = pooled_queries(keys, off, rng, counts)
    paths = tile_paths(keys.size, off, queries.size, qoff)
    assert "direct" in paths and ("resident" in paths or "sampled" in paths)
    both_sides(rsx, keys, off, queries, qoff, descending, eng, "drawn counts")
    # every key of every segment, its neighbours, the extremes and random absent values
    queries, qoff = pooled_queries(keys, off, rng)
    assert {"resident", "sampled", "direct"} <= set(tile_paths(keys.size, off, queries.size, qoff))
    both_sides(rsx, keys, off, queries, qoff, descending, eng, "every key")


# -- 2. duplicates -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [np.uint32, np.int64, np.float32], ids=lambda d: np.dtype(d).name)
def test_duplicates(rsx, dt):
    rng = np.random.default_rng(200)
    eng = engine(rsx, dt)
    for L in (4097, (1 << 20) + 3):
        keys = np.full(L, 77, dtype=dt)
        base = neighbours(keys[:1])                                               # the key, the one before, the one after
        for queries in (base, np.tile(base, 700)):                                # direct; then more than a tile: sampled
            lo, hi = both_sides(rsx, keys, None, queries, None, eng=eng, what=f"all equal, {L}")
            assert lo[:3].tolist() == [0, 0, L] and hi[:3].tolist() == [L, 0, L]
    # 2^8 distinct values in 2^20 + 3 keys: every run is longer than the sample stride of 1024
    L = (1 << 20) + 3
    vals = sort_engine_order(random_keys(dt, 256, rng))
    keys = sort_engine_order(vals[rng.integers(0, 256, L)])
    queries = np.concatenate([neighbours(vals), extremes(dt), random_keys(dt, 1800, rng)])
    assert set(tile_paths(L, None, queries.size, None)) == {"sampled"}
    lo, hi = both_sides(rsx, keys, None, queries, None, eng=eng, what="256 distinct values")
    assert int((hi - lo).max()) > 1024
    both_sides(rsx, keys, None, queries, None, eng=engine(rsx, dt, sampled=False), what="256 distinct values, direct")


# -- 3. the sampled path's edges -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [4097, 8191, 1024 * 1025 - 1, 1024 * 1025, (1 << 20) + 3])
def test_sampled_path_edges(rsx, L):
    rng = np.random.default_rng(L)
    for dt, keys in ((np.uint32, (np.arange(L, dtype=np.uint64) * 3 + 5).astype(np.uint32)),                       # distinct, with gaps
                     (np.uint64, np.sort(rng.integers(0, L // 2, L).astype(np.uint64) << np.uint64(33)))):         # duplicates at the samples
        p = sample_positions(L).astype(np.int64)
        assert p[0] == 0 and p[-1] < L and np.all(np.diff(p) >= 4)
        at = np.concatenate([p, np.maximum(p - 1, 0), np.minimum(p + 1, L - 1), [L - 1]])
        queries = np.concatenate([neighbours(keys[at]), extremes(dt)])
        assert queries.size > 9 * R.TILE_Q and set(tile_paths(L, None, queries.size, None)[:-1]) == {"sampled"}
        eng = engine(rsx, dt)
        both_sides(rsx, keys, None, queries, None, eng=eng, what=f"sampled {L}")
        # the same inside a ragged call: the long segment between two short ones, its queries not on the tile grid
        off = offsets_from([7, L, 100], start=1)
        k3 = np.concatenate([keys[-1:], keys[:7], keys, keys[:100], keys[:2]])
        q3 = np.concatenate([queries[:301], queries, queries[:50]])
        qoff = offsets_from([300, queries.size, 50], start=1)
        assert "sampled" in tile_paths(k3.size, off, q3.size, qoff)
        both_sides(rsx, k3, off, q3, qoff, eng=eng, what=f"sampled {L}, ragged")
    both_sides(rsx, keys, None, queries, None, eng=engine(rsx, dt, sampled=False), what=f"direct {L}")


# -- 4. the resident path with unaligned segment starts -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [np.uint32, np.uint64, np.float32], ids=lambda d: np.dtype(d).name)
def test_resident_unaligned_starts(rsx, dt):
    rng = np.random.default_rng(400)
    lengths = [5, 4096, 1021, 3, 2000, 4095, 1, 2, 6, 0, 4090]
    keys, off = ragged_case(dt, rng, False, lengths, start=1, tail=9)
    vec = 16 // np.dtype(dt).itemsize
    assert {int(o) % vec for o in off[:-1]} == set(range(vec)) and int(off[0]) > 0 and int(off[-1]) < keys.size
    # one whole tile of queries per segment: every tile is resident
    parts = [rng.permutation(np.concatenate([neighbours(keys[int(off[s]):int(off[s + 1])]), extremes(dt), random_keys(dt, 1024, rng)]))[:R.TILE_Q] for s in range(len(lengths))]
    queries = np.concatenate(parts)
    assert set(tile_paths(keys.size, off, queries.size, None)) == {"resident"}
    both_sides(rsx, keys, off, queries, None, what="resident, even form")
    qoff = np.arange(len(lengths) + 1, dtype=np.uint64) * R.TILE_Q
    both_sides(rsx, keys, off, queries, qoff, what="resident, ragged form")


# -- 5. the even form against the ragged form --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Q", [1, 16, 4096])
@pytest.mark.parametrize("cols", [1, 4096, 50257])
def test_even_form_equals_ragged_form(rsx, cols, Q):
    rng = np.random.default_rng(cols + Q)
    S = 3 if Q == 4096 else 40 if cols == 50257 else 1500 if Q == 1 else 200
    for dt, descending in ((np.uint32, False), (np.float32, True)):
        rows = random_keys(dt, S * cols, rng).reshape(S, cols)
        keys = np.concatenate([sort_engine_order(r, descending) for r in rows])
        own = keys.reshape(S, cols)[:, rng.integers(0, cols, Q)]                  # keys of the row itself, and random ones
        queries = np.where(rng.integers(0, 2, (S, Q)) == 0, own, random_keys(dt, S * Q, rng).reshape(S, Q)).astype(dt).reshape(-1)
        off = np.arange(S + 1, dtype=np.uint64) * cols
        qoff = np.arange(S + 1, dtype=np.uint64) * Q
        eng = engine(rsx, dt, descending)
        for right in (False, True):
            even, _ = run(rsx, keys, off, queries, None, right, descending, eng)
            ragged, _ = run(rsx, keys, off, queries, qoff, right, descending, eng)
            assert np.array_equal(even, ragged)
            check(even, search_oracle(keys, off, queries, None, right, descending), f"{S} x {cols}, {Q} per row")
        eng.sync()


# -- 6. floats: what sort_rows leaves, searched for the special values ---------------------------------------------------------------------------

@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_float_specials_after_sort_rows(rsx, dt, descending):
    t = _torch()
    rng = np.random.default_rng(600 + int(descending))
    rows, cols = 6, 5000
    x = random_keys(dt, rows * cols, rng).reshape(rows, cols)
    special = extremes(dt)                                                        # ±NaN, ±inf, ±0, ...
    x[:, :special.size * 3] = np.tile(special, 3)                                 # every row holds each of them three times
    x = rng.permuted(x, axis=1)
    values, _ = rsx.sort_rows(dev(t, x).view(getattr(t, np.dtype(dt).name)), descending=descending)
    keys = values.cpu().numpy().reshape(-1)
    assert np.array_equal(keys.view(R.UINT[keys.itemsize]), np.concatenate([sort_engine_order(r, descending) for r in x]).view(R.UINT[keys.itemsize]))
    per_row = np.concatenate([special, neighbours(special), random_keys(dt, 300, rng)])
    queries = np.tile(per_row, rows)
    off = np.arange(rows + 1, dtype=np.uint64) * cols
    lo, hi = both_sides(rsx, keys, off, queries, None, descending, what="specials")
    u = R.UINT[keys.itemsize]
    times = np.array([int(np.sum(x[0].view(u) == b)) for b in special.view(u)])  # equal by bits: -0.0 and +0.0, the NaNs, are keys of their own
    assert np.all(times >= 3) and np.array_equal((hi - lo)[:special.size], times)
    # and through the helper, on the tensor sort_rows returned
    q = dev(t, per_row).view(values.dtype).repeat(rows, 1)
    for right in (False, True):
        got = rsx.searchsorted(values, q, right=right, descending=descending)
        assert got.dtype == t.int64 and np.array_equal(got.cpu().numpy().reshape(-1), search_oracle(keys, off, queries, None, right, descending))


# -- 7. several tiles per workgroup ------------------------------------------------------------------------------------------------------------

def test_several_tiles_per_workgroup(rsx):
    """The launch rule (capi_search.inc): tiles per workgroup = ceil(tiles / (16 * CUs)), so a workgroup walks two tiles from
    16 * CUs + 1 tiles on.  64-bit keys; a resident, a sampled and many small segments, so that a workgroup keeps and drops what it staged."""
    t = _torch()
    cus = t.cuda.get_device_properties(0).multi_processor_count
    nq = R.TILE_Q * 16 * cus + 5
    rng = np.random.default_rng(7)
    small = [int(v) for v in rng.integers(0, 300, 2000)]
    lengths = [3000, 100000] + small + [4096]
    keys, off = ragged_case(np.uint64, rng, False, lengths, start=2)
    rest = nq - 10 - 2 * 1000000 - 2000 * 50
    qcounts = [1000000, 1000000] + [50] * 2000 + [rest]
    pools = [keys[int(off[s]):int(off[s + 1])] for s in range(len(lengths))]
    parts = [np.where(rng.integers(0, 2, c) == 0, (p if p.size else keys[:1])[rng.integers(0, max(p.size, 1), c)], random_keys(np.uint64, c, rng))
             for p, c in zip(pools, qcounts)]
    queries = np.concatenate([keys[:3]] + parts + [keys[:7]]).astype(np.uint64)
    qoff = offsets_from(qcounts, start=3)
    assert queries.size == nq and -(-((nq + R.TILE_Q - 1) // R.TILE_Q) // (16 * cus)) == 2
    assert {"resident", "sampled", "direct"} <= set(tile_paths(keys.size, off, nq, qoff))
    both_sides(rsx, keys, off, queries, qoff, what="two tiles per workgroup")


# -- 8. errors ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["off", "qoff"])
@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_write_nothing_and_are_reported_once(rsx, bad, which):
    rng = np.random.default_rng(23)
    n, nq = 40000, 30000
    keys = np.sort(rng.integers(0, 1 << 32, n, dtype=np.uint32))
    queries = rng.integers(0, 1 << 32, nq, dtype=np.uint32)
    good_off = np.array([0, 100, 5000, 5000, n], dtype=np.uint64)
    good_qoff = np.array([0, 3, 5000, 25000, nq], dtype=np.uint64)
    size = n if which == "off" else nq
    broken = np.array([0, 100, 5000, 4000 if bad == "decreasing" else size + 1, size], dtype=np.uint64)       # segment 2 is the first bad one
    off, qoff = (broken, good_qoff) if which == "off" else (good_off, broken)
    eng = engine(rsx, np.uint32)
    got, _ = run(rsx, keys, off, queries, qoff, eng=eng)
    assert np.all(got == FILL32), "a call with bad offsets wrote something"
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "segment 2 " in str(ei.value)
    eng.sync()                                                                   # reported once
    keys[:] = np.concatenate([np.sort(keys[int(a):int(b)]) for a, b in zip(good_off[:-1], good_off[1:])])
    both_sides(rsx, keys, good_off, queries, good_qoff, eng=eng, what="after bad offsets")      # the engine stays usable


def test_refusals(rsx):
    t = _torch()
    n, nq = 3 * 4096, 2048
    eng = rsx.Engine(np.uint32, n, payload=True)
    keys = t.arange(n + 4, dtype=t.int32, device="cuda")
    qs = t.arange(nq + 4, dtype=t.int32, device="cuda")
    out = t.full((nq + 4,), -7, dtype=t.int32, device="cuda")
    off = t.tensor([0, n, n, n], dtype=t.int64, device="cuda")
    qoff = t.tensor([0, nq, nq, nq], dtype=t.int64, device="cuda")
    lib = rsx.load_library()
    base = dict(d_sorted=keys.data_ptr(), n=n, d_offsets=off.data_ptr(), num_segments=1, d_queries=qs.data_ptr(), num_queries=nq,
                d_query_offsets=qoff.data_ptr(), d_index_out=out.data_ptr())
    ok = lambda **kw: eng.segmented_search(**{**base, **kw})
    e0, e1 = eng.result_device()
    for kw in (dict(d_sorted=keys.data_ptr() + 4),                               # keys not 16-byte aligned
               dict(d_sorted=None),                                              # what is required
               dict(d_queries=None), dict(d_index_out=None),
               dict(d_queries=qs.data_ptr() + 2),                                # not aligned to the element
               dict(d_index_out=out.data_ptr() + 2),
               dict(d_offsets=off.data_ptr() + 4), dict(d_query_offsets=qoff.data_ptr() + 4),
               dict(d_index_out=keys.data_ptr()),                                # the output on the keys,
               dict(d_index_out=qs.data_ptr()), dict(d_index_out=qs.data_ptr() + 4 * (nq - 1)),      # the queries,
               dict(d_index_out=off.data_ptr() - 8), dict(d_index_out=qoff.data_ptr() + 8),           # the offsets
               dict(d_index_out=e0), dict(d_sorted=e0), dict(d_queries=e0), dict(d_queries=e1)):      # anything on the engine's own buffers
        with pytest.raises(rsx.RadixSortError) as ei:
            ok(**kw)
        assert ei.value.status == 1 and "rsx_segmented_search" in str(ei.value), kw
    with rsx.Engine(np.uint64, CAP) as e64:
        with pytest.raises(rsx.RadixSortError) as ei:                            # 64-bit queries on a 4-byte boundary
            e64.segmented_search(**{**base, "n": n // 2, "num_queries": nq // 4, "d_queries": qs.data_ptr() + 4})
        assert ei.value.status == 1
    for kw in (dict(d_offsets=None),                                             # query offsets without haystack offsets
               dict(num_segments=3, d_query_offsets=None, num_queries=nq - 1),   # the even form with a remainder
               dict(n=(1 << 31) + 1), dict(num_queries=(1 << 31) + 1),
               dict(num_segments=(1 << 32) - 1)):
        with pytest.raises(rsx.RadixSortError) as ei:
            ok(**kw)
        assert ei.value.status == 4 and "rsx_segmented_search" in str(ei.value), kw
    P = C.c_void_p
    for flags in (1, 2, 3, 5, 8, 1 << 31):                                       # unknown flag bits: those of the unique and the scan included
        assert lib.rsx_segmented_search(eng._h, P(keys.data_ptr()), n, P(off.data_ptr()), 1, P(qs.data_ptr()), nq, P(qoff.data_ptr()), flags,
                                        P(out.data_ptr())) == 4
        assert b"rsx_segmented_search" in lib.rsx_last_error()
    assert lib.rsx_segmented_search(None, P(keys.data_ptr()), n, None, 1, P(qs.data_ptr()), nq, None, 0, P(out.data_ptr())) == 4
    # no queries and no segments: nothing is launched
    ok(num_queries=0)
    ok(num_segments=0)
    ok(num_queries=0, d_queries=None, d_index_out=None, d_offsets=None, d_query_offsets=None)
    eng.sync()
    assert bool((out == -7).all()), "a refused call wrote something"
    ok()                                                                         # and the call these were variations of works,
    eng.sync()
    assert out[:nq].tolist() == list(range(nq)) and out[nq:].tolist() == [-7] * 4
    ok(n=0, d_sorted=None, d_offsets=None, d_query_offsets=None, right=True)     # an empty haystack too: every result is 0
    eng.sync()
    assert out[:nq].tolist() == [0] * nq and out[nq:].tolist() == [-7] * 4


# -- 9. a haystack that is not sorted -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [np.uint32, np.float64], ids=lambda d: np.dtype(d).name)
def test_unsorted_haystack_stays_in_range(rsx, dt):
    rng = np.random.default_rng(900)
    lengths = LENGTHS + [100000, 4000]
    off = offsets_from(lengths, start=3)
    keys = random_keys(dt, int(off[-1]) + 5, rng)
    counts = drawn_counts(rng, len(LENGTHS)) + [3000, 3000]
    queries, qoff = pooled_queries(keys, off, rng, counts)
    assert {"resident", "sampled", "direct"} <= set(tile_paths(keys.size, off, queries.size, qoff))
    limit = np.concatenate([[-1, -1], np.repeat(np.diff(off.astype(np.int64)), counts), [-1, -1, -1]])
    for descending in (False, True):
        eng = engine(rsx, dt, descending)
        for right in (False, True):
            got, _ = run(rsx, keys, off, queries, qoff, right, descending, eng)
            inside = limit >= 0
            assert np.all(got[~inside] == FILL32) and np.all(got[inside].astype(np.int64) <= limit[inside])
        eng.sync()


# -- 10. engine state ----------------------------------------------------------------------------------------------------------------------------

def test_sort_state_is_untouched_and_n_exceeds_capacity(rsx):
    t = _torch()
    rng = np.random.default_rng(61)
    eng = rsx.Engine(np.uint32, CAP)
    x = rng.integers(0, 1 << 32, CAP, dtype=np.uint32)
    xd = dev(t, x)
    eng.sort_from(xd.data_ptr(), CAP)
    keys, off = ragged_case(np.uint32, rng)
    assert keys.size > 10 * CAP
    queries, qoff = pooled_queries(keys, off, rng, drawn_counts(rng, len(LENGTHS)))
    both_sides(rsx, keys, off, queries, qoff, eng=eng, what="on an engine that holds a sort's result")
    assert eng.geometry().num_keys == CAP
    out = t.zeros(CAP, dtype=t.int32, device="cuda")
    eng.copy_result(out.data_ptr())
    eng.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.sort(x))


def test_capture_and_replay(rsx):
    """every launch is sized from n, the segment count and the query count: one captured call is replayed on new keys, queries and offsets"""
    t = _torch()
    rng = np.random.default_rng(70)
    dt = np.int32
    keys, off = ragged_case(dt, rng)
    counts = drawn_counts(rng, len(LENGTHS))
    queries, qoff = pooled_queries(keys, off, rng, counts)
    n, nq, nseg = keys.size, queries.size, len(LENGTHS)
    side = t.cuda.Stream()
    eng = engine(rsx, dt, stream=side.cuda_stream)
    kd, qd, od, qod = dev(t, keys), dev(t, queries), dev(t, off), dev(t, qoff)
    out = dev(t, np.full(nq * 4, FILL, dtype=np.uint8))

    def call():
        eng.segmented_search(kd.data_ptr(), n, od.data_ptr(), nseg, qd.data_ptr(), nq, qod.data_ptr(), out.data_ptr(), right=True)

    call()                                                                       # eager: the first call of an engine allocates its status words
    eng.sync()
    check(out.cpu().numpy().view(np.uint32), search_oracle(keys, off, queries, qoff, True), "eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for rep in range(2):
        lens = [int(v) for v in rng.permutation(LENGTHS)]
        keys, off = ragged_case(dt, rng, False, lens, start=rep, tail=8 - rep)    # same n and segment count
        perm = [int(c) for c in rng.permutation(counts)]
        queries, qoff = pooled_queries(keys, off, rng, perm)                      # same query count
        assert keys.size == n and queries.size == nq
        kd.copy_(t.from_numpy(keys.view(np.int32)))
        qd.copy_(t.from_numpy(queries.view(np.int32)))
        od.copy_(t.from_numpy(off.view(np.int64)))
        qod.copy_(t.from_numpy(qoff.view(np.int64)))
        out.fill_(FILL - 256)
        graph.replay()
        t.cuda.synchronize()
        check(out.cpu().numpy().view(np.uint32), search_oracle(keys, off, queries, qoff, True), f"replay {rep}")
    del graph
    eng.sync()


# -- 11. the torch helpers -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["int32", "int64", "float32", "float64"])
def test_searchsorted_and_bucketize_match_torch(rsx, name):
    t = _torch()
    dt = getattr(t, name)
    g = t.Generator(device="cuda").manual_seed(11)
    draw = lambda *shape: (t.randint(-2000, 2000, shape, device="cuda", generator=g).to(dt) if not dt.is_floating_point
                           else t.randn(shape, device="cuda", generator=g, dtype=dt).round(decimals=2) + 0.0)
    seq1 = t.sort(draw(5000)).values
    seq3 = t.sort(draw(3, 4, 700), dim=-1).values
    v1, v3 = draw(7, 13, 11), draw(3, 4, 50)
    for right in (False, True):
        for i32 in (False, True):
            want = t.searchsorted(seq1, v1, right=right, out_int32=i32)
            got = rsx.searchsorted(seq1, v1, right=right, out_int32=i32)
            assert got.dtype == want.dtype and got.shape == want.shape and t.equal(got, want)
            want = t.searchsorted(seq3, v3, right=right, out_int32=i32)
            got = rsx.searchsorted(seq3, v3, right=right, out_int32=i32)
            assert got.dtype == want.dtype and got.shape == want.shape and t.equal(got, want)
            want = t.bucketize(v1, seq1, right=right, out_int32=i32)
            got = rsx.bucketize(v1, seq1, right=right, out_int32=i32)
            assert got.dtype == want.dtype and t.equal(got, want)
        side = "right" if right else "left"
        assert t.equal(rsx.searchsorted(seq1, v1, side=side), t.searchsorted(seq1, v1, side=side))
        assert t.equal(rsx.searchsorted(seq1, v1, right=right, side="right"), t.searchsorted(seq1, v1, side="right"))
    # a Python scalar; non-contiguous and misaligned inputs
    s = 3 if not dt.is_floating_point else 0.25
    assert t.equal(rsx.searchsorted(seq1, s), t.searchsorted(seq1, s)) and t.equal(rsx.bucketize(s, seq1, right=True), t.bucketize(s, seq1, right=True))
    wide = t.sort(draw(6, 1001), dim=-1).values
    assert t.equal(rsx.searchsorted(wide[:, 1:], v1[:6, :, 0]), t.searchsorted(wide[:, 1:].contiguous(), v1[:6, :, 0].contiguous()))
    assert t.equal(rsx.searchsorted(seq1[1:], v1.transpose(0, 2)), t.searchsorted(seq1[1:], v1.transpose(0, 2).contiguous()))
    assert t.equal(rsx.searchsorted(seq1[::2], v1), t.searchsorted(seq1[::2].contiguous(), v1))
    # descending rows, and the ragged helper against the referee
    desc = t.sort(draw(4, 900), dim=-1, descending=True).values
    q = draw(4, 33)
    want = search_oracle(desc.cpu().numpy().reshape(-1), np.arange(5, dtype=np.uint64) * 900, q.cpu().numpy().reshape(-1), None, False, True)
    assert np.array_equal(rsx.searchsorted(desc, q, descending=True).cpu().numpy().reshape(-1), want)
    off = t.tensor([0, 0, 1200, 5000], dtype=t.int64, device="cuda")
    seg = t.cat([t.sort(seq1[:1200]).values, t.sort(seq1[1200:]).values])
    vals, voff = draw(100), t.tensor([0, 10, 60, 100], dtype=t.int64, device="cuda")
    got = rsx.segmented_searchsorted(seg, off, vals, voff, right=True)
    want = search_oracle(seg.cpu().numpy(), off.cpu().numpy().astype(np.uint64), vals.cpu().numpy(), voff.cpu().numpy().astype(np.uint64), True)
    assert got.dtype == t.int64 and np.array_equal(got.cpu().numpy(), want)
    assert rsx.searchsorted(seq1[:0], v1).eq(0).all() and rsx.searchsorted(seq1, v1[:0]).shape == v1[:0].shape


def test_top_p_chain(rsx):
    """sort_rows -> cumsum -> searchsorted, the README's example, on 64 x 50257 float32: equal to the referee on this library's own cdf on
    every row, and to the same chain in torch on the rows where the two cumsums agree bitwise.  This library's cumsum adds in a fixed tree
    order, so where the terms fall below an ulp of the sum (the tail of sorted probabilities) a row may step down by an ulp and is then
    not strictly a sorted haystack; with one query per row the tile takes the direct path, whose bisection probes the midpoints
    np.searchsorted probes, so the two agree there as well.  The running maximum of the cdf is sorted by construction: on it every row
    equals the referee and torch, on both sides."""
    t = _torch()
    g = t.Generator(device="cuda").manual_seed(5)
    rows, cols = 64, 50257
    logits = t.randn((rows, cols), device="cuda", generator=g) * 3
    p = t.rand((rows, 1), device="cuda", generator=g) * 0.98 + 0.01
    probs, _ = rsx.sort_rows(t.softmax(logits, dim=-1), descending=True)
    cdf = rsx.cumsum(probs, dim=-1)
    cut = rsx.searchsorted(cdf, p)
    off = np.arange(rows + 1, dtype=np.uint64) * cols
    host, ph = cdf.cpu().numpy(), p.cpu().numpy().reshape(-1)
    got = cut.cpu().numpy().reshape(-1)
    assert tile_paths(rows * cols, off, rows, None) == ["direct"]
    is_sorted = np.all(np.diff(host, axis=1) >= 0, axis=1)
    want = search_oracle(host.reshape(-1), off, ph, None)
    tcdf = t.cumsum(t.sort(t.softmax(logits, dim=-1), dim=-1, descending=True).values, dim=-1)
    same = (tcdf.view(t.int32) == cdf.view(t.int32)).all(dim=1).cpu().numpy()
    tcut = t.searchsorted(tcdf, p).cpu().numpy().reshape(-1)
    print(f"top-p: {int(is_sorted.sum())} of {rows} cdf rows are sorted, {int(same.sum())} have torch's bits; "
          f"{int((got != want).sum())} cuts differ from the referee, {int((got != tcut)[same].sum())} from torch on those rows")
    assert cut.shape == (rows, 1) and cut.dtype == t.int64
    assert np.array_equal(got, want)
    assert np.array_equal(got[same], tcut[same])
    mono = t.cummax(cdf, dim=-1).values
    for right in (False, True):
        cut = rsx.searchsorted(mono, p, right=right)
        assert t.equal(cut, t.searchsorted(mono, p, right=right))
        assert np.array_equal(cut.cpu().numpy().reshape(-1), search_oracle(mono.cpu().numpy().reshape(-1), off, ph, None, right))
