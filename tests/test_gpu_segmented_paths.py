"""rsx_segmented_sort on the paths of rsx_segmented.hpp and capi_segmented.inc that tests/test_gpu_segmented.py never reaches: block
prefixes of the classify scan with more than 256 classify blocks (large segments, and bad ones, deep in the list); the grid stride of
the LDS sorts of classes 1 and 2 (a long segment, then a shorter one over its stale image); ranking rounds with one digit, with digits
on the 7 / 8 boundary only, and with real keys that equal the pad key; chain tiles of one key, whole tiles, large segments meeting
mid-tile, nlarge == max_large; a payload engine that sorts small shapes after larger ones, with a flat sort and a unique in between;
a captured call replayed over other keys, offsets and class mixes; offsets that fold back, where the scan switches the chain off.

The layouts are held in tests/_segmented_ref.py (tests/test_segmented.py checks on the CPU, at 256 CUs, that each reaches its path);
the tests whose path depends on the CU count assert it again with the device's own.  run / check / seg_oracle, sentinels and guard
bands are those of test_gpu_segmented.py: every comparison is exact equality of bits, keys and payload (payload = input index: the
stable argsort), and the sentinel at every position no valid segment covers.
"""
import numpy as np
import pytest

import _segmented_ref as S
from test_gpu_float_keys import UINT, random_bits
from test_gpu_float_keys import oracle as flat_oracle
from test_gpu_segmented import _torch, check, dev, host, run, seg_oracle, sentinel_keys, sentinel_payload
from test_gpu_unique import check as uniq_check
from test_gpu_unique import run as uniq_run

pytestmark = pytest.mark.gpu


def device_cus():
    return int(_torch().cuda.get_device_properties(0).multi_processor_count)


def check_many(x, off, got_k, got_p, descending, payload=True):
    """check() of test_gpu_segmented.py with the covered positions from S.covered (no Python loop over 600000 segments)"""
    want = seg_oracle(x, off, x.size, descending)
    inside = S.covered(off, x.size)
    u = UINT[x.dtype]
    bad = np.flatnonzero(got_k.view(u) != np.where(inside, x[want].view(u), sentinel_keys(x)))
    assert bad.size == 0, f"keys differ at {bad[:8]} (of {bad.size})"
    if payload:
        badp = np.flatnonzero(got_p != np.where(inside, want.astype(np.uint32), sentinel_payload(x.size)))
        assert badp.size == 0, f"payload differs at {badp[:8]} (of {badp.size})"


def with_ties(dtype, n, rng):
    x = random_bits(dtype, n, rng)
    x[rng.integers(0, n, n // 3)] = x[rng.integers(0, n, n // 3)]
    return x


# -- 1. sparse large segments over many classify blocks --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,descending", [(np.uint32, False), (np.uint64, True)], ids=["uint32-asc", "uint64-desc"])
def test_large_segments_across_classify_blocks(rsx, dtype, descending):
    """S.sparse_large: 293 classify blocks, two per scan thread; large segments in some 40 of them, the last one included: dest and tstart[]
    of almost every large segment depend on a non-zero block prefix"""
    n, off = S.sparse_large()
    g = S.seg_geometry(off, n, device_cus())
    print(n, S.summary(g))
    assert g["per"] == 2 and g["large_blocks"] >= 30 and g["last_large_block"] == g["nblocks"] - 1 and g["chain_ok"] == 1
    rng = np.random.default_rng(31 + descending)
    x = with_ties(dtype, n, rng)
    k, p, eng = run(rsx, x, off, descending, True)
    eng.sync()
    check_many(x, off, k, p, descending)


# -- 2. bad segments deep in the list --------------------------------------------------------------------------------------------------------

def test_bad_segments_beyond_the_first_scan_block(rsx):
    """S.sparse_large_bad: the first bad segment (550001) is found in the second classify block of a scan thread; it is reported once,
    every valid segment is sorted (the large ones after the spikes too), the bad ranges keep the sentinel, the engine stays usable"""
    n, off = S.sparse_large_bad()
    g = S.seg_geometry(off, n, device_cus())
    print(n, S.summary(g))
    assert g["first_bad"] == 550001 and g["per"] == 2 and g["chain_ok"] == 1 and g["large"].max() == 599999
    rng = np.random.default_rng(37)
    x = with_ties(np.uint32, n, rng)
    eng = rsx.Engine(np.uint32, n, payload=True)
    k, p, _ = run(rsx, x, off, False, True, eng=eng)
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "segment 550001 " in str(ei.value)
    eng.sync()                                                               # reported once
    inside = S.covered(off, n)
    for s in (550001, 580000):
        assert not inside[int(off[s]):int(S.sparse_large()[1][s + 2])].any()
    check_many(x, off, k, p, False)
    _, good = S.sparse_large()
    k, p, _ = run(rsx, x, good, False, True, eng=eng)
    eng.sync()
    check_many(x, good, k, p, False)


# -- 3. the grid stride of the LDS sorts of classes 1 and 2 -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,descending,payload", [(np.uint32, False, False), (np.int64, True, True), (np.float32, False, True)],
                         ids=["uint32-keys", "int64-desc-payload", "float32-payload"])
@pytest.mark.parametrize("cls", [1, 2])
def test_more_segments_than_workgroups(rsx, cls, dtype, descending, payload):
    """S.stride_layout at the device's CU count: 400 (class 1) / 200 (class 2) workgroups sort a second segment, a shorter one, after
    their first: its pads lie over the first one's image, and the counters and digit starts are reused"""
    cus = device_cus()
    n, off = S.stride_layout(cls, cus)
    g = S.seg_geometry(off, n, cus)
    print(n, S.summary(g))
    assert g["trips"][cls] >= 2 and g["count"][cls] > g["grid"][cls] == cus * S.PER_CU[cls]
    lens = np.diff(off.astype(np.int64))
    order = g["lists"][cls]
    second = np.arange(g["grid"][cls], g["count"][cls])
    assert np.all(lens[order[second]] < lens[order[second - g["grid"][cls]]])
    rng = np.random.default_rng(41 + cls)
    x = S.few_distinct(dtype, off, n, rng)
    k, p, eng = run(rsx, x, off, descending, payload)
    eng.sync()
    check_many(x, off, k, p, descending, payload)


# -- 4. one digit per pass, and pads ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype", [np.uint32, np.int64, np.float64], ids=lambda d: np.dtype(d).name)
def test_degenerate_digits_and_pad_keys(rsx, dtype, descending):
    """seg_rank on tiles whose keys share one digit, sit on the 7 / 8 and 0 / 15 boundaries only, differ in one byte only, or equal the pad
    key (the pads must rank after them by index alone), in every class and in the chain; sorted and reverse-sorted input.  The payload is
    the input index, so equal keys out of order show."""
    off = S.offsets_from(S.DIGIT_LENGTHS)
    n = int(off[-1])
    eng = rsx.Engine(dtype, n, payload=True, descending=descending)
    for i, kind in enumerate(S.DIGIT_SETS):
        rng = np.random.default_rng(50 + i)
        x = S.digit_keys(kind, dtype, off, n, rng, descending)
        k, p, _ = run(rsx, x, off, descending, True, eng=eng)
        eng.sync()
        try:
            check(x, off, k, p, descending)
        except AssertionError as e:
            raise AssertionError(f"{kind}: {e}") from None


# -- 5. the chain's tiles against the 4096-key grid -------------------------------------------------------------------------------------------

GRID_RUNS = [(np.uint32, False, True, 0), (np.int64, False, True, 8), (np.float32, True, True, 0), (np.float64, False, True, 0),
             (np.uint32, True, False, 4)]


@pytest.mark.parametrize("dtype,descending,payload,shift", GRID_RUNS, ids=["uint32", "int64-shifted", "float32-desc", "float64", "uint32-desc-keys-shifted"])
@pytest.mark.parametrize("layout", ["grid", "full_house"])
def test_tiles_against_the_grid(rsx, layout, dtype, descending, payload, shift):
    """S.grid_layout: tiles of one key at both ends of a segment, segments of whole tiles only, two large segments inside one grid tile,
    a last tile of one key at n.  S.full_house_layout: nlarge == max_large, the last rows of the chain's tables in use."""
    n, off = S.grid_layout() if layout == "grid" else S.full_house_layout()
    g = S.seg_geometry(off, n, device_cus())
    print(n, S.summary(g))
    if layout == "grid":
        assert list(zip(g["first_tile"], g["last_tile"])) == S.GRID_TILES
    else:
        assert g["nlarge"] == g["max_large"] == 37
    rng = np.random.default_rng(60 + GRID_RUNS.index((dtype, descending, payload, shift)))
    x = with_ties(dtype, n, rng)
    k, p, eng = run(rsx, x, off, descending, payload, out_shift=shift)
    eng.sync()
    check(x, off, k, p, descending, payload)


# -- 6. one payload engine, growing then shrinking --------------------------------------------------------------------------------------------

def test_one_payload_engine_across_shapes(rsx):
    """S.engine_sequence on ONE uint32 payload engine of 2^22 keys: after [1 << 22] and [4097] * 200 the small-segment list, the
    large-segment table, the tile starts and the digit table hold the larger calls' rows and keys[] / perm[] the chain's ping-pong; the
    smaller calls that follow must read none of it.  A flat sort of the engine's own upload (with its payload) runs between steps 3
    and 4, a rsx_segmented_unique with counts, first positions and inverse on the same engine between steps 4 and 5 (the binding allows
    both: the unique sorts through this very chain).  The last call is repeated: same bytes."""
    rng = np.random.default_rng(71)
    eng = rsx.Engine(np.uint32, S.ENGINE_CAPACITY, payload=True)
    last = None
    for step, (lens, start) in enumerate(S.engine_sequence()):
        off = S.offsets_from(lens, start)
        n = int(off[-1]) + (5 if step in (2, 4) else 0)
        assert n <= S.ENGINE_CAPACITY
        x = with_ties(np.uint32, n, rng)
        k, p, _ = run(rsx, x, off, False, True, eng=eng)
        eng.sync()
        check_many(x, off, k, p, False)
        last = (x, off, k, p)
        if step == 2:
            y = with_ties(np.uint32, 100003, rng)
            eng.upload(y, np.arange(y.size, dtype=np.uint32))
            eng.sort()
            eng.sync()
            ky, py = eng.download(want_perm=True)
            want = flat_oracle(y)
            assert np.array_equal(ky, y[want]) and np.array_equal(py, want.astype(np.uint32))
        if step == 3:
            uoff = S.offsets_from([0, 1, 300, 5000, 4096, 2, 9000], start=3)
            z = rng.integers(0, 50, int(uoff[-1]) + 5).astype(np.uint32)
            got, _ = uniq_run(rsx, z, uoff, eng=eng)
            eng.sync()
            uniq_check(z, uoff, got)
    x, off, k, p = last
    k2, p2, _ = run(rsx, x, off, False, True, eng=eng)
    eng.sync()
    assert k2.tobytes() == k.tobytes() and p2.tobytes() == p.tobytes()


# -- 7. capture and replay --------------------------------------------------------------------------------------------------------------------

def test_graph_capture_and_replay(rsx):
    """A warmed rsx_segmented_sort (int64 keys, payload) is captured on the engine's stream; each replay reads new keys and new offsets
    from the same buffers with another class mix: large and small, then small segments and empties only (off[0] > 0, most of the
    output left alone), then one segment of everything.  The outputs are refilled with the sentinel before each replay."""
    t = _torch()
    rng = np.random.default_rng(73)
    n, nseg = 300000, 8
    stream = t.cuda.Stream()
    eng = rsx.Engine(np.int64, n, payload=True)
    eng.set_stream(stream.cuda_stream)
    keys = t.zeros(n, dtype=t.int64, device="cuda")
    pay = dev(t, np.arange(n, dtype=np.uint32))
    offs = t.zeros(nseg + 1, dtype=t.int64, device="cuda")
    out = t.zeros(n, dtype=t.int64, device="cuda")
    pout = t.zeros(n, dtype=t.int32, device="cuda")

    def load(lens, start=0):
        assert len(lens) == nseg
        off = S.offsets_from(lens, start)
        assert int(off[-1]) <= n
        x = with_ties(np.int64, n, rng)
        keys.copy_(t.from_numpy(x))
        offs.copy_(t.from_numpy(off.astype(np.int64)))
        out.copy_(t.from_numpy(sentinel_keys(x).view(np.int64)))
        pout.copy_(t.from_numpy(sentinel_payload(n).view(np.int32)))
        t.cuda.synchronize()
        return x, off

    def call():
        eng.segmented_sort(keys.data_ptr(), n, offs.data_ptr(), nseg, out.data_ptr(), pay.data_ptr(), pout.data_ptr())

    def verify(x, off):
        check(x, off, host(out, np.int64), host(pout, np.uint32), False)

    first = load([100000, 5000, 1, 0, 150000, 300, 2000, 17])
    call()                                                                   # warm-up: scratch grows here
    stream.synchronize()
    verify(*first)
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=stream):
        call()
    second = load([300, 0, 4096, 1, 1000, 0, 17, 2], start=4099)
    graph.replay()
    t.cuda.synchronize()
    verify(*second)
    third = load([0, 0, 0, n, 0, 0, 0, 0])
    graph.replay()
    t.cuda.synchronize()
    verify(*third)
    fourth = load([4097, 0, 200000, 1, 60000, 2, 30000, 257], start=1)
    graph.replay()
    t.cuda.synchronize()
    verify(*fourth)
    eng.sync()


# -- 8. offsets that fold back ----------------------------------------------------------------------------------------------------------------

def test_folded_offsets_switch_the_chain_off(rsx):
    """[0, 5000, 0, 5000, 0, 5000] over 5000 keys: three valid large segments of 5000 keys each where the host sized seg_large for ONE
    (max_large = 5000 / 4097), seg_tstart for two entries and the table for three tiles.  Walked through seg_geometry and the kernels:
    seg_scan_kernel finds tot[SF_LARGE] = 3 > max_large, so chain_ok = nlarge = tiles = 0 and tstart[] is not written; with chain_ok
    0 seg_classify_kernel<true> writes no row of large[] / tstart[] (it only counts); there is no small segment, so the list is not
    written and the LDS sorts find count 0; seg_histogram_kernel and seg_reorder_kernel loop over hdr->tiles = 0 tiles; the table
    scan runs over the 3 * 16 allocated entries.  So nothing is stored past a buffer and no output position is written: all keep the
    sentinel.  Segment 1 ([5000, 0)) is reported, once.

    [0, 300, 0, 300, 0, 300, 0, 300] over 300 keys: max_large = 0 and there is no large segment, so the bounds hold (chain_ok 1, no
    chain launched).  Four identical class 1 segments go to the list (4 <= nseg = 7 rows), the class 1 grid is min(7, 300 / 257, ..) = 1:
    one workgroup sorts [0, 300) four times from the same input to the same output, so [0, 300) holds the oracle's order."""
    rng = np.random.default_rng(83)
    n, off = S.FOLD_LARGE
    g = S.seg_geometry(off, n, device_cus())
    assert (g["chain_ok"], g["nlarge"], g["tiles"], g["first_bad"]) == (0, 0, 0, 1)
    x = with_ties(np.uint32, n, rng)
    eng = rsx.Engine(np.uint32, n, payload=True)
    k, p, _ = run(rsx, x, off, False, True, eng=eng)                        # guard bands checked inside
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "segment 1 " in str(ei.value)
    eng.sync()                                                               # reported once
    assert np.array_equal(k, sentinel_keys(x)) and np.array_equal(p, sentinel_payload(n))
    good = S.offsets_from([4097, 3, 900])
    k, p, _ = run(rsx, x, good, False, True, eng=eng)
    eng.sync()
    check(x, good, k, p, False)

    n, off = S.FOLD_SMALL
    g = S.seg_geometry(off, n, device_cus())
    assert (g["chain_ok"], g["count"], g["grid"][1], g["first_bad"]) == (1, [0, 4, 0], 1, 1)
    x = with_ties(np.uint32, n, rng)
    eng = rsx.Engine(np.uint32, n, payload=True)
    k, p, _ = run(rsx, x, off, False, True, eng=eng)
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "segment 1 " in str(ei.value)
    eng.sync()
    once = np.array([0, n], dtype=np.uint64)
    assert np.array_equal(seg_oracle(x, off, n), seg_oracle(x, once, n))    # the overlapping segments are identical: one answer
    check(x, once, k, p, False)
    good = S.offsets_from([100, 0, 200])
    k, p, _ = run(rsx, x, good, False, True, eng=eng)
    eng.sync()
    check(x, good, k, p, False)
