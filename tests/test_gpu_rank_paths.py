"""rsx_segmented_rank on the launch paths of rsx_rank.hpp and capi_rank.inc that tests/test_gpu_rank.py never reaches (its largest call has
14 segments, one trip of every grid and join records in the first eight threads of one wave; tests/test_rank.py pins that):

  A  the item loop of rank_small_kernel: more segments of a class than workgroups, the second item the shorter one, so that it is ranked
     over the image, the positions and the rank slots of a longer segment; with ties (one barrier sequence at the loop's end) and without;
  B  real keys equal to the pad key (the encoded all-ones key) as the last tie group of small segments shorter than their class's tile,
     where the pads sort directly behind them and the group's end must come out as the segment's length;
  C  the stride loop of rank_ones_kernel (600 000 segments), the classify scan with two blocks per thread under the rank's classify,
     37 trips of the class-0 grid; and bad offsets deep in that list, reported under the rank's name;
  D  rank_join_kernel beyond one wave and beyond 256 tiles: the cross-wave fold, two tiles per thread, idle threads, pieces, lane scans
     and wave totals without a head, runs that begin and end exactly on tile edges;
  E  the grid strides of rank_edge_kernel, rank_write_kernel and rank_join_kernel: more tiles and more large segments than workgroups,
     as many large segments as the keys can hold;
  F  the flat form in every regime of the sort chain, on one engine and one key buffer: where the chain leaves its result differs;
  G  one engine, one wait: ranks between a unique, a histogram, a scan and a compact, which share the positions, the segmented table and
     the status word with it; a rank with bad offsets among good calls of other kinds;
  H  one captured rank replayed over other offsets: another class mix, no large segment, only large and empty segments.

The layouts and path predicates are held in tests/_rank_ref.py (tests/test_rank.py checks them on the CPU, at three CU counts where the
path depends on the count); every test here rebuilds its layout for the device's own CU count, prints the figures and asserts the path
before it compares.  Every comparison is exact integer equality with the referee, entry for entry, through run / check of
tests/test_gpu_rank.py: the sentinel where nothing is written, guard bands around both outputs.  Every engine a test creates is closed by
the test (the flat form's by its fixture).
"""
import numpy as np
import pytest

import _rank_ref as R
import _segmented_ref as S
from _histogram_ref import histogram_oracle
from test_gpu_compact import random_mask
from test_gpu_family_engine import CAP, Call, compact_call, scan_call, u32
from test_gpu_rank import FRONT, _band, _unband, check, engine, mixed_case, random_keys, run, run_check_all
from test_gpu_scan import ragged as scan_ragged
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL32, LENGTHS
from test_gpu_unique import check as unique_check
from test_gpu_unique_reduce_paths import Outputs
from test_gpu_wselect_paths import device_cus

pytestmark = pytest.mark.gpu


def run_checked(rsx, eng, x, off, want, calls, what):
    """calls: (method, with the tie counts or without) in order"""
    for method, want_ties in calls:
        check(run(rsx, eng, x, off, method, want_ties=want_ties), want, method, f"{what}{'' if want_ties else ' (no ties)'}")


# -- A. the small kernel's second trip --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls,dt,descending", [(0, np.uint32, False), (1, np.uint64, True), (2, np.int32, False)],
                         ids=["class0-uint32", "class1-uint64-desc", "class2-int32"])
def test_more_segments_of_a_class_than_workgroups(rsx, cls, dt, descending):
    """S.stride_layout at the device's CU count: 400 (classes 0, 1) / 200 (class 2) workgroups of rank_small_kernel rank a second segment,
    a shorter one, after their first: its pads lie over the first one's keys and positions, its rank slots over the first one's ranks.
    AVERAGE with the tie counts, DENSE without: the two ends of the item loop."""
    cus = device_cus()
    n, off = S.stride_layout(cls, cus)
    g = R.rank_geometry(off, n, cus)
    print(f"cus {cus} n {n} {R.rank_summary(g)}")
    assert g["small_trips"][cls] >= 2 and g["count"][cls] > g["grid"][cls] == cus * S.PER_CU[cls]
    lens = np.diff(off.astype(np.int64))
    order, grid = g["lists"][cls], g["grid"][cls]
    second = np.arange(grid, g["count"][cls])
    assert np.all(lens[order[second]] < lens[order[second - grid]])
    rng = np.random.default_rng(500 + cls)
    x = random_keys(rng, dt, n)                                                  # an alphabet of 8 values: long tie groups
    want = R.rank_oracle_many(x, off, descending, fill=FILL32)
    eng = engine(rsx, dt, n, descending)
    run_checked(rsx, eng, x, off, want, [(R.AVERAGE, True), (R.DENSE, False)], f"class {cls}, second trip")
    eng.sync()
    eng.close()


# -- B. real keys equal to the pad key ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,descending", R.PAD_PAIRS, ids=[f"{dt}-{'desc' if d else 'asc'}" for dt, d in R.PAD_PAIRS])
def test_pad_equal_keys_as_the_last_tie_group(rsx, dt, descending):
    """R.pad_equal_layout / pad_equal_keys: in every class segments of TILE_c - 1, TILE_c - 17 and 2 TILE_c / 3 keys whose last third, and
    five keys more, ARE the pad key of rank_small_kernel (uint32 max ascending, 0 descending, +NaN 0x7FFFFFFF ascending, -NaN 0xFFFFFFFF
    descending): the pads sort directly behind them, no head separates the two, and the group's end must be the segment's length."""
    n, off, planted = R.pad_equal_layout()
    rng = np.random.default_rng(520 + R.PAD_PAIRS.index((dt, descending)))
    x, counts = R.pad_equal_keys(dt, descending, n, off, planted, rng)
    g = R.rank_geometry(off, n, device_cus())
    print(f"n {n} pad {int(R.pad_value(dt, descending).view(np.uint32)):#x} planted {counts} {R.rank_summary(g)}")
    assert g["count"] == [3, 3, 3] and g["nlarge"] == 1 and len(planted) == 10
    eng = engine(rsx, dt, 1 << 15, descending)
    ranks, ties, _ = run_check_all(rsx, eng, x, off, descending, what=f"pad-equal {dt} descending={descending}")
    pad = R.pad_value(dt, descending).view(np.uint32)
    for s in planted:                                                            # from the referee: the planted group is the last run, of the planted size
        a, b = int(off[s]), int(off[s + 1])
        at = np.flatnonzero(x[a:b].view(np.uint32) == pad)
        assert len(at) == counts[s] and np.all(ties[a:b][at] == counts[s]) and np.all(ranks[R.MAX][a:b][at] == b - a - 1)
        assert np.all(ranks[R.MIN][a:b][at] == b - a - counts[s]) and int(ranks[R.DENSE][a:b].max()) == int(ranks[R.DENSE][a + at[0]])
    eng.sync()
    eng.close()


# -- C. many segments -----------------------------------------------------------------------------------------------------------------------------

def test_many_segments_and_bad_offsets_deep_in_the_list(rsx):
    """S.sparse_large: 600 000 segments of 0 .. 3 keys with 43 large ones in 41 classify blocks.  rank_ones_kernel's stride loop makes
    three trips at 256 CUs, the classify scan takes two blocks per thread under the rank's classify, the class-0 grid makes 37 trips.
    Then S.sparse_large_bad on the same engine: segment 550001 is reported once, under the rank's name, nothing is written, and the
    next good call is right."""
    cus = device_cus()
    n, off = S.sparse_large()
    g = R.rank_geometry(off, n, cus)
    print(f"cus {cus} n {n} ones {g['ones']} {R.rank_summary(g)}")
    assert g["ones_trips"] >= 2 and g["per"] == 2 and g["small_trips"][0] >= 2 and g["nlarge"] >= 30 and g["large_blocks"] >= 30
    rng = np.random.default_rng(530)
    x = random_keys(rng, np.uint32, n)
    want = R.rank_oracle_many(x, off, fill=FILL32)
    eng = engine(rsx, np.uint32, n)
    run_checked(rsx, eng, x, off, want, [(R.ORDINAL, True), (R.MAX, False)], "sparse large")
    eng.sync()
    nb, bad = S.sparse_large_bad()
    assert nb == n and R.rank_geometry(bad, n, cus)["first_bad"] == 550001
    ranks, ties = run(rsx, eng, x, bad, R.AVERAGE)
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "rsx_segmented_rank" in str(ei.value) and "segment 550001 " in str(ei.value), str(ei.value)
    eng.sync()                                                                   # reported once
    assert np.all(ranks == FILL32) and np.all(ties == FILL32)
    run_checked(rsx, eng, x, off, want, [(R.MIN, True)], "after bad offsets")
    eng.sync()
    eng.close()


# -- D. the join beyond one wave and beyond 256 tiles ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,descending,methods", [(np.uint32, False, tuple(range(5))), (np.float64, True, (R.AVERAGE, R.DENSE))],
                         ids=["uint32-all-methods", "float64-desc"])
def test_join_beyond_one_wave_and_beyond_256_tiles(rsx, dt, descending, methods):
    """R.join_layout: large segments of 65, 256 and 385 tiles in one call, each from the middle of a tile, small ones between them, the
    keys built from run lists and shuffled.  65 tiles: the cross-wave fold of the join's scan carries a head into the second wave.  256
    tiles: every thread one record, two whole waves of threads without a head.  385 tiles (257 cannot hold a run of 2 * 128 tiles'
    worth beside the rest): two tiles per thread, the last thread with one, 63 idle threads, threads whose whole piece is headless, two
    whole waves headless, a run that begins on a tile's first key and ends on a tile's last, ten tiles in which every key is a head."""
    cus = device_cus()
    n, off, names, runs = R.join_layout()
    g = R.rank_geometry(off, n, cus)
    rng = np.random.default_rng(540 + descending)
    x = R.join_keys(dt, descending, n, off, names, runs, rng)
    facts = [R.join_facts(a, s) for a, s in R.sorted_keys_layout(x, off, descending)]
    paths = R.join_paths(facts)
    print(f"cus {cus} n {n} {R.rank_summary(g)}")
    for f in facts:
        print({k: v for k, v in f.items() if k not in ("edges", "thread_headless")}, "headless threads", sum(f["thread_headless"]))
    assert g["T"] == list(R.JOIN_TILES) and g["join_per"] == [1, 1, 2] and all(int(off[s]) % R.TILE for s in names.values())
    assert all(paths.values()), [name for name, reached in paths.items() if not reached]
    eng = engine(rsx, dt, n, descending)
    run_check_all(rsx, eng, x, off, descending, what=f"join {np.dtype(dt).name}", methods=methods)
    eng.sync()
    eng.close()


# -- E. grid strides of the tile kernels and the join ------------------------------------------------------------------------------------------------

def test_more_tiles_and_large_segments_than_workgroups(rsx):
    """R.grid_stride_layout: cus * 8 + 40 large segments of 4097 .. 4300 keys on grids of cus * 8: rank_join_kernel's last 40 segments and
    the last third of the tiles of rank_edge_kernel / rank_write_kernel belong to a second and third trip, over the scan words of the
    first; rank_tile searches 2088 tile starts (at 256 CUs), and there are as many large segments as n keys can hold (or up to three
    fewer: the last rows of the large-segment table)."""
    cus = device_cus()
    n, off = R.grid_stride_layout(cus)
    g = R.rank_geometry(off, n, cus)
    print(f"cus {cus} n {n} {R.rank_summary(g)}")
    assert g["join_trips"] >= 2 and g["tile_trips"] >= 2 and 0 <= g["max_large"] - g["nlarge"] <= 3 and int(off[0]) == 5
    rng = np.random.default_rng(550)
    x = rng.integers(-20, 20, n).astype(np.int32)
    want = R.rank_oracle(x, off, fill=FILL32)
    eng = engine(rsx, np.int32, n)
    # one call (two took longer than the slowest test of test_gpu_segmented_paths.py): DENSE reads the join's dense carry, the tie
    # counts are end - start, its other two
    run_checked(rsx, eng, x, off, want, [(R.DENSE, True)], "grid strides")
    eng.sync()
    eng.close()


# -- F. the flat form in every sort regime -----------------------------------------------------------------------------------------------------------

# (n, digit width, the two calls): the regimes in the order of R.FLAT_SIZES, back to a small n, then the 8-bit chain
FLAT_STEPS = [(n, 4, pair) for n, pair in zip(R.FLAT_SIZES, [((R.AVERAGE, True), (R.DENSE, False)), ((R.ORDINAL, True), (R.MAX, False)),
                                                             ((R.MIN, True), (R.AVERAGE, False)), ((R.DENSE, True), (R.ORDINAL, False)),
                                                             ((R.MAX, True), (R.MIN, False))])]
FLAT_STEPS += [(5000, 4, ((R.AVERAGE, True), (R.DENSE, False)))]
FLAT_STEPS += [(n, 8, pair) for n, pair in zip(R.FLAT_SIZES_8BIT, [((R.AVERAGE, True), (R.ORDINAL, False)), ((R.DENSE, True), (R.MAX, False))])]


@pytest.fixture(scope="module")
def flat_engine(rsx):
    """one payload engine of capacity 2^23 and one device key buffer for every flat step, in order"""
    t = _torch()
    eng = engine(rsx, np.int32, R.FLAT_CAPACITY)
    keys = t.empty(R.FLAT_CAPACITY, dtype=t.int32, device="cuda")
    yield eng, keys
    eng.close()


@pytest.mark.parametrize("n,bits,calls", FLAT_STEPS, ids=[f"{n}-{bits}bit" for n, bits, _ in FLAT_STEPS])
def test_flat_form_in_every_sort_regime(rsx, flat_engine, n, bits, calls):
    """d_offsets == NULL goes through the engine's own sort chain, which picks its regime by n (R.flat_regime, from the engine's defaults:
    there is no getter for them) and leaves the sorted keys and positions in another pair of buffers each time; the rank reads them
    from wherever that is.  2^19: the last small-tile self-scan size; 2^19 + 1: the first size on 4096-key tiles; 257 tiles - 100: the
    flat join with two tiles per thread; 2^22: the self-scan's last size; 2^22 + 4097: the look-ahead chain, five tiles per join thread;
    5000 again on what the large calls left; then 8-bit digits.  The keys are rewritten in place in one device buffer."""
    t = _torch()
    eng, keys = flat_engine
    eng.set_option(rsx.OPT_RADIX_BITS, bits)
    g = R.rank_geometry(None, n, device_cus())
    print(f"n {n} digits {bits} regime {R.flat_regime(n, bits)} {R.rank_summary(g)}")
    assert g["nlarge"] == 1 and g["T"] == [(n + R.TILE - 1) // R.TILE] and n <= R.FLAT_CAPACITY
    rng = np.random.default_rng(n + bits)
    x = random_keys(rng, np.int32, n, values=2000)                               # half the keys one value, the rest in runs of some hundred
    want = R.rank_oracle(x, None, fill=FILL32)
    keys[:n].copy_(t.from_numpy(x))                                              # rewritten in place
    t.cuda.synchronize()
    for method, want_ties in calls:
        r_buf, t_buf = _band(t, n * 4), _band(t, n * 4)
        eng.segmented_rank(keys.data_ptr(), n, None, 1, method, r_buf.data_ptr() + FRONT, t_buf.data_ptr() + FRONT if want_ties else None)
        t.cuda.synchronize()
        ranks, ties = _unband(r_buf, n * 4, "ranks"), _unband(t_buf, n * 4, "ties")
        assert want_ties or np.all(ties == FILL32)
        check((ranks, ties if want_ties else None), want, method, f"flat {n}, {bits}-bit digits")
    eng.sync()
    eng.set_option(rsx.OPT_RADIX_BITS, 4)


# -- G. one engine, one wait -----------------------------------------------------------------------------------------------------------------------

def rank_call(t, x, off, method, what):
    n, nseg = x.size, 1 if off is None else len(off) - 1
    ins = dict(keys=x) if off is None else dict(keys=x, off=off)

    def launch(eng, i, o):
        eng.segmented_rank(i["keys"], n, i.get("off"), nseg, method, o("ranks"), o("ties"))

    def verify(got):
        check((got["ranks"], got["ties"]), R.rank_oracle(x, off, fill=FILL32), method, what)

    return Call(t, what, ins, dict(ranks=4 * n, ties=4 * n), dict(ranks=np.uint32, ties=np.uint32), launch, verify)


def unique_positions_call(t, x, off, what):
    """a segmented unique with first positions and the inverse map: it carries the positions 0, 1, 2, ... that the rank carries too"""
    n, nseg = x.size, len(off) - 1

    def launch(eng, i, o):
        eng.segmented_unique(i["keys"], n, i["off"], nseg, o("keys"), o("run_offsets"), o("counts"), o("first"), o("inverse"))

    return Call(t, what, dict(keys=x, off=off), dict(keys=4 * n, run_offsets=8 * (nseg + 1), counts=4 * n, first=4 * n, inverse=4 * n),
                dict(keys=np.uint32, run_offsets=np.uint64, counts=np.uint32, first=np.uint32, inverse=np.uint32), launch,
                lambda got: unique_check(x, off, got))


def histogram_call(t, x, off, B, what):
    n, nseg = x.size, len(off) - 1

    def launch(eng, i, o):
        eng.segmented_histogram(i["keys"], n, i["off"], nseg, B, o("counts"))

    def verify(got):
        assert np.array_equal(got["counts"].reshape(nseg, B).astype(np.int64), histogram_oracle(x, off, B)), f"{what}: counts differ"

    return Call(t, what, dict(keys=x, off=off), dict(counts=4 * nseg * B), dict(counts=np.uint32), launch, verify)


def test_ranks_between_the_other_users_of_the_engine(rsx):
    """Seven calls enqueued back to back on one engine, one eng.sync() at the end: a unique with positions (it fills the positions the
    rank then shares), a rank, a histogram (the segmented table with its own stride), a flat rank, a scan, a rank with other offsets and
    a compact.  Each output equals its referee, and bit for bit the same call on a fresh engine."""
    t = _torch()
    rng = np.random.default_rng(560)
    off_u = S.offsets_from(LENGTHS, start=3)
    n_u = int(off_u[-1]) + 5
    n_m, off_m, x_m = mixed_case(rng, np.uint32)
    off_h = S.offsets_from([5, 30000, 0, 4096, 50000, 17, 15000], start=3)
    n_h = int(off_h[-1]) + 9
    n_flat = 70001
    n_scan, off_scan, keys_scan = scan_ragged(rng, np.uint32)
    off_o = S.offsets_from([5000, 4097, 0, 1, 300, 20000, 2, 9000], start=9)
    n_o = int(off_o[-1]) + 2
    off_c = S.offsets_from(LENGTHS * 2, start=3)
    n_c = int(off_c[-1]) + 5
    calls = [unique_positions_call(t, u32(rng, n_u, 300), off_u, "1 unique with positions"),
             rank_call(t, x_m, off_m, R.AVERAGE, "2 rank, mixed"),
             histogram_call(t, u32(rng, n_h, 70), off_h, 64, "3 histogram"),
             rank_call(t, random_keys(rng, np.uint32, n_flat, values=50), None, R.ORDINAL, "4 rank, flat"),
             scan_call(t, keys_scan, rng.integers(-1 << 30, 1 << 30, n_scan).astype(np.int32), off_scan, "5 scan by key"),
             rank_call(t, random_keys(rng, np.uint32, n_o), off_o, R.DENSE, "6 rank, other offsets"),
             compact_call(t, u32(rng, n_c, 50), off_c, "7 compact, mask", mask=random_mask(n_c, rng))]
    assert all(c.ins["keys"].numel() <= CAP for c in calls)
    outs = [c.outputs() for c in calls]
    eng = rsx.Engine(np.uint32, CAP, payload=True)
    t.cuda.synchronize()                                                         # uploads and fills have landed; from here on nothing waits
    for c, o in zip(calls, outs):
        c.enqueue(eng, o)
    eng.sync()
    got = [o.read() for o in outs]
    eng.close()
    for c, g in zip(calls, got):
        c.verify(g)
    for c, g in zip(calls, got):                                                 # the same call on an engine of its own
        alone = c.outputs()
        with rsx.Engine(np.uint32, CAP, payload=True) as fresh:
            c.enqueue(fresh, alone)
            fresh.sync()
        for name, a in alone.read().items():
            assert np.array_equal(a, g[name]), f"{c.what}: {name} differs from the same call on a fresh engine"


def test_bad_rank_among_good_calls_of_other_kinds(rsx):
    """(i) a good scan, a rank whose segment 2 ends before it begins, a good histogram and a good rank, one wait: one report, the bad
    rank's, under its name; it wrote nothing and the good calls are right.  (ii) a bad rank and a bad compact before one wait: one
    report, the first call's.  Then a good rank."""
    t = _torch()
    rng = np.random.default_rng(570)
    n = 40000
    x = random_keys(rng, np.uint32, n)
    good_off = np.array([0, 100, 5000, 5001, 30000, n], dtype=np.uint64)
    bad_at_2 = np.array([0, 100, 5000, 4000, 30000, n], dtype=np.uint64)
    bad_at_3 = np.array([0, 100, 5000, 5001, n + 1, n], dtype=np.uint64)
    n_scan, off_scan, keys_scan = scan_ragged(rng, np.uint32)
    bad_rank = rank_call(t, x, bad_at_2, R.AVERAGE, "rank, bad at segment 2")
    scan = scan_call(t, keys_scan, rng.integers(-1 << 30, 1 << 30, n_scan).astype(np.int32), off_scan, "scan before a bad rank")
    hist = histogram_call(t, u32(rng, n, 70), good_off, 64, "histogram behind a bad rank")
    good_rank = rank_call(t, x, good_off, R.MAX, "rank behind a bad rank")
    bad_compact = compact_call(t, x, bad_at_3, "compact, bad at segment 3", mask=random_mask(n, rng))

    def named(eng):
        with pytest.raises(rsx.RadixSortError) as ei:
            eng.sync()
        return ei.value.status, str(ei.value)

    with rsx.Engine(np.uint32, CAP, payload=True) as eng:
        group = [scan, bad_rank, hist, good_rank]
        outs = [c.outputs() for c in group]
        t.cuda.synchronize()
        for c, o in zip(group, outs):
            c.enqueue(eng, o)
        status, text = named(eng)
        assert status == 4 and "rsx_segmented_rank" in text and "segment 2 " in text, text
        eng.sync()                                                               # reported once
        got = [o.read() for o in outs]
        assert np.all(got[1]["ranks"] == FILL32) and np.all(got[1]["ties"] == FILL32)
        for i in (0, 2, 3):
            group[i].verify(got[i])
        group = [bad_rank, bad_compact]
        outs = [c.outputs() for c in group]
        t.cuda.synchronize()
        for c, o in zip(group, outs):
            c.enqueue(eng, o)
        status, text = named(eng)
        assert status == 4 and "rsx_segmented_rank" in text and "segment 2 " in text, text              # the first report stays
        eng.sync()
        got = [o.read() for o in outs]
        assert np.all(got[0]["ranks"] == FILL32) and np.all(got[0]["ties"] == FILL32)
        assert np.all(got[1]["koff"] == 0) and np.all(got[1]["keys"] == FILL32) and np.all(got[1]["index"] == FILL32)
        out = good_rank.outputs()
        t.cuda.synchronize()
        good_rank.enqueue(eng, out)
        eng.sync()
        good_rank.verify(out.read())


# -- H. replay over other offsets --------------------------------------------------------------------------------------------------------------------

def test_captured_rank_replayed_over_other_offsets(rsx):
    """One rsx_segmented_rank captured on a side stream (a linear capture: no parallel branches) after an eager call with the mixed
    layout, then replayed after the keys AND the offsets were rewritten in place, with the same n and segment count: another class
    mix, no large segment at all, every segment large or empty.  The grids were fixed at capture; the header on the device decides
    what each of them does."""
    t = _torch()
    rng = np.random.default_rng(580)
    n, off, x = mixed_case(rng, np.uint32)
    nseg = len(off) - 1
    kd, od = dev(t, x), dev(t, off)
    out = Outputs(t, dict(ranks=4 * n, ties=4 * n), dict(ranks=np.uint32, ties=np.uint32))
    side = t.cuda.Stream()
    eng = engine(rsx, np.uint32, 1 << 16)
    eng.set_stream(side.cuda_stream)
    method = R.AVERAGE
    call = lambda: eng.segmented_rank(kd.data_ptr(), n, od.data_ptr(), nseg, method, out.ptr("ranks"), out.ptr("ties"))
    result = lambda: (lambda got: (got["ranks"], got["ties"]))(out.read())
    call()                                                                       # eager: the first call of an engine allocates its scratch
    eng.sync()
    check(result(), R.rank_oracle(x, off, fill=FILL32), method, "eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for name, lengths in R.REPLAY_LENGTHS.items():
        off2 = S.offsets_from(lengths, start=R.REPLAY_STARTS[name])
        g = R.rank_geometry(off2, n, device_cus())
        print(f"{name}: {R.rank_summary(g)}")
        assert len(off2) == len(off) and int(off2[-1]) <= n and g["chain_ok"] == 1
        x2 = random_keys(rng, np.uint32, n)
        kd.copy_(dev(t, x2))                                                     # rewritten in place
        od.copy_(dev(t, off2))
        out.refill()                                                             # the sentinel anew (and a device-wide wait)
        graph.replay()
        t.cuda.synchronize()
        check(result(), R.rank_oracle(x2, off2, fill=FILL32), method, f"replay, {name}")
    del graph
    eng.sync()
    eng.close()
