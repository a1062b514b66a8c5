"""The segmented reduction without a GPU: the referee of tests/_segreduce_ref.py against hand-written cases, model_sum against a hand
expansion of the order written in rsx_segreduce.hpp, the layouts against the paths they are named after, the declaration in header,
library and binding, and the helpers' argument errors."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import _segreduce_ref as R
from _segreduce_ref import JOIN, TILE, UNIT, WAVE, WIDE, model_sum, offsets_from, paths, reduce_oracle, reduce_terms
from test_segmented import HEADER

f32 = np.float32


def test_symbol_in_header_exports_and_binding(rsx):
    raw = open(HEADER).read()
    for name, code in (("SUM", 0), ("MIN", 1), ("MAX", 2), ("ARGMIN", 3), ("ARGMAX", 4)):
        assert re.search(rf"#define\s+RSX_REDUCE_{name}\s+{code}\b", raw), name
        assert getattr(rsx, "REDUCE_" + name) == code == R.OPCODE[name.lower()]
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_reduce\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_reduce is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_values", "uint64_t n", "const uint64_t* d_offsets", "uint64_t num_segments", "uint32_t flags",
                      "uint32_t op", "uint32_t value_kind", "void* d_values_out", "uint32_t* d_index_out"]
    assert "rsx_segmented_reduce" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_reduce
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_reduce\b", out)
    for name in ("segmented_reduce", "reduce_rows", "amax", "amin", "argmax", "argmin", "max_rows", "min_rows"):
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_reduce)
    for name in ("sum", "min", "max"):                            # the module keeps the builtins
        assert not hasattr(rsx, name), name


def test_referee_hand_made():
    v = np.array([3, -1, 7, 7, 2, -1, 5], dtype=np.int32)
    off = [0, 0, 4, 4, 7]
    assert reduce_oracle(v, off, "sum")[0].tolist() == [0, 16, 0, 6]
    assert reduce_oracle(v, off, "min")[0].tolist() == [2 ** 31 - 1, -1, 2 ** 31 - 1, -1]
    assert reduce_oracle(v, off, "max")[0].tolist() == [-2 ** 31, 7, -2 ** 31, 5]
    res, idx = reduce_oracle(v, off, "argmax")
    assert idx.tolist() == [-1, 2, -1, 2] and res.tolist() == [-2 ** 31, 7, -2 ** 31, 5]      # the first of the two 7s
    res, idx = reduce_oracle(v, off, "argmin")
    assert idx.tolist() == [-1, 1, -1, 1] and res.tolist() == [2 ** 31 - 1, -1, 2 ** 31 - 1, -1]
    w = np.array([2 ** 31 - 1, 1, 5], dtype=np.int32)
    assert reduce_oracle(w, [0, 2, 3], "sum")[0].tolist() == [-2 ** 31, 5]                        # integer sums wrap
    f = np.array([1.0, np.nan, 9.0, np.nan, -0.0, 0.0, -0.0, np.inf], dtype=f32)
    off = [0, 4, 7, 8, 8]
    assert np.isnan(reduce_oracle(f, off, "max")[0][0]) and np.isnan(reduce_oracle(f, off, "min")[0][0])
    res, idx = reduce_oracle(f, off, "argmax")
    assert idx.tolist() == [1, 0, 0, -1] and np.isnan(res[0]) and np.signbit(res[1]) and res[3] == -np.inf    # first NaN; -0.0 ties with +0.0
    res, idx = reduce_oracle(f, off, "argmin")
    assert idx.tolist() == [1, 0, 0, -1] and res[3] == np.inf
    assert reduce_oracle(f, off, "sum")[0].dtype == np.float64 and reduce_oracle(f, off, "sum")[0][3] == 0
    assert reduce_oracle(f, None, "argmax")[1].tolist() == [1]                                    # no offsets: one segment
    m, mag = reduce_terms(f[4:], [0, 3, 4])
    assert m.tolist() == [3, 1] and mag[0] == 0 and mag[1] == np.inf


def hand_fold(x):
    """left to right in the values' own precision"""
    acc = x[0]
    for y in x[1:]:
        acc = acc + y
    return acc


def test_model_sum_one_tile_with_boundaries_at_20_and_1000():
    """three segments in one tile, [0, 20), [20, 1000), [1000, 4096), expanded by hand from the header's text"""
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(TILE) * 10.0 ** rng.integers(-3, 4, TILE)).astype(f32)
    got = model_sum(v, [0, 20, 1000, TILE])
    # [0, 20): ends at element 3 of thread 1, which has no restart at or before it: T(0) o a[3], T(0) = thread 0's fold
    want0 = hand_fold(v[0:16]) + hand_fold(v[16:20])
    # [20, 1000): begins at element 4 of thread 1, ends at element 7 of thread 62 (all in wave 0): T(61) o a[7], with T(61) cut at thread 1,
    # whose own part is the fold of its elements 4 .. 15
    def t61():
        def x(level, lane):
            own = hand_fold(v[20:32]) if lane == 1 else hand_fold(v[16 * lane:16 * lane + 16])
            if level == 0 or lane == 1:
                return own
            d = 1 << (level - 1)
            right = x(level - 1, lane)
            if lane - d < 1:
                return right
            return x(level - 1, lane - d) + right
        return x(6, 61)
    want1 = t61() + hand_fold(v[992:1000])
    # [1000, 4096): begins at element 8 of thread 62 and ends with the tile: T(255).  Wave 0's total is x(63) cut at thread 62; the waves
    # 1, 2, 3 have no restart: their totals are full Hillis-Steele scans; the totals are folded left to right and put on the LEFT of x(63
    # of wave 3).  T(255) = ((w0 o w1) o w2) o w3.
    def wave_total(wave, cut_lane=None, cut_from=0):
        def x(level, lane):
            g = wave * 64 + lane
            own = hand_fold(v[16 * g + (cut_from if lane == cut_lane else 0):16 * g + 16])
            if level == 0 or lane == cut_lane:
                return own
            d = 1 << (level - 1)
            right = x(level - 1, lane)
            if lane - d < (cut_lane if cut_lane is not None else 0):
                return right
            return x(level - 1, lane - d) + right
        return x(6, 63)
    want2 = ((wave_total(0, 62, 8) + wave_total(1)) + wave_total(2)) + wave_total(3)
    assert got.dtype == f32
    assert [x.tobytes() for x in got] == [f32(want0).tobytes(), f32(want1).tobytes(), f32(want2).tobytes()]


def test_model_sum_join_by_hand():
    """a segment over 3 and over 70 tiles, all values exact in float32, so every association gives the exact sum; and the join's order on
    values where it matters: tail o ((l0 o l1) o ...) as the tree of one wave"""
    rng = np.random.default_rng(6)
    for tiles in (3, 70, 258):
        n, off = R.layout_long(tiles)
        v = rng.integers(-8, 9, n).astype(f32)
        assert np.array_equal(model_sum(v, off), reduce_oracle(v, off, "sum")[0].astype(f32))
    # 4 tiles: [5, 4 * 4096): tail = tile 0 from 5, leads = tiles 1, 2 and 3: J = (l1 o l2) o l3 (distance 1, then 2), result tail o J
    n = 4 * TILE
    v = np.zeros(n, dtype=f32)
    v[5], v[TILE], v[2 * TILE], v[3 * TILE] = 1.0, 2.0 ** 24, 1.0, -2.0 ** 24
    got = model_sum(v, [5, n])[0]
    assert got == f32(f32(1.0) + f32(f32(f32(2.0 ** 24) + f32(1.0)) + f32(-2.0 ** 24))) == 1.0      # the lead of tile 2 is lost in J
    assert reduce_oracle(v, [5, n], "sum")[0][0] == 2.0


@pytest.mark.parametrize("vt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_model_sum_within_the_any_order_bound(vt):
    rng = np.random.default_rng(7)
    n, off = R.layout_ragged()
    v = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(vt)
    ref = reduce_oracle(v, off, "sum")[0]
    wide = ref.dtype.type
    m, mag = reduce_terms(v, off)
    k = np.maximum(m - 1, 0).astype(wide)
    u = wide(UNIT[np.dtype(vt)])
    bound = k * u / (1 - k * u) * mag + m.astype(wide) * wide(np.finfo(wide).eps) * mag
    assert np.all(np.abs(model_sum(v, off).astype(wide) - ref) <= bound)
    assert WIDE[np.dtype(vt)] is wide


LAYOUT_PATHS = {
    "ragged": (R.layout_ragged, {"off[0] > 0", "off[S] < n", "empty", "inside a thread", "inside a wave", "inside a tile", "join: one wave"}),
    "inside": (R.layout_inside, {"inside a thread", "inside a wave", "inside a tile", "empty"}),
    "ends on edge": (R.layout_ends_on_edge, {"ends on a tile edge", "join: one wave", "off[S] < n"}),
    "first and last": (R.layout_first_last, {"boundary at a tile's first element", "boundary at a tile's last element"}),
    "64 leads": (lambda: R.layout_long(64, start=TILE - 1), {"join: one wave", "boundary at a tile's last element"}),
    "65 leads": (lambda: R.layout_long(65, start=TILE - 1), {"join: four waves"}),
    "70 tiles": (lambda: R.layout_long(70), {"join: four waves"}),
    "258 tiles": (lambda: R.layout_long(258), {"join: more than one partial per thread"}),
    "two tiles, one segment": (lambda: R.layout_two_tiles(False), {"two tiles per workgroup", "join: more than one partial per thread"}),
    "two tiles, rows": (lambda: R.layout_two_tiles(True), {"two tiles per workgroup", "ends on a tile edge", "boundary at a tile's first element"}),
    "5000 empty": (R.layout_many_empty, {"empty", "inside a tile"}),
    "empty at the end": (R.layout_empty_at_end, {"empty where no tile is", "ends on a tile edge"}),
    "all empty": (R.layout_all_empty, {"empty", "off[0] > 0", "off[S] < n"}),
}


@pytest.mark.parametrize("name", list(LAYOUT_PATHS))
def test_layouts_reach_their_paths(name):
    make, want = LAYOUT_PATHS[name]
    n, off = make()
    o = off.astype(np.int64)
    assert np.all(o[1:] >= o[:-1]) and o[-1] <= n
    got = paths(n, off)
    assert want <= got, f"{name}: missing {want - got}"
    if name == "inside":
        assert not any(p.startswith("join") for p in got)
    if name == "64 leads":
        assert "join: four waves" not in got                      # the last size that the first wave joins alone
    if name == "all empty":
        assert got == want
    if name == "5000 empty":
        assert np.count_nonzero(o[1:] == o[:-1]) == 5000
    assert JOIN == 256 and WAVE == 64


# -- the layouts of tests/test_gpu_segreduce_paths.py --------------------------------------------------------------------------------------

def test_old_layouts_never_put_three_starts_into_a_thread():
    """what the layouts above leave out: at most 2 starts in a thread, off[S] never on a thread edge inside a tile nor at a tile's last
    element (at its second element only as off[S] = n = 2^24 + 4097, in the two-tile layouts)"""
    new = {"three or more starts in a thread", "16 starts in a thread", "4096 starts in a tile", "empty between one-element segments",
           "stop on a thread edge inside a tile", "stop at a tile's last element"}
    for name, (make, _) in LAYOUT_PATHS.items():
        assert not (paths(*make()) & new), name


def test_dense_layouts_reach_their_paths():
    want = {"every element": {"16 starts in a thread", "three or more starts in a thread", "4096 starts in a tile"},
            "ones and empties": {"three or more starts in a thread", "empty between one-element segments", "empty"},
            "thread edges": {"boundary on a thread edge", "boundary one element behind a thread edge", "inside a thread"}}
    for name, make in R.DENSE.items():
        n, off = make()
        o = off.astype(np.int64)
        assert o[0] == 3 and o[-1] == 3 + 2 * TILE + 37 and n == o[-1] + 5 and np.all(o[1:] >= o[:-1])
        got = paths(n, off)
        assert want[name] <= got, f"{name}: missing {want[name] - got}"
        assert {"off[0] > 0", "off[S] < n"} <= got
    o = R.layout_ones_and_empties()[1].astype(np.int64)
    assert np.diff(o)[:7].tolist() == [1, 0, 2, 0, 0, 1, 3] and np.bincount(o[:-1][np.diff(o) > 0] // R.KPT).max() >= 4
    o = R.layout_thread_edges()[1].astype(np.int64)
    assert o[:5].tolist() == [3, 16, 32, 33, 48] and "16 starts in a thread" not in paths(*R.layout_thread_edges())


def test_position_layouts_reach_their_stops():
    layouts = R.position_layouts()
    P = R.POSITIONS
    assert len(layouts) == len(P) * (len(P) - 1) // 2 + 10 + 2 and all(n == 3 * TILE for n, _ in layouts)
    got = set()
    for n, off in layouts:
        o = off.astype(np.int64)
        assert np.all(o[1:] > o[:-1]) and o[-1] <= n
        got |= paths(n, off)
    assert {"stop on a thread edge inside a tile", "stop at a tile's second element", "stop at a tile's last element", "ends on a tile edge",
            "boundary at a tile's first element", "boundary at a tile's last element", "inside a thread", "join: one wave"} <= got
    two = [off.astype(np.int64)[1] for _, off in layouts if len(off) == 3]
    assert two == [15, 16, 17, 1023, 1024, 4095, 4096, 4097, 8191, 8192]
    # off[S] on a thread edge inside a tile with off[0] in an earlier thread of that tile or in an earlier tile: the stop is the first flag of
    # thread hi / 16 (j0 == 0, tid > 0) and closes a segment by ids.last or by lead[]
    ends = [(int(off[0]), int(off[-1])) for _, off in layouts if len(off) == 2]
    assert (17, 1024) in ends and (15, 16) in ends                  # ... by ids.last: the segment began in this tile
    assert (5, TILE + 1024) in ends and (5, 2 * TILE + 16) in ends  # ... by lead[]: it began one and two tiles earlier


def test_two_joins_layout_schedules_both_orders():
    """from the offsets alone (no 18M values): the join's workgroups 5, 105 and 125 take a second open tile"""
    n, off = R.layout_two_joins()
    assert (n + TILE - 1) // TILE == 4401 and R.chunk_of(n) == 2 and R.join_grid(n, len(off) - 1) == 4096
    sched = R.join_schedule(n, off)
    # (the segment that begins in tile 4221 ends at n - 4 in tile 4400: 179 tiles behind it)
    assert sched == {0: [(0, 5)], 5: [(5, 30), (4101, 100)], 35: [(35, 70)], 105: [(105, 195), (4201, 20)], 300: [(300, 3801)], 125: [(4221, 179)]}
    kind = lambda m: "one wave" if m <= WAVE else "four waves"
    orders = {tuple(kind(m) for _, m in tiles) for tiles in sched.values() if len(tiles) == 2}
    assert orders == {("one wave", "four waves"), ("four waves", "one wave")}
    assert max(m for tiles in sched.values() for _, m in tiles) > 2 * JOIN and -(-3801 // JOIN) == 15        # more than 2 partials a thread
    assert sched[125][0][0] >= 4096                                 # a second trip without a first join
    # the tile kernel: a boundary inside the first tile of a workgroup and inside the second tile of one
    o = off.astype(np.int64)
    inner = o[1:-1] // TILE
    assert np.any(inner % 2 == 0) and np.any(inner % 2 == 1)
    got = paths(n, off)
    assert {"two tiles per workgroup", "join: one wave", "join: four waves", "join: more than one partial per thread"} <= got
    # 4097 tiles is the least at which a workgroup of the join gets a second tile
    assert R.join_grid(4096 * TILE, 1) == 4096 and (4097 * TILE + TILE - 1) // TILE > 16 * R.CUS


def test_million_segments_layout_needs_a_second_trip():
    n, off = R.layout_million_segments()
    S = len(off) - 1
    assert S == (1 << 20) + 4099 and S > 256 * 16 * 256 and R.join_grid(n, S) * JOIN < S
    o = off.astype(np.int64)
    assert o[0] == 5 and n == o[-1] + 5 and np.diff(o)[:6].tolist() == [1, 0, 2, 0, 0, 1] and 650000 < n < 750000
    assert R.dense_paths(o) >= {"empty between one-element segments", "three or more starts in a thread"}
    assert np.count_nonzero(np.diff(o)[1 << 20:] == 0) > 2000      # empty segments among those of the second trip


def special_values(vt, n, rng):
    """values whose sums are exact in the wide format in any order (whole multiples of 2^-10 below 2^10), with NaN, +-inf and +-0.0 for floats"""
    vt = np.dtype(vt)
    if vt.kind == "i":
        info = np.iinfo(vt)
        return rng.integers(info.min, info.max, n, dtype=vt, endpoint=True)
    v = (rng.integers(-(1 << 20), 1 << 20, n) / 1024.0).astype(vt)
    pick = rng.integers(0, 40, n)
    for code, special in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0)):
        v[pick == code] = special
    return v


@pytest.mark.parametrize("vt", [np.int32, np.int64, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("op", R.OPS)
def test_fast_referee_equals_loop_referee(vt, op):
    rng = np.random.default_rng(R.OPS.index(op) * 4 + np.dtype(vt).itemsize)
    layouts = [R.layout_ragged, R.layout_many_empty, R.layout_all_empty, lambda: (100, None)] + list(R.DENSE.values())
    arg = op in ("argmin", "argmax")
    for make in layouts:
        n, off = make()
        for ties in (False, True):
            v = rng.integers(-2, 3, n).astype(vt) if ties else special_values(vt, n, rng)
            if ties and np.dtype(vt).kind == "f":
                v[rng.integers(0, 9, n) == 0] = -0.0
            want, widx = reduce_oracle(v, off, op)
            got, gidx = R.reduce_fast(v, off, op)
            assert got.dtype == want.dtype and got.shape == want.shape
            if arg:
                assert np.array_equal(gidx, widx) and got.tobytes() == want.tobytes()          # the element itself: its bits
            else:
                assert gidx is None and widx is None
                assert np.array_equal(got, want, equal_nan=np.dtype(vt).kind == "f")          # (the sign of a zero result is numpy's choice)
            if np.dtype(vt).kind == "f":
                (m, mag), (fm, fmag) = reduce_terms(v, off), R.terms_fast(v, off)
                assert np.array_equal(m, fm) and np.array_equal(mag, fmag, equal_nan=True)
                inside = v if off is None else v[int(off[0]):int(off[-1])]
                if np.dtype(vt).kind == "f" and not ties and inside.size > 1000:
                    assert np.isnan(inside).any() and np.isinf(inside).any() and np.any((inside == 0) & np.signbit(inside)) and np.any((inside == 0) & ~np.signbit(inside))


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    assert lib.rsx_segmented_reduce(None, None, 16, None, 1, 0, 0, 0, None, None) == 4            # a null engine is refused
    assert b"rsx_segmented_reduce" in lib.rsx_last_error()
    torch = pytest.importorskip("torch")
    vals = torch.ones(10, dtype=torch.float32)
    offsets = torch.tensor([0, 10], dtype=torch.int64)
    with pytest.raises(ValueError):              # host tensors: no CPU fallback
        rsx.segmented_reduce(vals, offsets)
    for fn in (rsx.reduce_rows, rsx.amax, rsx.amin, rsx.argmax, rsx.argmin, rsx.max_rows, rsx.min_rows):
        with pytest.raises(ValueError):
            fn(vals.reshape(2, 5))
    with pytest.raises(ValueError):              # an unknown op
        rsx.segmented_reduce(vals, offsets, op="prod")
    with pytest.raises(ValueError):
        rsx.reduce_rows(vals, op="prod")
    for dt in (torch.float16, torch.bfloat16, torch.bool):
        with pytest.raises(TypeError):           # value types outside the four
            rsx.segmented_reduce(vals.to(dt), offsets)
        with pytest.raises(TypeError):
            rsx.reduce_rows(vals.to(dt))
        with pytest.raises(TypeError):
            rsx.argmax(vals.to(dt))
    with pytest.raises(TypeError):               # the mean of integers
        rsx.segmented_reduce(vals.to(torch.int32), offsets, op="mean")
