"""CPU checks of the scan by key: header, exports, binding and the Python callables agree on rsx_segmented_scan; the two forms of the host
referee agree with each other and with a hand-made case; the transcribed device order (model_scan) is an order of the same sum; and the
call and the torch helpers fail loudly instead of working on the CPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import _scan_ref as S
from _scan_ref import BLOCK, OPS, RUNS, TILE, UNIT, WAVE, WIDE, flat_scan, identity, keys_of_runs, model_scan, restarts, same_values, scan_oracle, scan_terms
from test_gpu_segmented import offsets_from
from test_segmented import HEADER

VTYPES = (np.int32, np.int64, np.float32, np.float64)
# the issue's lengths: thread, wave and tile edges, empty segments, a deep start
LENGTHS = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 9000, 0, 3, 20011]
# RUNS and keys_of_runs live in _scan_ref.py, next to the layouts that are built from them


def test_symbol_in_header_exports_and_binding(rsx):
    raw = open(HEADER).read()
    assert re.search(r"#define\s+RSX_SCAN_EXCLUSIVE\s+2\b", raw)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_scan\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_scan is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "const void* d_values", "uint64_t n", "const uint64_t* d_offsets",
                      "uint64_t num_segments", "uint32_t flags", "uint32_t op", "uint32_t value_kind", "void* d_values_out"]
    assert "rsx_segmented_scan" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_scan
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_scan\b", out)
    for name in ("segmented_scan", "scan_by_key", "cumsum"):
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_scan)
    assert rsx.SCAN_EXCLUSIVE == 2 and rsx.SCAN_EXCLUSIVE & rsx.UNIQUE_CONSECUTIVE == 0


def test_hand_made_example():
    """an empty segment, off[0] = 1, an unwritten tail; key runs 7 | 3 3 | 3 -> the boundary at 4 splits equal keys | 7"""
    keys = np.array([7, 7, 3, 3, 3, 7, 7], dtype=np.uint32)
    off = np.array([1, 1, 4, 6], dtype=np.uint64)
    for form in (scan_oracle, flat_scan):
        for vt in VTYPES:
            v = np.array([1, 2, 4, 8, 16, 32, 64]).astype(vt)
            big, small = identity(vt, "min"), identity(vt, "max")
            assert restarts(7, off, keys)[0].tolist() == [False, True, True, False, True, True, False]
            assert form(v, off, keys, "sum").tolist() == [1, 2, 4, 12, 16, 32, 64]
            assert form(v, off, keys, "sum", True).tolist() == [1, 0, 0, 4, 0, 0, 64]
            assert form(v, off, keys, "min").tolist() == [1, 2, 4, 4, 16, 32, 64]
            assert form(v, off, keys, "min", True).tolist() == [1, big, big, 4, big, big, 64]
            assert form(v, off, keys, "max").tolist() == [1, 2, 4, 8, 16, 32, 64]
            assert form(v, off, keys, "max", True).tolist() == [1, small, small, 4, small, small, 64]
            # without keys: the segments [1, 4) and [4, 6)
            assert form(v, off, None, "sum").tolist() == [1, 2, 6, 14, 16, 48, 64]
            assert form(v, off, None, "sum", True).tolist() == [1, 0, 2, 6, 0, 16, 64]
            assert form(v, off, None, "max", True).tolist() == [1, small, 2, 4, small, 16, 64]
            # without offsets: the key runs of [0, 7); without either: the plain scan
            assert form(v, None, keys, "sum").tolist() == [1, 3, 4, 12, 28, 32, 96]
            assert form(v, None, None, "sum").tolist() == [1, 3, 7, 15, 31, 63, 127]
            assert form(v, None, None, "min", True).tolist() == [big, 1, 1, 1, 1, 1, 1]
        # integer sums wrap in the value's own width
        assert form(np.array([2**31 - 1, 1, 5], dtype=np.int32)).tolist() == [2**31 - 1, -(2**31), -(2**31) + 5]
        assert form(np.array([-2**63, -1], dtype=np.int64)).tolist() == [-2**63, 2**63 - 1]
        # a NaN poisons the rest of its run only; infinities are ordinary numbers
        f = np.array([1.0, np.nan, -2.0, np.inf, 5.0, -np.inf], dtype=np.float32)
        z = np.array([1, 1, 1, 2, 2, 3], dtype=np.int32)
        lo, hi = form(f, None, z, "min"), form(f, None, z, "max")
        assert lo[0] == 1 and np.isnan(lo[1:3]).all() and lo[3:].tolist() == [np.inf, 5.0, -np.inf]
        assert hi[0] == 1 and np.isnan(hi[1:3]).all() and hi[3:].tolist() == [np.inf, np.inf, -np.inf]
        # -0.0 and +0.0 keys are two runs, equal-bit NaN keys are one
        k = np.array([0.0, -0.0, np.nan, np.nan, 1.0], dtype=np.float32)
        assert form(np.arange(1, 6, dtype=np.int64), None, k, "sum").tolist() == [1, 2, 3, 7, 5]


@pytest.mark.parametrize("vt", VTYPES, ids=lambda d: np.dtype(d).name)
def test_referee_forms_agree_on_ragged_layouts(vt):
    rng = np.random.default_rng(VTYPES.index(vt))
    off = offsets_from(LENGTHS, start=3)
    n = int(off[-1]) + 5
    if np.dtype(vt).kind == "i":
        info = np.iinfo(vt)
        v = rng.integers(info.min, info.max, n, dtype=vt, endpoint=True)              # sums that wrap
    else:
        v = rng.integers(-1024, 1025, n).astype(vt)                                   # integer-valued: every order of a sum is exact
    for keys in (None, keys_of_runs(n, rng), keys_of_runs(n, rng, np.uint64, [1, 2, 3])):
        for o in (off, None):
            for op in OPS:
                w = v.copy()
                if op != "sum" and np.dtype(vt).kind == "f":
                    w[rng.integers(0, 400, n) == 0] = np.nan
                for excl in (False, True):
                    a, b = scan_oracle(w, o, keys, op, excl), flat_scan(w, o, keys, op, excl)
                    assert a.dtype == b.dtype and same_values(a, b), (op, excl)
                    lo, hi = (0, n) if o is None else (int(o[0]), int(o[-1]))
                    assert same_values(a[:lo], w[:lo]) and same_values(a[hi:], w[hi:])
    # what every inclusive sum satisfies: the last element of a segment holds the segment's sum (exact here)
    a = scan_oracle(v, off, None, "sum")
    for s in range(len(LENGTHS)):
        lo, hi = int(off[s]), int(off[s + 1])
        if hi > lo and np.dtype(vt).kind == "f":
            assert float(a[hi - 1]) == float(v[lo:hi].astype(np.float64).sum())
    m, mag = scan_terms(v.astype(np.float64), off, None)
    assert int(m[int(off[3])]) == 1 and int(m[int(off[-1]) - 1]) == 20011 and int(m[0]) == 0 and int(m[-1]) == 0


def model_cases():
    """(n, offsets, keys): runs that cross threads, waves and tiles; off[0] deep in the grid; off[S] inside a tile and on a tile's edge"""
    rng = np.random.default_rng(41)
    off = offsets_from(LENGTHS, start=3)
    n = int(off[-1]) + 5
    yield n, off, None
    yield n, off, keys_of_runs(n, rng)
    yield n, None, keys_of_runs(n, rng)
    yield 3 * TILE, None, None
    yield 5 * TILE + 7, np.array([2 * TILE + 100, 2 * TILE + 100, 3 * TILE, 5 * TILE], dtype=np.uint64), keys_of_runs(5 * TILE + 7, rng, np.uint64, [17, 300, 5000])
    yield 5000, np.array([7, 7, 4096, 4096, 4990], dtype=np.uint64), None


def test_model_scan_equals_the_oracle_where_every_order_is_exact():
    """integer-valued floats whose every partial sum is representable: every association gives the same bits, the written one included"""
    rng = np.random.default_rng(42)
    for n, off, keys in model_cases():
        for vt, vmax in ((np.float32, 256), (np.float64, 1 << 20)):               # 20011 * 256 < 2^24
            v = rng.integers(-vmax, vmax + 1, n).astype(vt)
            for excl in (False, True):
                got = model_scan(v, off, keys, excl)
                want = scan_oracle(v, off, keys, "sum", excl)
                assert got.dtype == np.dtype(vt) and np.array_equal(got, want.astype(vt)), (n, vt, excl)


def test_model_scan_within_the_any_order_bound_on_general_inputs():
    """|model - exact| <= gamma_(m-1) * sum|v| (+ the referee's own rounding, m * u_wide * sum|v|), m = elements folded"""
    rng = np.random.default_rng(43)
    for n, off, keys in model_cases():
        for vt in (np.float32, np.float64):
            v = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(vt)
            ref = scan_oracle(v, off, keys, "sum")
            got = model_scan(v, off, keys)
            wide = ref.dtype.type
            m, mag = scan_terms(v, off, keys)
            k = np.maximum(m - 1, 0).astype(wide)
            u = wide(UNIT[np.dtype(vt)])
            bound = k * u / (1 - k * u) * mag + m.astype(wide) * wide(np.finfo(wide).eps) * mag
            assert np.all(np.abs(got.astype(wide) - ref) <= bound), vt
            inc, exc = got, model_scan(v, off, keys, True)
            mask, lo, hi = restarts(n, off, keys)
            inside = np.flatnonzero(~mask[lo + 1:hi]) + lo + 1                    # the exclusive result holds the inclusive bits one place on
            assert np.array_equal(exc[inside], inc[inside - 1]) and np.all(exc[mask] == 0)
    # and the association matters on such inputs: a plain left-to-right sum gives other bits somewhere
    v = (rng.standard_normal(3 * TILE) * 10.0 ** rng.integers(-6, 7, 3 * TILE)).astype(np.float32)
    assert not np.array_equal(model_scan(v), np.add.accumulate(v, dtype=np.float32))


def test_model_scan_carry_over_70_tiles():
    """one run of 70 tiles that begins mid-tile: a second block of the grid level when it begins late in a block of 1024 tiles"""
    rng = np.random.default_rng(45)
    for start in (2000, 1000 * TILE + 2000):                                      # tiles 0 .. 70, and 1000 .. 1070 across the block edge at 1024
        n = start + 70 * TILE + 1011
        off = np.array([start, start + 70 * TILE + 1000, n - 5], dtype=np.uint64)
        v = rng.integers(-(1 << 20), (1 << 20) + 1, n).astype(np.float64)
        assert np.array_equal(model_scan(v, off), scan_oracle(v, off).astype(np.float64))
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)).astype(np.float32)
        ref = scan_oracle(v, off)
        m, mag = scan_terms(v, off)
        k = np.maximum(m - 1, 0).astype(np.float64)
        bound = k * 2.0 ** -24 / (1 - k * 2.0 ** -24) * mag + m * 2.0 ** -52 * mag
        assert np.all(np.abs(model_scan(v, off).astype(np.float64) - ref) <= bound)


def test_model_scan_hand_built_tile():
    """one tile with a restart at 20, written out by hand from the header comment of rsx_scan_by_key.hpp"""
    rng = np.random.default_rng(44)
    for vt in (np.float32, np.float64):
        f = np.dtype(vt).type
        v = (rng.standard_normal(4096) * 10.0 ** rng.integers(-3, 4, 4096)).astype(vt)
        keys = np.ones(4096, dtype=np.uint32)
        keys[:20] = 0

        def fold(a):                                  # left to right
            r = a[0]
            for t in a[1:]:
                r = f(r + t)
            return r

        got = model_scan(v, None, keys)
        assert got[5] == fold(v[:6]) and got[14] == fold(v[:15])
        assert got[15] == fold(v[:16])                                      # T(0): the thread's own fold
        assert got[17] == f(fold(v[:16]) + fold(v[16:18]))                  # G o a[1]
        assert got[20] == v[20] and got[30] == fold(v[20:31])               # after the restart of thread 1
        thread = [fold(v[16 * t:16 * t + 16]) for t in range(256)]
        thread[1] = fold(v[20:32])
        assert got[31] == thread[1]                                         # T(1): cut by the thread's own restart
        assert got[47] == f(thread[1] + thread[2])                          # T(2): distance 1 only (lane 1 holds the restart)
        assert got[63] == f(thread[1] + f(thread[2] + thread[3]))           # T(3) = x[1] o (x[2] o x[3]): distance 1, then 2
        assert got[50] == f(got[47] + fold(v[48:51]))
        # two more tiles of the same run: the grid level joins the tails by the wave scan, F(last of tile 1) = tail0 o tail1
        w = np.concatenate([v, v[::-1], v * f(3)])
        k3 = np.concatenate([keys, np.ones(8192, dtype=np.uint32)])
        g3 = model_scan(w, None, k3)
        tail0 = g3[4095]
        tail1 = model_scan(w[4096:8192])[4095]
        tail2 = model_scan(w[8192:])[4095]
        assert np.array_equal(g3[:4095], got[:4095])
        assert g3[8191] == f(tail0 + tail1) and g3[12287] == f(tail0 + f(tail1 + tail2))
        assert g3[4096] == f(tail0 + w[4096]) and g3[8192 + 16] == f(f(g3[8191] + fold(w[8192:8208])) + w[8208])


# -- the layouts of tests/test_gpu_scan_paths.py: what each reaches, and the referee on them -----------------------------------------------

PATH_LAYOUTS = {"A": lambda: S.layout_deep(), "A-keys u32": lambda: S.layout_deep(np.uint32), "A-keys u64": lambda: S.layout_deep(np.uint64),
                "B": lambda: S.layout_long(), "B-deep": lambda: S.layout_long(True), "C": lambda: S.layout_misaligned(),
                **{f"D {kind}{', keys' if kd else ''}": (lambda kind=kind, kd=kd: S.layout_dense(kind, kd))
                   for kind in ("mixed", "ones", "empty", "empty_edge") for kd in (None, np.uint32)},
                "E": lambda: S.layout_two_tiles(256), "E, no offsets": lambda: S.layout_two_tiles(256, False)}      # E as it is on 256 CUs


@pytest.mark.parametrize("name", list(PATH_LAYOUTS))
def test_model_scan_equals_the_oracle_on_the_path_layouts(name):
    """integer-valued floats with (longest run) * max|v| below 2^24 / 2^53: every partial sum of every order is representable.  (E holds
    2^24 elements: float32 only.)"""
    n, off, keys = PATH_LAYOUTS[name]()
    rng = np.random.default_rng(list(PATH_LAYOUTS).index(name) + 300)
    longest = S.longest_run(n, off, keys)
    for vt, cap, most in ((np.float32, 1 << 24, 256), (np.float64, 1 << 53, 1 << 20)):
        if n > (1 << 23) and vt is np.float64:
            continue
        vmax = min(most, (cap - 1) // max(longest, 1))
        assert vmax >= 1 and longest * vmax < cap                                  # B: a run of about 4.5M elements, |v| <= 3 in float32
        v = rng.integers(-vmax, vmax + 1, n).astype(vt)
        lo, hi = (0, n) if off is None else (int(off[0]), int(off[-1]))
        for excl in (False, True):
            got = model_scan(v, off, keys, excl)
            want = scan_oracle(v, off, keys, "sum", excl).astype(vt)
            assert got.dtype == np.dtype(vt) and np.array_equal(got, want), (name, vt, excl)
            assert np.array_equal(got[:lo], v[:lo]) and np.array_equal(got[hi:], v[hi:])


def test_path_layouts_reach_their_paths():
    """computed from each layout alone, on the grid of rsx_scan_by_key.hpp: tiles of 4096, waves of 64 tiles, carry blocks of 1024"""
    tiles_of = lambda a, b: ((b - 1) // TILE - a // TILE + 1)
    # A: off[0] deep in a wave and in a block, mid-tile; a run with tiles on both sides of tile 1024
    for kd in (None, np.uint32, np.uint64):
        n, off, keys = S.layout_deep(kd)
        a, b = S.runs_of(n, off, keys)
        t_first = int(off[0]) // TILE
        assert t_first % WAVE != 0 and t_first % BLOCK != 0 and int(off[0]) % TILE != 0
        assert np.any((a // TILE) // BLOCK < ((b - 1) // TILE) // BLOCK)
        assert (a[0], int(b[0])) == (int(off[0]), 1030 * TILE + 5 if kd else int(off[1]))
        assert keys is None or (keys.dtype == kd and np.flatnonzero(keys[1:] != keys[:-1]).tolist() == [1030 * TILE + 4])
    # B: a run over all 16 waves of a carry block and at least one wave more; deep: dead lanes before off[0], elements before it in its tile
    for deep in (False, True):
        n, off, keys = S.layout_long(deep)
        a, b = S.runs_of(n, off, keys)
        assert int(tiles_of(a, b).max()) >= BLOCK + WAVE and keys is None
        assert not deep or (0 < int(off[0]) // TILE < WAVE and int(off[0]) % TILE != 0 and int(off[-1]) < n)
    # C: two whole tiles between two partial ones
    n, off, _ = S.layout_misaligned()
    lo, hi = int(off[0]), int(off[-1])
    whole = [t for t in range((n + TILE - 1) // TILE) if t * TILE >= lo and (t + 1) * TILE <= hi]
    assert len(whole) >= 2 and 0 not in whole and hi // TILE not in whole and lo > 0 and hi < n
    # D: two groups of more than 4096 equal offsets, one of them on a tile edge, more than 1024 offsets inside one tile
    n, off, keys = S.layout_dense("mixed", np.uint32)
    o = off.astype(np.int64)
    where, count = np.unique(o, return_counts=True)
    groups = where[count > 4096]
    assert groups.size >= 2 and np.any(groups % TILE == 0) and np.any(groups % TILE != 0)
    assert int(np.bincount(o // TILE).max()) > 1024 and int(o[0]) == TILE + 17 and abs(n - 4 * TILE) < 512
    assert set(np.diff(o).tolist()) == {0, 1, 2, 3} and set(np.diff(np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1], [True]]))).tolist()) == {1, 2, 3}
    n, off, _ = S.layout_dense("ones")
    mask, lo, hi = restarts(n, off)
    assert mask[lo:hi].all() and hi - lo > 2 * TILE and lo % TILE != 0
    for kind, edge in (("empty", False), ("empty_edge", True)):
        n, off, _ = S.layout_dense(kind)
        assert n > 0 and off.size == 9 and np.all(off == off[0]) and 0 < int(off[0]) < n and (int(off[0]) % TILE == 0) == edge
    # E: two tiles per workgroup, and one at the size below
    for cus in S.CU_COUNTS:
        n = S.two_tiles_n(cus)
        tiles = (n + TILE - 1) // TILE
        assert -(-tiles // (16 * cus)) == 2 and -(-(tiles - 1) // (16 * cus)) == 1
    n, off, keys = S.layout_two_tiles(256)
    assert n == S.two_tiles_n(256) and keys.dtype == np.uint64 and keys.size == n and int(off[0]) == 3 and int(off[-1]) == n - 7
    assert S.layout_two_tiles(256, False)[1] is None


def test_referee_forms_agree_on_the_dense_layout():
    """layout D, where nearly every element is a restart: the loop over the runs and the flat form"""
    for kind in ("mixed", "ones"):
        for kd in (None, np.uint32):
            n, off, keys = S.layout_dense(kind, kd)
            rng = np.random.default_rng(320)
            for vt in (np.int32, np.float64):
                v = rng.integers(-1000, 1001, n).astype(vt)
                for op in OPS:
                    w = v.copy()
                    if op != "sum" and np.dtype(vt).kind == "f":
                        w[rng.integers(0, 50, n) == 0] = np.nan
                    for excl in (False, True):
                        a, b = scan_oracle(w, off, keys, op, excl), flat_scan(w, off, keys, op, excl)
                        assert a.dtype == b.dtype and same_values(a, b), (kind, kd, vt, op, excl)
    # every element a restart: the exclusive result is the identity everywhere in range
    n, off, _ = S.layout_dense("ones")
    lo, hi = int(off[0]), int(off[-1])
    v = np.arange(1, n + 1, dtype=np.int32)
    for op in OPS:
        assert np.all(scan_oracle(v, off, None, op, True)[lo:hi] == identity(np.int32, op))
        assert np.array_equal(scan_oracle(v, off, None, op), v)
    # nothing in range: nothing changes
    for kind in ("empty", "empty_edge"):
        n, off, keys = S.layout_dense(kind, np.uint32)
        v = np.arange(n, dtype=np.float64)
        assert np.array_equal(scan_oracle(v, off, keys), v) and np.array_equal(model_scan(v, off, keys), v) and np.array_equal(flat_scan(v, off, keys), v)


def test_a_nan_sticks_to_the_end_of_its_run_across_tiles():
    """what tests/test_gpu_scan_paths.py expects of min / max, held by the referee first: a NaN in the second tile of the first run shows
    in every later output of that run (69 and 1094 tiles; 29 where a key change ends the run) and stops at the next restart"""
    for n, off, keys in (S.layout_deep(), S.layout_deep(np.uint32), S.layout_long(True)):
        a, b = S.runs_of(n, off, keys)
        lo, end, hi = int(a[0]), int(b[0]), int(off[-1])
        pos = (lo // TILE + 1) * TILE + 77
        assert (end - pos) // TILE >= 28 and (end < hi or keys is None)
        for vt in (np.float32, np.float64):
            v = np.random.default_rng(330).uniform(1.0, 2.0, n).astype(vt)
            v[pos] = np.nan
            for op in ("min", "max"):
                for excl in (False, True):
                    for form in (scan_oracle, flat_scan) if keys is not None and vt is np.float32 else (scan_oracle,):
                        assert S.nan_sticks(form(v, off, keys, op, excl), lo, pos, end, hi, excl), (n, vt, op, excl)
            assert not S.nan_sticks(v, lo, pos, end, hi)                          # (the check can fail)


def tiny_layouts():
    off = offsets_from(LENGTHS, start=3)
    yield int(off[-1]) + 5, off
    yield 70 * TILE, None


def test_subnormals_and_negative_zero_in_the_referee():
    """what tests/test_gpu_scan_paths.py expects of sums at the bottom of the float range, held by the referee first: model_scan flushes
    nothing (where every order is exact it equals the oracle bit for bit, with partial sums on both sides of finfo.tiny), and a run of
    -0.0 sums to -0.0 at every position in both"""
    rng = np.random.default_rng(340)
    for n, off in tiny_layouts():
        lo, hi = (0, n) if off is None else (int(off[0]), int(off[-1]))
        for vt in (np.float32, np.float64):
            bits = {4: np.uint32, 8: np.uint64}[np.dtype(vt).itemsize]
            tiny = np.finfo(vt).tiny
            v = S.tiny_values(vt, n, rng, S.longest_run(n, off))
            assert np.any((v != 0) & (np.abs(v) < tiny)) and np.any(np.abs(v) >= tiny)
            for excl in (False, True):
                got, want = model_scan(v, off, None, excl), scan_oracle(v, off, None, "sum", excl)
                assert np.array_equal(want.astype(vt).astype(want.dtype), want)         # exact: the oracle's sums are values of the type
                assert np.array_equal(got.view(bits), want.astype(vt).view(bits)), (n, vt, excl)
            inc = np.abs(got[lo:hi])
            assert np.any((inc != 0) & (inc < tiny)) and np.any(inc >= tiny) and np.any(np.abs(np.diff(np.sign(inc - tiny))) == 2)
            g = S.tiny_values(vt, n, rng)                                          # the general ones of the GPU test: both ranges, too
            assert np.any((g != 0) & (np.abs(g) < tiny)) and np.any(np.abs(g) >= tiny) and not np.any(np.abs(g) > 64 * tiny)
            s = np.abs(model_scan(g, off)[lo:hi])
            assert np.any((s != 0) & (s < tiny)) and np.any(s >= tiny)
            z = g.copy()
            a, b = (0, n) if off is None else (int(off[12]), int(off[13]))         # the 9000-element segment, or everything
            assert b - a >= 9000
            z[a:b] = -0.0
            minus = np.array([-0.0], dtype=vt).view(bits)[0]
            assert minus != 0
            assert np.all(model_scan(z, off)[a:b].view(bits) == minus) and np.all(scan_oracle(z, off).astype(vt)[a:b].view(bits) == minus)


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    assert lib.rsx_segmented_scan(None, None, None, 16, None, 1, 0, 0, 0, None) == 4          # a null engine is refused
    assert b"rsx_segmented_scan" in lib.rsx_last_error()
    torch = pytest.importorskip("torch")
    keys = torch.arange(10, dtype=torch.int32)
    vals = torch.ones(10, dtype=torch.float32)
    offsets = torch.tensor([0, 10], dtype=torch.int64)
    with pytest.raises(ValueError):              # host tensors: no CPU fallback
        rsx.segmented_scan(vals, offsets)
    with pytest.raises(ValueError):
        rsx.scan_by_key(keys, vals)
    with pytest.raises(ValueError):
        rsx.cumsum(vals)
    with pytest.raises(ValueError):              # an unknown op
        rsx.segmented_scan(vals, offsets, op="prod")
    with pytest.raises(ValueError):              # shapes differ
        rsx.scan_by_key(keys, vals[:9])
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.bool):
        with pytest.raises(TypeError):           # value types outside the four
            rsx.segmented_scan(vals.to(dt), offsets)
        with pytest.raises(TypeError):
            rsx.cumsum(vals.to(dt))
    with pytest.raises(TypeError):               # key types outside _KEY_DTYPES
        rsx.scan_by_key(keys.to(torch.int16), vals)
    if not torch.cuda.is_available():
        with pytest.raises(rsx.RadixSortError) as ei:
            rsx.Engine(np.uint32, 16).segmented_scan(None, 0, 16, None, 1, rsx.REDUCE_SUM, rsx.VALUE_FLOAT32, 0)
        assert ei.value.status == 2              # INITIALIZATION_FAILED: no device, no silent CPU path
