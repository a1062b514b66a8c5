"""CPU tests of the categorical draw (rsx_segmented_sample; tests/test_gpu_sample.py holds the GPU ones): the header, the binding and the
exports agree; the walk over a segment's per-tile masses and the crossing inside a piece — csrc/rsx_sample_math.hpp through the
stand-alone sample_selftest, plain and under -fsanitize=address,undefined — against the referee tests/_sample_ref.py; the referee by hand
and its vectorised form against the loop form; the paths of every layout the GPU tests run, with THIS kernel's constants; and the
refusals of the C ABI without an engine and of the torch helpers on host tensors and foreign dtypes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _compact_ref
import _sample_ref as R
import _whistogram_ref
from _sample_ref import sample_loop, sample_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "radix-sort_amd", "host", "bin")
SELFTESTS = {"plain": os.path.join(BIN, "sample_selftest"), "sanitized": os.path.join(BIN, "sample_selftest_san")}
NO_TILE = 0xFFFFFFFF


def test_header_binding_and_exports_agree(rsx):
    header = open(os.path.join(ROOT, "include", "radixsort_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"int\s+rsx_segmented_sample\s*\(([^;]*)\)\s*;", text)
    assert m, "rsx_segmented_sample is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "const void* d_weights", "uint64_t n", "const uint64_t* d_offsets", "uint64_t num_segments",
                      "const void* d_bounds", "const void* d_targets", "uint32_t draws_per_segment", "uint32_t flags", "uint32_t weight_kind",
                      "int32_t weight_exp", "uint32_t* d_index_out", "uint64_t* d_mass_out", "uint64_t* d_total_out"]
    for name, value in (("RSX_WSELECT_FRACTION", R.FRACTION), ("RSX_COMPACT_INVERT", R.INVERT), ("RSX_COMPACT_STRICT", R.STRICT)):
        d = re.search(r"#define\s+" + name + r"\s+(\d+)", header)
        assert d and int(d.group(1)) == value, name
    assert (rsx.WSELECT_FRACTION, rsx.COMPACT_INVERT, rsx.COMPACT_STRICT) == (128, 16, 32)
    assert "rsx_segmented_sample" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_sample
    P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert fn.argtypes == [P, P, P, U64, P, U64, P, P, U32, U32, U32, C.c_int32, P, P, P]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_sample\b", out)
    assert all(callable(f) for f in (rsx.segmented_sample, rsx.multinomial, rsx.sample_rows, rsx.Engine.segmented_sample))


def test_kernel_constants_match_the_referee():
    math = open(os.path.join(ROOT, "radix-sort_amd", "csrc", "rsx_sample_math.hpp")).read()
    for pattern, value in ((r"constexpr int kTileShift = (\d+);", 12), (r"constexpr uint32_t kWalkLane = (\d+);", R.WALK_LANE),
                           (r"constexpr uint32_t kWalkTiles = (\d+);", R.WALK_TILES)):
        m = re.search(pattern, math)
        assert m and int(m.group(1)) == value, pattern
    assert R.TILE == 1 << 12 == _compact_ref.TILE and R.WALK_TILES == 64 * R.WALK_LANE
    src = open(os.path.join(ROOT, "radix-sort_amd", "csrc", "rsx_sample.hpp")).read()
    m = re.search(r"constexpr int kSampleThreads = (\d+);", src)
    assert m and int(m.group(1)) == 64 * R.WAVES
    assert "kSampleGroup = kWave * rsx_sample::kWalkLane" in src and R.GROUP == 64 * R.WALK_LANE
    inc = open(os.path.join(ROOT, "radix-sort_amd", "csrc", "capi_sample.inc")).read()
    m = re.search(r"\(slots \+ waves - 1\) / waves, cus \* (\d+)\)", inc)
    assert m and int(m.group(1)) == R.DRAW_PER_CU


# -- the walk and the crossing as the kernel takes them -------------------------------------------------------------------------------------------

def _walk_line(ta, masses, T):
    return f"W {ta} {ta + len(masses) - 1} {T} " + " ".join(str(int(v)) for v in masses) + "\n"


def _walk_want(ta, masses, T):
    run = 0
    for i, m in enumerate(masses):
        if run < T <= run + int(m):
            return f"W {ta + i} {run}"
        run += int(m)
    return f"W {NO_TILE} {run}"


def _locate_want(masses, before, T):
    run = before
    for i, m in enumerate(masses):
        run += int(m)
        if int(m) and run - int(m) < T <= run:
            return f"L {i} {run}"
    return f"L {len(masses)} {run}"


def _selftest_cases():
    """(line, expected output): partial sequences with zero-mass tiles and chunks, targets at 0, 1, total, total + 1 and at every chunk
    boundary's prefix and that prefix + 1; pieces with zero masses and a running mass to begin with"""
    rng = np.random.default_rng(11)
    cases = []
    for ntiles in (1, 2, 3, R.WALK_LANE, R.WALK_TILES - 1, R.WALK_TILES, R.WALK_TILES + 1, 2 * R.WALK_TILES, 3 * R.WALK_TILES + 5):
        for style in ("random", "sparse", "hollow", "zero"):
            m = rng.integers(1, 1 << 44, ntiles)
            if style == "sparse":
                m[rng.random(ntiles) < 0.7] = 0
            elif style == "hollow":
                m[1:-1] = 0                                         # only the first and the last tile weigh anything
            elif style == "zero":
                m[:] = 0
            if style == "sparse" and ntiles > R.WALK_TILES:
                m[R.WALK_TILES:2 * R.WALK_TILES] = 0                # a whole chunk without mass
            ta = int(rng.integers(0, 1 << 19))
            total = int(m.sum())
            prefix = [int(m[:c].sum()) for c in range(R.WALK_TILES, ntiles, R.WALK_TILES)]
            ends = np.cumsum(m)[rng.integers(0, ntiles, 4)].tolist()
            targets = {0, 1, total, total + 1, total // 2, *prefix, *(p + 1 for p in prefix), *ends, *(e + 1 for e in ends)}
            targets |= {int(rng.integers(1, total + 1)) for _ in range(4)} if total else set()
            for T in sorted(targets):
                cases.append((_walk_line(ta, m, T), _walk_want(ta, m, T)))
    for count in (0, 1, 5, 64, 255, 256, 257, 4096):
        m = rng.integers(0, 1 << 32, count)
        m[rng.random(count) < 0.5] = 0
        before = int(rng.integers(0, 1 << 40))
        total = int(m.sum())
        for T in sorted({0, 1, before, before + 1, before + total, before + total + 1, before + total // 2, *(before + int(v) for v in np.cumsum(m)[:3])}):
            cases.append((f"L {count} {before} {T} " + " ".join(str(int(v)) for v in m) + "\n", _locate_want(m, before, T)))
    return cases


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_selftest_walk_and_crossing(tmp_path, which):
    exe = SELFTESTS[which]
    assert os.path.exists(exe), "run __graft_entry__.build()"
    cases = _selftest_cases()
    assert len(cases) > 400
    path = tmp_path / "cases.txt"
    path.write_text("".join(line for line, _ in cases))
    proc = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, (proc.returncode, proc.stderr[-2000:])                 # 2: the chunked walk differs from the linear scan
    lines = proc.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for (line, want), got in zip(cases, lines):
        assert got == want, (line[:200], got, want)
    # found and not found, in the first chunk and in a later one, behind a chunk without mass
    tiles = [(int(c[0].split()[1]), int(g.split()[1])) for c, g in zip(cases, lines) if g.startswith("W")]
    assert any(t == NO_TILE for _, t in tiles) and any(t != NO_TILE and t - ta >= 2 * R.WALK_TILES for ta, t in tiles)
    assert any(t != NO_TILE and t - ta < R.WALK_TILES for ta, t in tiles)


def test_selftest_refuses_absurd_lines(tmp_path):
    for text in ("X 1 2 3\n", "W 5 4 1 7\n", "W 0 1 1 7\n", "W 0 0 1\n", "W 0 0 1 -3\n", "W 0 4294967295 1 7\n", "L 2 0 1 5\n", "L 4194305 0 1\n",
                 "W 0 0 1 17592186044417\n", "L 1 9223372036854775807 1 1\n", "W 0 0\n", "L\n", "W 0 0 1 x\n"):
        path = tmp_path / "bad.txt"
        path.write_text(text)
        assert subprocess.run([SELFTESTS["plain"], str(path)], capture_output=True).returncode == 1, text
        assert subprocess.run([SELFTESTS["sanitized"], str(path)], capture_output=True).returncode == 1, text


# -- the referee ---------------------------------------------------------------------------------------------------------------------------------

def test_referee_by_hand():
    w = np.array([3, 0, 2, 5], dtype=np.uint32)
    index, mass, written, total = sample_oracle(w, None, np.arange(1, 11, dtype=np.uint64))
    assert index[0].tolist() == [0, 0, 0, 2, 2, 3, 3, 3, 3, 3] and written.all() and total.tolist() == [10]
    assert mass[0].tolist() == [3, 3, 3, 5, 5, 10, 10, 10, 10, 10]
    assert np.bincount(index[0], minlength=4).tolist() == w.tolist()               # each index is drawn exactly `mass` times, the zero never
    index, mass, written, total = sample_oracle(w, None, np.array([0, 11], dtype=np.uint64))
    assert not written.any()
    p = np.array([0.5, 0.25, 0.25], dtype=np.float32)
    u = np.array([0.0, 0.5, np.nextafter(0.5, 1.0), 0.75, 1.0, np.nan])
    index, mass, written, total = sample_oracle(p, None, u, fraction=True)
    assert total.tolist() == [1 << 31] and written[0].tolist() == [True] * 5 + [False]
    assert index[0, :5].tolist() == [0, 0, 1, 1, 2] and mass[0, :5].tolist() == [1 << 30, 1 << 30, 3 << 29, 3 << 29, 1 << 31]
    # a bound: descending, keep p >= 0.25 strictly above it: only the first element weighs anything
    index, mass, written, total = sample_oracle(None, None, u, fraction=True, keys=p, bounds=np.array([0.25], dtype=np.float32), descending=True,
                                                strict=True)
    assert total.tolist() == [1 << 30] and index[0, :5].tolist() == [0] * 5


@pytest.mark.parametrize("wdt", ["uint32", "float32", "float64", "self"])
def test_referee_forms_agree_on_the_ragged_layout(wdt):
    n, off = _compact_ref.ragged_layout()
    for c, (bound, descending) in enumerate(((None, False), ("bound", False), ("strict", True), ("invert", True))):
        rng = np.random.default_rng(300 + c)
        wexp = {"uint32": 0, "float32": -3, "float64": 5, "self": 0}[wdt]
        if wdt == "self":
            keys, w = _whistogram_ref.case_weights(rng, np.float32, n, off, wexp), None
        else:
            keys, w = rng.integers(0, 50, n).astype(np.int32), _whistogram_ref.case_weights(rng, np.dtype(wdt), n, off, wexp)
        kw = dict(keys=keys, descending=descending, weight_exp=wexp)
        if bound:
            kw.update(bounds=keys[rng.integers(0, n, len(off) - 1)], strict=bound == "strict", invert=bound == "invert")
        ref = R.Referee(w, off, **kw)
        for fraction in (False, True):
            t = _sample_targets(ref.total, 3, rng, fraction)
            index, mass, written, total = ref(t, fraction)
            loop, totals = sample_loop(w, off, t, fraction, **kw)
            assert totals == total.tolist()
            assert [(int(i), int(m)) if ok else (None, None) for i, m, ok in zip(index.ravel(), mass.ravel(), written.ravel())] == loop
            assert written.any() and not written.all()
            assert np.all(ref.m[off.astype(np.int64)[:-1, None].repeat(3, 1)[written] + index[written]] > 0)       # an answer has mass


def _sample_targets(total, Rr, rng, fraction):
    import _wselect_ref
    t = _wselect_ref.random_targets(total, Rr, rng)
    if not fraction:
        return t
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(total[:, None] > 0, t.astype(np.float64) / np.maximum(total[:, None], 1).astype(np.float64), rng.random(t.shape))
    u[rng.random(u.shape) < 0.1] = np.nan
    return u


# -- the paths: every layout of the GPU tests reaches the path it is named for --------------------------------------------------------------------------

def test_layouts_reach_their_paths():
    ones = lambda n: np.ones(n, dtype=np.int64)
    n, off = R.one_tile_layout()
    f = R.walk_facts(ones(n), off, 0)
    assert f["one_tile"] and f["tiles"] == (1, 1) and R.tile_sums(n, off) == [None, None, None]      # read by its draws alone
    n, off = R.crossing_layout()
    f = R.walk_facts(ones(n), off, 1)
    assert f["tiles"] == (0, 1) and f["pieces"] == [1000, 2000] and f["chunks"] == 1 and R.tile_sums(n, off) == ["tail", "lead"]
    assert all(R.walk_facts(ones(n), off, s)["one_tile"] for s in (0, 2))
    n, off = R.hollow_layout()
    f = R.walk_facts(ones(n), off, 1)
    assert f["tiles"] == (0, 5) and len(f["pieces"]) == 6 and R.tile_sums(n, off)[:6] == ["tail", "both", "both", "both", "both", "lead"]
    n, off = R.long_layout()
    f = R.walk_facts(ones(n), off, R.LONG_SEGMENT)
    assert f["chunks"] == 2 and len(f["pieces"]) == R.WALK_TILES + 2 and len(f["chunk_prefix"]) == 1
    assert int(off[R.LONG_SEGMENT + 1] - off[R.LONG_SEGMENT]) == (R.WALK_TILES + 1) * R.TILE + 17
    assert len(R.long_targets(ones(n), off)) == 4
    sums = R.tile_sums(n, off)
    assert sums.count("both") >= R.WALK_TILES and "lead+tail" in sums                                 # tile 1: segment 0 ends, segment 1 begins
    n, off = R.many_layout()
    grid, slots = R.draw_grid(len(off) - 1, 1)
    assert slots == R.MANY_SEGMENTS > grid * R.WAVES and set(np.diff(off.astype(np.int64)).tolist()) == set(range(8))
    assert set(R.tile_sums(n, off)) <= {None, "lead", "tail", "lead+tail"}
    n, off = R.inner_layout()
    o = off.astype(np.int64)
    assert o[0] > R.TILE and o[0] % R.TILE and o[-1] < n - R.TILE and o[-1] % R.TILE
    assert R.tile_sums(n, off)[0] is None and R.tile_sums(n, off)[-1] is None and "both" in R.tile_sums(n, off)
    # the ragged matrix has segments inside a tile, over one edge and over several
    n, off = _compact_ref.ragged_layout()
    kinds = {(f["one_tile"], f["chunks"]) for f in (R.walk_facts(ones(n), off, s) for s in range(len(off) - 1))}
    assert kinds == {(True, 0), (True, 1), (False, 1)} and "both" in R.tile_sums(n, off)


# -- the launch paths of tests/test_gpu_sample_paths.py, from the layouts alone, at 256 CUs and at one other count ----------------------------------

def _not_read_run(walk):
    """the longest run of consecutive tiles that sample_tile_kernel does not read, over the workgroups in order"""
    best = run = 0
    for kind in (k for g in walk for k in g):
        run = run + 1 if kind is None else 0
        best = max(best, run)
    return best


@pytest.mark.parametrize("cus", [256, 304, 128])
def test_two_tile_layout_reaches_its_paths(cus):
    n, off, names = R.two_tile_layout(cus)
    o = off.astype(np.int64)
    assert n == (16 * cus + 3) * R.TILE + 77 and R.tile_grid(n, cus) == (2, 8 * cus + 2)
    walk = R.group_walk(n, off, cus)
    assert len(walk) == 8 * cus + 2 and all(len(g) == 2 for g in walk)
    assert walk[0] == ("outside", "tail")                                          # off[0] in a workgroup's second tile
    assert walk[1] == ("both", "lead+tail")                                        # two block sums behind a tile already summed
    assert walk[-1] == ("lead", "outside") and o[-1] % R.TILE and o[-1] < n        # off[S] in a workgroup's first tile
    assert _not_read_run(walk) >= 3 and walk[4] == walk[5] == (None, None)
    lens = np.diff(o)
    first = names["short"]
    assert int((lens[first:names["before_bulk"]] == 7).sum()) >= 1800 and o[first] == 8 * R.TILE and o[names["before_bulk"]] == 12 * R.TILE
    # a segment ends and another begins on one tile edge, with empty segments before and on it
    e, b = names["to_edge"], names["from_edge"]
    assert o[e + 1] == o[b] == 5 * R.TILE and b == e + 3 and not lens[e + 1:b].any() and not lens[names["empty"]:e].any() and e == names["empty"] + 3
    assert (o[b + 1] - o[b]) == 3 * R.TILE and o[e] // R.TILE == 3
    ones = np.ones(n, dtype=np.int64)
    assert R.walk_facts(ones, off, names["two_edges"])["tiles"] == (1, 3) and R.walk_facts(ones, off, names["few"])["one_tile"]
    # the bulk: at least 3 walk chunks (16 at 256 CUs), from a tile that is no multiple of 4 to the first tile of a workgroup
    s = names["bulk"]
    a, z = R.weightless_chunk(off, s)
    m = ones.copy()
    m[a:z] = 0
    f = R.walk_facts(m, off, s)
    ta, tb = f["tiles"]
    assert f["chunks"] >= (16 if cus >= 256 else 3) and ta % 4 != 0 and tb % 2 == 0 and tb == 16 * cus + 2
    assert (a, z) == ((ta + R.WALK_TILES) * R.TILE, (ta + 2 * R.WALK_TILES) * R.TILE) and z < o[s + 1]
    assert f["chunk_prefix"][1] == f["chunk_prefix"][0] > 0 and f["chunk_prefix"][2] > f["chunk_prefix"][1]      # the weightless chunk
    assert not any(f["pieces"][R.WALK_TILES:2 * R.WALK_TILES]) and all(f["pieces"][:R.WALK_TILES])
    t = R.chunk_targets(m, off, s)
    assert len(t) == 2 + 2 * min(8, f["chunks"] - 1) <= 32


@pytest.mark.parametrize("cus", [256, 304, 128])
def test_second_trip_layout_reaches_its_path(cus):
    n, off, names = R.second_trip_layout(cus)
    nseg = len(off) - 1
    grid, slots = R.draw_grid(nseg, R.SECOND_TRIP_R, cus)
    assert nseg == 48 * cus and grid == 32 * cus and slots == 144 * cus > R.WAVES * grid
    assert all(s * R.SECOND_TRIP_R >= R.WAVES * grid and s >= nseg - 5 * cus for s in names.values())           # every planted slot in the second trip
    ones = np.ones(n, dtype=np.int64)
    facts = {name: R.walk_facts(ones, off, s) for name, s in names.items()}
    assert facts["two_tiles"]["chunks"] == 1 and len(facts["two_tiles"]["pieces"]) == 2
    assert facts["long"]["chunks"] == 2 and len(facts["long"]["pieces"]) == 300
    assert facts["empty"]["tiles"] is None and facts["one_tile"]["one_tile"] and int(off[names["one_tile"] + 1] - off[names["one_tile"]]) == 3000
    a, z = R.weightless_chunk(off, names["long"])
    m = ones.copy()
    m[a:z] = 0
    f = R.walk_facts(m, off, names["long"])
    assert z == int(off[names["long"] + 1]) and sum(f["pieces"][R.WALK_TILES:]) == 0 and f["chunk_prefix"][0] == sum(f["pieces"]) > 0
    lens = np.diff(off.astype(np.int64))
    small = np.delete(lens, [s for s in names.values()] + [s - 1 for s in names.values()])
    assert set(small.tolist()) == set(range(8))


def test_group_layout_and_targets():
    n, off = R.group_layout()
    ones = np.ones(n, dtype=np.int64)
    f = R.walk_facts(ones, off, R.GROUP_ONE_TILE)
    a = int(off[R.GROUP_ONE_TILE])
    assert f["one_tile"] and a == R.TILE + 1001 and a % 4 and f["pieces"] == [3000] and divmod(3000, R.GROUP) == (11, 184)
    f = R.walk_facts(ones, off, R.GROUP_TWO_TILES)
    assert f["pieces"] == [3595, 1001] and int(off[0]) % 4 and all(p % R.GROUP for p in f["pieces"])
    assert [e for e, _ in R.group_edges(ones, off, R.GROUP_ONE_TILE)] == list(range(256, 3000, 256)) + [3000]
    assert [e for e, _ in R.group_edges(ones, off, R.GROUP_TWO_TILES)] == list(range(256, 3595, 256)) + [3595] + list(range(3595 + 256, 4596, 256)) + [4596]
    # a group of zero mass: its end's prefix repeats and is dropped; nothing is 0 or above the total
    m = ones.copy()
    m[a + 3 * R.GROUP:a + 4 * R.GROUP] = 0
    t = R.group_targets(m, off, R.GROUP_ONE_TILE)
    assert t == sorted(set(t)) and t[0] == 256 and t[-1] == 3000 - 256 and 768 in t and 769 in t and len(t) == 2 * 11 - 1
    assert len(R.group_targets(ones, off, R.GROUP_TWO_TILES)) == 2 * 19 - 1


def test_huge_total_layout_passes_2_to_53_in_both_directions():
    n, off = R.huge_total_layout()
    length = int(off[1] - off[0])
    assert length == (1 << 22) + 3 * R.TILE + 5 and int(off[0]) > 0 and n > int(off[1])
    f = R.walk_facts(np.ones(n, dtype=np.int64), off, 0)
    assert len(f["pieces"]) == 1028 and f["chunks"] == 5
    up, down = length * 0xFFFFFFFF, length * 0xFFFFFFFD
    assert up > down > 1 << 53
    assert int(float(up)) - up == 1 and int(float(down)) - down == -1              # the double nearest the total lies above it, and below it
    w = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    assert int(R.Referee(w, off).total[0]) == up and int(R.Referee(w - np.uint32(2), off).total[0]) == down


def test_first_suite_stays_on_one_tile_per_workgroup():
    """the gap that tests/test_gpu_sample_paths.py closes: no layout of tests/test_gpu_sample.py gives a workgroup of sample_tile_kernel a
    second tile at any CU count from 64 on, or a walk a third chunk"""
    layouts = [f() for f in R.LAYOUTS.values()] + [_compact_ref.ragged_layout(), (3 * 4096 + 17, np.array([7, 5000, 5000, 3 * 4096 + 7], dtype=np.uint64))]
    for n, off in layouts:
        assert R.tile_grid(n, 64)[0] == R.tile_grid(n, 256)[0] == 1
        ones = np.ones(n, dtype=np.int64)
        long_ones = np.flatnonzero(np.diff(off.astype(np.int64)) > R.TILE)
        assert all(R.walk_facts(ones, off, s)["chunks"] <= 2 for s in long_ones)
    n, off = R.many_layout()
    assert R.draw_grid(len(off) - 1, 1)[1] > R.WAVES * R.draw_grid(len(off) - 1, 1)[0] and np.diff(off.astype(np.int64)).max() <= 7     # the one second trip: R = 1, short segments


# -- no CPU path ---------------------------------------------------------------------------------------------------------------------------------

def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    assert lib.rsx_segmented_sample(None, None, None, 0, None, 1, None, None, 1, 0, 1, 0, None, None, None) == 4     # a null engine
    assert lib.rsx_last_error() == b"rsx_segmented_sample: null engine"
    torch = pytest.importorskip("torch")
    w = torch.rand(10)
    off = torch.tensor([0, 4, 10], dtype=torch.int64)
    u = torch.rand(2, dtype=torch.float64)
    for call in (lambda: rsx.segmented_sample(w, off, u=u), lambda: rsx.segmented_sample(w, None, targets=torch.ones(1, dtype=torch.int64)),
                 lambda: rsx.segmented_sample(w, off, u=u, bound=torch.zeros(2), descending=True),
                 lambda: rsx.segmented_sample(torch.ones(10, dtype=torch.int32), off, u=u),
                 lambda: rsx.multinomial(w.reshape(2, 5), 3), lambda: rsx.multinomial(w.double(), 1, u=torch.rand(1, dtype=torch.float64)),
                 lambda: rsx.sample_rows(w.reshape(2, 5)), lambda: rsx.sample_rows(w.reshape(2, 5), top_p=0.9),
                 lambda: rsx.sample_rows(w.reshape(2, 5), top_k=2, min_p=0.1)):
        with pytest.raises(ValueError, match="device tensor"):      # host tensors: no CPU fallback
            call()


def test_dtype_refusals(rsx):
    torch = pytest.importorskip("torch")
    off = torch.tensor([0, 4, 10], dtype=torch.int64)
    u = torch.rand(2, dtype=torch.float64)
    for bad in (torch.ones(10, dtype=torch.float16), torch.ones(10, dtype=torch.bfloat16), torch.ones(10, dtype=torch.bool), torch.ones(10, dtype=torch.int64)):
        for call in (lambda: rsx.segmented_sample(bad, off, u=u), lambda: rsx.multinomial(bad.reshape(2, 5), 1), lambda: rsx.sample_rows(bad.reshape(2, 5))):
            with pytest.raises(TypeError, match=r"unsupported weight type .* \(float32, float64, or int32 / uint32 masses\)"):
                call()
    with pytest.raises(TypeError, match="float32 and float64"):
        rsx.sample_rows(torch.ones(2, 5, dtype=torch.int32))
    for call in (lambda: rsx.segmented_sample([0.5] * 10, off, u=u), lambda: rsx.multinomial(np.ones((2, 5), dtype=np.float32), 1)):
        with pytest.raises(TypeError, match="must be a tensor"):
            call()
