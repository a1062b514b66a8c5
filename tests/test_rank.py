"""CPU tests of the segmented rank (rsx_segmented_rank; tests/test_gpu_rank.py holds the GPU ones): the header, the binding and the exports
agree; the referee tests/_rank_ref.py by hand for all five methods and against scipy.stats.rankdata where scipy is installed; the carries
over a sorted segment's tiles and the rank rule — csrc/rsx_rank_math.hpp through the stand-alone rank_selftest, plain and under
-fsanitize=address,undefined — against the referee; the argument errors of the torch helpers that need no device; the one-lexsort form of
the referee against the looped one; and every layout of tests/test_gpu_rank_paths.py pinned to the launch path it is named for, at three
CU counts where the path depends on the count."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _rank_ref as R
import _segmented_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "radix-sort_amd", "host", "bin")
SELFTESTS = {"plain": os.path.join(BIN, "rank_selftest"), "sanitized": os.path.join(BIN, "rank_selftest_san")}


def test_header_binding_and_exports_agree(rsx):
    header = open(os.path.join(ROOT, "include", "radixsort_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"int\s+rsx_segmented_rank\s*\(([^;]*)\)\s*;", text)
    assert m, "rsx_segmented_rank is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "uint64_t n", "const uint64_t* d_offsets", "uint64_t num_segments", "uint32_t flags",
                      "uint32_t method", "uint32_t* d_rank_out", "uint32_t* d_ties_out"]
    assert "rsx_segmented_rank" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_rank
    P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert fn.argtypes == [P, P, U64, P, U64, U32, U32, P, P]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_rank\b", out)
    assert all(callable(f) for f in (rsx.segmented_rank, rsx.rankdata, rsx.Engine.segmented_rank))


def test_method_codes_match_header_binding_and_kernels(rsx):
    header = open(os.path.join(ROOT, "include", "radixsort_hip.h")).read()
    math = open(os.path.join(ROOT, "radix-sort_amd", "csrc", "rsx_rank_math.hpp")).read()
    m = re.search(r"kOrdinal = (\d+), kMin = (\d+), kMax = (\d+), kDense = (\d+), kAverage = (\d+);", math)
    assert m and [int(v) for v in m.groups()] == [0, 1, 2, 3, 4]
    for name, value in (("ORDINAL", 0), ("MIN", 1), ("MAX", 2), ("DENSE", 3), ("AVERAGE", 4)):
        d = re.search(r"#define\s+RSX_RANK_" + name + r"\s+(\d+)", header)
        assert d and int(d.group(1)) == value == getattr(rsx, "RANK_" + name) == getattr(R, name), name
    assert rsx.RANK_METHODS == R.METHODS


# -- the referee ----------------------------------------------------------------------------------------------------------------------------------

def test_referee_by_hand():
    x = np.array([30, 10, 20, 10, 30, 30], dtype=np.int32)
    ranks, ties = R.rank_segment(x)
    assert ranks[R.ORDINAL].tolist() == [3, 0, 2, 1, 4, 5]
    assert ranks[R.MIN].tolist() == [3, 0, 2, 0, 3, 3]
    assert ranks[R.MAX].tolist() == [5, 1, 2, 1, 5, 5]
    assert ranks[R.DENSE].tolist() == [2, 0, 1, 0, 2, 2]
    assert ranks[R.AVERAGE].tolist() == [8, 1, 4, 1, 8, 8]                      # min + max
    assert ties.tolist() == [3, 2, 1, 2, 3, 3]
    ranks, ties = R.rank_segment(x, descending=True)
    assert ranks[R.ORDINAL].tolist() == [0, 4, 3, 5, 1, 2]
    assert ranks[R.MIN].tolist() == [0, 4, 3, 4, 0, 0] and ranks[R.DENSE].tolist() == [0, 2, 1, 2, 0, 0]
    # signed keys, and floats in totalOrder: -NaN < -inf < -0.0 < +0.0 < +inf < +NaN; equal-bit NaNs tie
    ranks, _ = R.rank_segment(np.array([-1, 0, -2 ** 31, 2 ** 31 - 1], dtype=np.int32))
    assert ranks[R.ORDINAL].tolist() == [1, 2, 0, 3]
    nan_neg = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    f = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, nan_neg, np.nan, 1.0], dtype=np.float32)
    ranks, ties = R.rank_segment(f)
    assert ranks[R.MIN].tolist() == [3, 2, 6, 5, 1, 0, 6, 4]
    assert ties.tolist() == [1, 1, 2, 1, 1, 1, 2, 1]
    # the whole call: two groups across a segment boundary, an empty segment, positions outside [off[0], off[S]) untouched
    x = np.array([9, 5, 5, 5, 5, 7, 9], dtype=np.uint32)
    ranks, ties, written = R.rank_oracle(x, [1, 3, 3, 6], fill=77)
    assert ranks[R.MAX].tolist() == [77, 1, 1, 1, 1, 2, 77] and ties.tolist() == [77, 2, 2, 2, 2, 1, 77]
    assert written.tolist() == [False, True, True, True, True, True, False]


def test_referee_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(5)
    for L in (1, 2, 17, 300):
        x = rng.integers(-6, 6, L).astype(np.int64)
        ranks, _ = R.rank_segment(x)
        for name, code in R.METHODS.items():
            want = stats.rankdata(x, method=name)
            got = ranks[code].astype(np.float64) / 2 + 1 if name == "average" else ranks[code].astype(np.int64) + 1
            assert np.array_equal(got, want), (L, name)


# -- the rule and the carries as the kernels take them -----------------------------------------------------------------------------------------------

def _case(tile, a, runs):
    """(line of the case file, expected output) of a sorted segment given as (value, count) runs"""
    keys = np.repeat(np.array([v for v, _ in runs], dtype=np.uint64), [c for _, c in runs])
    L = len(keys)
    ranks, ties = R.rank_segment(keys)                                          # already sorted: sorted order = index order
    T = (a + L + tile - 1) // tile if L else 0
    lines = [f"S {L} {T}"] + [" ".join(str(int(v)) for v in row) for row in list(ranks) + [ties]]
    return f"S {tile} {a} {len(runs)} " + " ".join(f"{v} {c}" for v, c in runs) + "\n", "\n".join(lines)


def _selftest_cases():
    rng = np.random.default_rng(3)
    cases = [
        _case(4, 0, [(1, 2), (2, 3), (3, 3)]),                                  # a run spanning no whole tile, crossing one edge
        _case(4, 0, [(1, 3), (2, 6), (3, 3)]),                                  # ... one whole tile (positions 4..7 hold no head)
        _case(4, 1, [(1, 2), (2, 14), (3, 1)]),                                 # ... three whole tiles, from a segment that starts mid-tile
        _case(4, 0, [(7, 16)]),                                                 # one run: only the first tile holds a head
        _case(4, 0, [(1, 4), (2, 4)]),                                          # the segment ends on a tile edge, heads on the edges
        _case(4, 3, [(1, 1), (2, 8)]),                                          # ... after a first tile of one key
        _case(4, 2, [(5, 1)]),
        _case(R.TILE, 100, [(1, 5), (2, 3 * R.TILE + 5), (3, 7)]),              # the kernels' tile: 12 293 equal keys in the middle
        _case(R.TILE, 0, [(v, 1) for v in range(2 * R.TILE)]),                  # strictly increasing
    ]
    for _ in range(40):
        tile = int(rng.integers(1, 9))
        runs, v = [], 0
        for _ in range(int(rng.integers(1, 12))):
            v += int(rng.integers(1, 3))
            runs.append((v, int(rng.integers(1, 3 * tile + 2))))
        cases.append(_case(tile, int(rng.integers(0, tile)), runs))
    return cases


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_selftest_matches_the_referee(build, tmp_path):
    exe = SELFTESTS[build]
    assert os.path.exists(exe), f"{exe} is missing (build() makes it)"
    cases = _selftest_cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(line for line, _ in cases))
    proc = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, (proc.returncode, proc.stderr[-2000:])
    assert proc.stdout == "".join(want + "\n" for _, want in cases)


@pytest.mark.parametrize("text", ["X 1 2\n", "S 0 0 1 5 1\n", "S 4 4 1 5 1\n", "S 4 0 1 5 0\n", "S 4 0 2 5 1\n"])
def test_selftest_refuses_malformed_files(text, tmp_path):
    path = tmp_path / "bad.txt"
    path.write_text(text)
    assert subprocess.run([SELFTESTS["plain"], str(path)], capture_output=True).returncode == 1


# -- the helpers' argument errors -----------------------------------------------------------------------------------------------------------------

def test_helper_argument_errors(rsx):
    torch = pytest.importorskip("torch")
    x = torch.zeros(8, dtype=torch.float32)
    off = torch.tensor([0, 8], dtype=torch.int64)
    for call in (lambda **kw: rsx.segmented_rank(x, off, **kw), lambda **kw: rsx.rankdata(x, **kw)):
        with pytest.raises(ValueError, match="method"):
            call(method="first")
        with pytest.raises(ValueError, match="method"):
            call(method=1)
        with pytest.raises(ValueError, match="device tensor"):
            call()
    for dtype in (torch.bfloat16, torch.float16, torch.bool):
        with pytest.raises(TypeError, match="unsupported key type"):
            rsx.rankdata(torch.zeros(4, dtype=dtype))
        with pytest.raises(TypeError, match="unsupported key type"):
            rsx.segmented_rank(torch.zeros(4, dtype=dtype), off)


# -- the referee in one lexsort; the layouts of tests/test_gpu_rank_paths.py reach their paths ----------------------------------------------------

CU_COUNTS = [256, 304, 128]                                                     # those of tests/test_sample.py
MIXED_LENGTHS = [0, 1, 2, 260, 0, 1200, 3500, 30000, 1, 4097, 700, 9000, 4096, 0]      # tests/test_gpu_rank.py's, from 37 with a tail of 50


def _same(many, looped):
    return all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(many, looped))


@pytest.mark.parametrize("descending", [False, True])
def test_oracle_many_equals_the_looped_oracle_on_the_mixed_layout(descending):
    rng = np.random.default_rng(40 + descending)
    off = S.offsets_from(MIXED_LENGTHS, start=37)
    n = int(off[-1]) + 50
    for dt in (np.uint32, np.float64, np.int64):
        x = (rng.standard_normal(n) * 2).round().astype(dt) if np.dtype(dt).kind == "f" else rng.integers(0, 9, n).astype(dt)
        assert _same(R.rank_oracle_many(x, off, descending, fill=0xC3C3C3C3), R.rank_oracle(x, off, descending, fill=0xC3C3C3C3)), np.dtype(dt).name


def test_oracle_many_equals_the_looped_oracle_on_many_tiny_segments():
    rng = np.random.default_rng(42)
    off = S.offsets_from(rng.integers(0, 4, 5000), start=2)
    n = int(off[-1]) + 3
    x = rng.integers(-2, 2, n).astype(np.int32)
    many, looped = R.rank_oracle_many(x, off, fill=5), R.rank_oracle(x, off, fill=5)
    assert _same(many, looped) and not many[2][:2].any() and not many[2][-3:].any() and many[2][2:-3].all()
    none = R.rank_oracle_many(x, np.array([4, 4, 4], dtype=np.uint64), fill=5)                        # nothing inside any segment
    assert not none[2].any() and np.all(none[0] == 5) and np.all(none[1] == 5)


def test_rank_geometry_by_hand():
    # 3 segments at 256 CUs: a one-key, a class-0 and a large one of 3 tiles (it begins at 4090 and ends at 4090 + 4200 = 8290 > 8192)
    off = np.array([4000, 4001, 4090, 8290], dtype=np.uint64)
    g = R.rank_geometry(off, 9000, 256)
    assert (g["ones"], g["count"], g["nlarge"], g["tiles"]) == (1, [1, 0, 0], 1, 3) and (g["max_large"], g["max_tiles"]) == (2, 5)
    assert (g["ones_grid"], g["ones_trips"], g["small_trips"], g["tile_grid"], g["tile_trips"], g["join_grid"], g["join_trips"]) == (1, 1, [1, 0, 0], 5, 1, 2, 1)
    assert (g["T"], g["join_per"], g["join_used"]) == ([3], [1], [3])
    flat = R.rank_geometry(None, 257 * R.TILE - 100, 256)
    assert (flat["nlarge"], flat["tiles"], flat["T"], flat["join_per"], flat["join_used"]) == (1, 257, [257], [2], [129])
    assert (flat["ones_trips"], flat["small_trips"], flat["tile_grid"], flat["tile_trips"], flat["join_grid"], flat["join_trips"]) == (0, [0, 0, 0], 257, 1, 1, 1)
    assert R.rank_geometry(None, 5000, 256)["T"] == [2] and R.rank_geometry(None, 5, 256)["T"] == [1]


def test_join_facts_by_hand():
    # a segment from global index 4094: tiles of 2, 4096 and 3 keys.  Sorted keys: 5 | 5 ... 5 7 | 7 8 8
    s = np.concatenate([[5, 5], np.full(4095, 5), [7], [7, 8, 8]]).astype(np.uint32)
    f = R.join_facts(4094, s)
    assert f["edges"] == [(1, 0, 0), (1, 4097, 4097), (1, 4099, 4099)] and (f["T"], f["per"], f["used"], f["idle"]) == (3, 1, 3, 253)
    assert f["last_key_head"] and not f["first_key_head"] and not f["wave_headless"] and f["thread_headless"] == [False] * 3
    s = np.concatenate([[5, 6], np.full(4096, 7), [8, 8, 8]]).astype(np.uint32)             # the run of 7 fills tile 1 exactly
    f = R.join_facts(4094, s)
    assert f["edges"] == [(2, 0, 1), (1, 2, 2), (1, 4098, 4098)] and f["first_key_head"] and f["last_key_head"] and f["all_heads_tiles"] == 1
    s = np.zeros(3 * R.TILE, dtype=np.uint64)                                    # one run over three whole tiles
    f = R.join_facts(0, s)
    assert f["edges"] == [(1, 0, 0), (0, None, None), (0, None, None)] and f["thread_headless"] == [False, True, True]
    assert R.tile_facts(0, s) == (True, True)


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_stride_layouts_give_the_small_kernel_a_second_trip(cus):
    for cls in range(3):
        n, off = S.stride_layout(cls, cus)
        g = R.rank_geometry(off, n, cus)
        assert g["small_trips"][cls] == 2 and g["count"][cls] > g["grid"][cls] == cus * S.PER_CU[cls] and g["nlarge"] == 0
        lens = np.diff(off.astype(np.int64))
        order, grid = g["lists"][cls], g["grid"][cls]
        second = np.arange(grid, g["count"][cls])
        assert np.all(lens[order[second]] < lens[order[second - grid]])          # the second item runs over a longer segment's image


def test_pad_equal_layout_and_keys():
    n, off, planted = R.pad_equal_layout()
    g = R.rank_geometry(off, n, 256)
    lens = np.diff(off.astype(np.int64))
    assert g["count"] == [3, 3, 3] and g["ones"] == 3 and g["nlarge"] == 1 and lens[g["large"][0]] == 4097 + 300 and len(planted) == 10
    for c, tile in enumerate(R.CLASS_TILE):
        assert sorted(lens[g["lists"][c]].tolist()) == sorted([tile - 1, tile - 17, 2 * tile // 3]) and max(lens[g["lists"][c]]) < tile
    assert [R.pad_value(dt, d).view(np.uint32).item() for dt, d in R.PAD_PAIRS] == [0xFFFFFFFF, 0, 0x7FFFFFFF, 0xFFFFFFFF]
    for i, (dt, descending) in enumerate(R.PAD_PAIRS):
        x, counts = R.pad_equal_keys(dt, descending, n, off, planted, np.random.default_rng(i))
        pad = R.pad_value(dt, descending).view(np.uint32)
        ranks, ties, _ = R.rank_oracle(x, off, descending)
        for s in planted:
            a, b = int(off[s]), int(off[s + 1])
            at = np.flatnonzero(x[a:b].view(np.uint32) == pad)
            assert len(at) == counts[s] == (b - a) // 3 + 5 and np.all(at[-((b - a) // 3):] == np.arange(b - (b - a) // 3, b) - a)
            assert np.all(ties[a:b][at] == counts[s]) and np.all(ranks[R.MAX][a:b][at] == b - a - 1) and np.all(ranks[R.MIN][a:b][at] == b - a - counts[s])
            assert int(ranks[R.DENSE][a:b].max()) == int(ranks[R.DENSE][a:b][at[0]]) >= 2          # the last run of the segment, behind others


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_sparse_large_reaches_the_ones_second_trip(cus):
    n, off = S.sparse_large()
    g = R.rank_geometry(off, n, cus)
    assert g["ones_trips"] >= 2 and g["per"] == 2 and g["small_trips"][0] >= 2 and g["nlarge"] >= 30 and g["large_blocks"] >= 30
    assert g["ones"] > 100000 and g["ones_grid"] == cus * 4
    if cus == 256:
        assert (g["ones_trips"], g["small_trips"][0], g["nlarge"], g["large_blocks"]) == (3, 37, 43, 41)
    nb, bad = S.sparse_large_bad()
    assert nb == n and R.rank_geometry(bad, n, cus)["first_bad"] == 550001


def test_join_layout_reaches_every_path_of_the_join():
    n, off, names, runs = R.join_layout()
    g = R.rank_geometry(off, n, 256)
    o = off.astype(np.int64)
    assert g["T"] == list(R.JOIN_TILES) == [65, 256, 385] and g["join_per"] == [1, 1, 2] and g["join_used"] == [65, 256, 193]
    assert all(o[s] % R.TILE for s in names.values()) and g["large"].tolist() == list(names.values()) and g["count"][1] and g["count"][2] and g["ones"]
    for dt, descending in (("uint32", False), ("float64", True)):
        x = R.join_keys(dt, descending, n, off, names, runs, np.random.default_rng(3))
        facts = [R.join_facts(a, s) for a, s in R.sorted_keys_layout(x, off, descending)]
        t65, t256, t385 = facts
        paths = R.join_paths(facts)
        assert all(paths.values()), [name for name, reached in paths.items() if not reached]
        assert (t65["used"], t65["idle"]) == (65, 191) and not t65["thread_headless"][64] and any(t65["thread_headless"])      # one record in the second wave
        assert (t256["per"], t256["used"], t256["idle"]) == (1, 256, 0) and t256["wave_headless"] and all(t256["thread_headless"][61:195])
        assert not t256["thread_headless"][60] and not t256["thread_headless"][195]
        assert (t385["per"], t385["used"], t385["idle"], t385["last_thread_tiles"]) == (2, 193, 63, 1)
        assert t385["thread_headless"][7] and t385["thread_headless"][8] and not t385["thread_headless"][6] and not t385["thread_headless"][9]
        assert t385["first_key_head"] and t385["last_key_head"] and t385["all_heads_tiles"] >= 8 and t385["wave_headless"]
        assert all(t385["thread_headless"][51:192]) and not t385["thread_headless"][50] and not t385["thread_headless"][192]
        e = t385["edges"]
        assert e[12][0] == 1 and all(t[0] == 0 for t in e[13:18]) and e[11][2] == e[12][1] - 1     # the 6-tile run begins with tile 12, behind a one-key run ...
        assert e[18][1] == e[12][1] + 6 * R.TILE and e[19][2] == e[18][1] + 2 * R.TILE - 1          # ... and ends with tile 17; a run from tile 19's last key


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_grid_stride_layout_reaches_the_second_trips(cus):
    n, off = R.grid_stride_layout(cus)
    g = R.rank_geometry(off, n, cus)
    lens = np.diff(off.astype(np.int64))
    assert g["nlarge"] == cus * 8 + 40 and g["join_grid"] == g["tile_grid"] == cus * 8 and g["join_trips"] == 2 and g["tile_trips"] >= 2
    assert 0 <= g["max_large"] - g["nlarge"] <= 3 and int(off[0]) == 5 and int(off[-1]) == n and g["ones"] >= 2 and (lens == 0).sum() >= 4
    large = lens[g["large"]]
    assert large.min() == R.TILE + 1 and R.TILE + 100 < large.max() <= R.TILE + 204 and set(g["T"]) <= {2, 3} and g["count"] == [0, 0, 0]


def test_flat_sizes_cover_every_regime():
    assert [R.flat_regime(n) for n in R.FLAT_SIZES] == ["small-tile self-scan", "self-scan", "self-scan", "self-scan", "look-ahead chain"]
    assert R.flat_regime(4096) == "one tile" and R.flat_regime(5000) == "small-tile self-scan"
    assert [R.flat_regime(n, 8) for n in R.FLAT_SIZES_8BIT] == ["8-bit chain"] * 2
    assert max(R.FLAT_SIZES) <= R.FLAT_CAPACITY
    per = [R.rank_geometry(None, n, 256)["join_per"][0] for n in R.FLAT_SIZES]
    assert per == [1, 1, 2, 4, 5] and R.rank_geometry(None, R.FLAT_SIZES[2], 256)["join_used"] == [129]
    # tests/test_gpu_rank.py's flat form stops at 10 000 keys: one tile and the small-tile self-scan only
    assert {R.flat_regime(n) for n in (1, 5, 4096, 4097, 10000)} == {"one tile", "small-tile self-scan"}


def test_replay_layouts_keep_the_size_and_change_the_classes():
    n = sum(MIXED_LENGTHS) + 37 + 50
    base = R.rank_geometry(S.offsets_from(MIXED_LENGTHS, start=37), n, 256)
    assert base["count"] == [1, 2, 3] and base["nlarge"] == 3 and base["ones"] == 2
    seen = {}
    for name, lengths in R.REPLAY_LENGTHS.items():
        off = S.offsets_from(lengths, start=R.REPLAY_STARTS[name])
        assert len(lengths) == len(MIXED_LENGTHS) and int(off[-1]) <= n
        g = R.rank_geometry(off, n, 256)
        assert g["chain_ok"] == 1 and g["nlarge"] <= g["max_large"] == base["max_large"]
        seen[name] = (g["count"], g["nlarge"], g["ones"])
    assert seen["another class mix"] == ([3, 2, 3], 3, 2) and seen["no large segment"] == ([3, 2, 7], 0, 1) and seen["large or empty"] == ([0, 0, 0], 6, 0)


def test_first_suite_stays_on_the_first_trips():
    """what tests/test_gpu_rank.py's largest call reaches: one trip everywhere, join records in the first eight threads of one wave"""
    off = S.offsets_from(MIXED_LENGTHS, start=37)
    g = R.rank_geometry(off, sum(MIXED_LENGTHS) + 87, 256)
    assert g["ones_trips"] == 1 and max(g["small_trips"]) == 1 and g["tile_trips"] == 1 and g["join_trips"] == 1 and g["per"] == 1
    assert max(g["T"]) <= 9 and max(g["join_per"]) == 1
