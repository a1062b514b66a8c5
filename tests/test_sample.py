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
