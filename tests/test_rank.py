"""CPU tests of the segmented rank (rsx_segmented_rank; tests/test_gpu_rank.py holds the GPU ones): the header, the binding and the exports
agree; the referee tests/_rank_ref.py by hand for all five methods and against scipy.stats.rankdata where scipy is installed; the carries
over a sorted segment's tiles and the rank rule — csrc/rsx_rank_math.hpp through the stand-alone rank_selftest, plain and under
-fsanitize=address,undefined — against the referee; and the argument errors of the torch helpers that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _rank_ref as R

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
