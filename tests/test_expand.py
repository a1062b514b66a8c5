"""CPU checks of the expand: header, exports, binding and the Python callables agree on rsx_segmented_expand; the host referee
(tests/_expand_ref.py) agrees with np.repeat, with the owner rule through np.searchsorted and with brute force; every layout the GPU tests
run reaches the kernel path it is named for; the stand-alone expand_selftest — the owner rule and the tile arithmetic the kernels call,
compiled by g++ — gives the referee's owners, ranks, splits and store counts on those layouts, plain and as a second stand-alone binary
built with -fsanitize=address,undefined (nothing is loaded into Python under a sanitizer); and the call and the torch helpers fail loudly
instead of working on the CPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _expand_ref as R
from _expand_ref import FILL, GENERAL, NONE, TILE
from test_search import header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "radix-sort_amd", "host", "bin")
SELFTESTS = {"plain": os.path.join(BIN, "expand_selftest"), "sanitized": os.path.join(BIN, "expand_selftest_san")}
HELPERS = ("segmented_expand", "segment_ids", "segment_ranks", "repeat_interleave", "broadcast_segments", "gather_ranges", "pack_rows")


def test_header_binding_and_exports_agree(rsx):
    text = re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S)
    m = re.search(r"int\s+rsx_segmented_expand\s*\(([^;]*)\)\s*;", text)
    assert m, "rsx_segmented_expand is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_values", "uint64_t num_values", "uint32_t value_bytes", "const uint64_t* d_offsets",
                      "uint64_t num_segments", "uint64_t n", "const uint64_t* d_starts", "uint32_t flags", "void* d_values_out",
                      "uint32_t* d_segment_out", "uint32_t* d_rank_out"]
    flag = re.search(r"#define\s+RSX_EXPAND_GATHER\s+(\d+)", header_text())
    assert flag and int(flag.group(1)) == 64 == rsx.EXPAND_GATHER
    taken = [rsx.UNIQUE_CONSECUTIVE, rsx.SCAN_EXCLUSIVE, rsx.SEARCH_RIGHT, rsx.COMPACT_PARTITION, rsx.COMPACT_INVERT, rsx.COMPACT_STRICT]
    assert sorted(taken) == [1, 2, 4, 8, 16, 32]                  # bits 0-5; the expand has bit 6
    assert "rsx_segmented_expand" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_expand
    P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert fn.argtypes == [P, P, U64, U32, P, U64, U64, P, U32, P, P, P]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_expand\b", out)
    for name in HELPERS:
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_expand)


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    assert lib.rsx_segmented_expand(None, None, 0, 4, None, 1, 16, None, 0, None, None, None) == 4         # a null engine is refused
    assert lib.rsx_last_error() == b"rsx_segmented_expand: null engine"
    torch = pytest.importorskip("torch")
    off = torch.tensor([0, 3, 10], dtype=torch.int64)
    vals = torch.ones(2, dtype=torch.float32)
    for call in (lambda: rsx.segmented_expand(off, vals), lambda: rsx.segment_ids(off), lambda: rsx.segment_ranks(off, n=10),
                 lambda: rsx.repeat_interleave(vals, 2), lambda: rsx.repeat_interleave(torch.tensor([1, 2])),
                 lambda: rsx.broadcast_segments(vals, off), lambda: rsx.gather_ranges(vals, off[:-1], off[1:]),
                 lambda: rsx.pack_rows(torch.ones(2, 3), torch.tensor([1, 2]))):
        with pytest.raises(ValueError):                            # host tensors: no CPU fallback
            call()


# -- the referee ---------------------------------------------------------------------------------------------------------------------------

def test_referee_against_np_repeat_and_brute_force():
    rng = np.random.default_rng(1)
    for trial in range(60):
        lens = rng.integers(0, 6, int(rng.integers(1, 40)))
        lens[rng.integers(0, lens.size)] = int(rng.integers(0, 50))
        off = R.offsets_from(lens, start=int(rng.integers(0, 9)))
        seg, rank = R.owners(off)
        assert np.array_equal(seg, np.repeat(np.arange(lens.size), lens))
        assert np.array_equal(rank, np.concatenate([np.arange(k) for k in lens] + [np.zeros(0, dtype=np.int64)]))
        for other in (R.owners_searchsorted(off), R.owners_brute(off)):
            assert np.array_equal(seg, other[0]) and np.array_equal(rank, other[1])
        n = int(off[-1]) + int(rng.integers(0, 5))
        vals = rng.integers(0, 1 << 32, lens.size, dtype=np.uint32)
        vout, sout, rout, written = R.expand_oracle(off, n, vals)
        assert written.sum() == lens.sum() and np.all(sout[~written] == 0xC3C3C3C3) and np.all(vout[~written] == 0xC3C3C3C3)
        assert np.array_equal(vout[written], np.repeat(vals, lens)) and np.array_equal(sout[written], seg) and np.array_equal(rout[written], rank)
        src = rng.integers(0, 1 << 32, 200, dtype=np.uint32)
        starts = rng.integers(0, 200 - int(lens.max()) + 1, lens.size)
        gout = R.expand_oracle(off, n, src, starts)[0]
        want = np.concatenate([src[a:a + k] for a, k in zip(starts, lens)] + [np.zeros(0, dtype=np.uint32)])
        assert np.array_equal(gout[written], want)
    assert R.valid([0, 5, 4, 9], 9) == 1 and R.valid([0, 5, 10], 9) == 1 and R.valid([0, 5, 9], 9) is None
    assert R.valid([0, 5, 9], 9, starts=[0, 7], num_values=10) == 1 and R.valid([0, 5, 9], 9, starts=[5, 6], num_values=10) is None


# -- the layouts of the GPU tests ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.LAYOUTS) + list(R.BIG_LAYOUTS))
def test_layouts_reach_the_paths_they_are_named_for(name):
    make, want = {**R.LAYOUTS, **R.BIG_LAYOUTS}[name]
    n, off = make()
    assert R.valid(off, n) is None if len(off) < 100000 else bool(np.all(np.diff(off.astype(np.int64)) >= 0) and int(off[-1]) <= n)
    got = R.paths(off, n)
    assert want <= got, (name, sorted(want - got))


def test_layout_sizes_are_the_ones_asked_for():
    assert [R.LAYOUTS[k][0]()[0] for k in ("one of 1", "one of 4095", "one of 4096", "one of 4097", "one of 3 tiles + 5")] == [1, 4095, 4096, 4097, 3 * 4096 + 5]
    n, off = R.layout_all_ones()
    assert n == 2 * TILE + 3 and [p for p, _, _ in R.tile_paths(off, n)] == [GENERAL] * 3 and R.tile_paths(off, n)[0][1] == TILE
    n, off = R.layout_one(3 * TILE + 5)
    assert [p for p, _, _ in R.tile_paths(off, n)] == [GENERAL, FILL, FILL, GENERAL]
    n, off = R.layout_dense_empties()
    assert len(off) - 1 == TILE + 302 and R.tile_paths(off, n) == [(GENERAL, TILE + 303, 5)]
    n, off = R.layout_ragged_ends()
    assert n == 2 * TILE + 11 and int(off[0]) == 5 and int(off[-1]) == n - 3
    n, off = R.layout_empties("all")
    assert [p for p, _, _ in R.tile_paths(off, n)] == [NONE]
    for e in (0, 1, 7):
        n, off = R.layout_edges(e)
        o = off.astype(np.int64)
        assert all(np.count_nonzero(o == k * TILE) == e + 1 for k in range(4))
    n, off = R.layout_multi_tile()
    assert n == (1 << 24) + 4099 and len(off) - 1 == 4099 and R.tiles_per_workgroup(n) == 2
    n, off = R.layout_many_segments()
    assert len(off) - 1 == (1 << 20) + 4099
    n, off = R.layout_zipf()
    assert abs(n - (1 << 18)) < 16


# -- the stand-alone program: the kernels' own functions on the CPU ----------------------------------------------------------------------------

def selftest(tmp_path, which, off, n, addr, eb):
    path = tmp_path / "case.txt"
    path.write_text(f"{len(off) - 1} {n} {addr} {eb}\n" + " ".join(str(int(v)) for v in off) + "\n")
    proc = subprocess.run([SELFTESTS[which], str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    assert proc.stderr == "", proc.stderr[-2000:]                  # a sanitizer report would stand here
    own, tiles = [], []
    for line in proc.stdout.splitlines():
        f = line.split()
        (own if f[0] == "o" else tiles).append([int(v) for v in f[1:]])
    return np.array(own, dtype=np.int64).reshape(-1, 2), tiles


def stores_of(addr, eb, a, b):
    """head, 16-byte stores, tail of [a, b) for an output at byte address addr: counted element by element"""
    per = 16 // eb
    full = [g for g in range((addr // eb + a) // per, (addr // eb + b) // per + 1) if g * per >= addr // eb + a and (g + 1) * per <= addr // eb + b]
    if not full:
        head = min((-(addr // eb + a)) % per, b - a)
        return head, 0, b - a - head
    return full[0] * per - (addr // eb + a), len(full), addr // eb + b - (full[-1] + 1) * per


@pytest.mark.parametrize("which", list(SELFTESTS))
@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_selftest_on_the_layouts(tmp_path, name, which):
    n, off = R.LAYOUTS[name][0]()
    seg, rank = R.owners(off)
    lo, hi = int(off[0]), int(off[-1])
    paths = R.tile_paths(off, n)
    o = off.astype(np.int64)
    for addr, eb in ((0, 4), (4, 4), (8, 4), (12, 4), (0, 8), (8, 8)):
        own, tiles = selftest(tmp_path, which, off, n, addr, eb)
        assert np.array_equal(own[:, 0], seg) and np.array_equal(own[:, 1], rank)
        assert len(tiles) == len(paths)
        for (t, s_lo, s_hi, a, b, head, nvec, tail), (path, k, _) in zip(tiles, paths):
            assert (s_lo, s_hi) == (int(np.count_nonzero(o < t * TILE)), int(np.count_nonzero(o < (t + 1) * TILE)))
            if path == NONE:
                assert a >= b
                continue
            assert (a, b) == (max(lo, t * TILE), min(hi, (t + 1) * TILE)) and s_hi - s_lo == k
            assert (head, nvec, tail) == stores_of(addr, eb, a, b)
            assert head < 16 // eb and tail < 16 // eb and head + nvec * (16 // eb) + tail == b - a
            assert (addr + (a + head) * eb) % 16 == 0 or nvec == 0
            if path == FILL:
                assert 1 <= s_lo <= len(off) - 1 and np.all(seg[a - lo:b - lo] == s_lo - 1)


def test_selftest_refuses_bad_cases(tmp_path):
    for text in ("2 10 0 4\n0 5 4\n", "2 10 0 4\n0 5 11\n", "2 10 2 4\n0 5 10\n", "2 10 0 3\n0 5 10\n", "2 10 0 4\n0 5\n"):
        path = tmp_path / "bad.txt"
        path.write_text(text)
        for exe in SELFTESTS.values():
            assert subprocess.run([exe, str(path)], capture_output=True, text=True).returncode == 1, text
