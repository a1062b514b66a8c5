"""CPU checks of the histogram: header, exports, binding and the Python callables agree on rsx_segmented_histogram; the two forms of the
host referee (tests/_histogram_ref.py) agree with each other, with numpy and with torch on the CPU; the stand-alone bins_selftest — the
functions the kernels call, compiled by g++ — gives the referee's bin for every key of cases built around the edges of the arithmetic;
the layouts the GPU tests run reach the paths they are named after; and the call and the torch helpers fail loudly instead of working on
the CPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _histogram_ref as H
from _histogram_ref import NO_BIN, bins_of, histogram_loop, histogram_oracle, piece_paths, piece_slots
from _search_ref import UINT
from test_search import header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "radix-sort_amd", "host", "bin", "bins_selftest")
HELPERS = ("segmented_histogram", "bincount", "histc", "histogram", "bincount_rows", "histogram_rows")


def test_symbol_in_header_exports_and_binding(rsx):
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_histogram\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_histogram is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "uint64_t n", "const uint64_t* d_offsets", "uint64_t num_segments", "const void* d_edges",
                      "uint64_t lo_bits", "uint64_t hi_bits", "uint32_t width_shift", "uint64_t num_bins", "uint32_t flags", "uint32_t* d_counts_out"]
    assert "rsx_segmented_histogram" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_histogram
    P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert fn.argtypes == [P, P, U64, P, U64, P, U64, U64, U32, U64, U32, P]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_histogram\b", out)
    for name in HELPERS:
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_histogram)


def test_constants_match_the_kernel_header():
    """tests/_histogram_ref.py states the kernels' constants; the numbers are those of rsx_bins.hpp"""
    src = lambda f: open(os.path.join(ROOT, "radix-sort_amd", "csrc", f)).read()
    num = lambda text, name: int(re.search(name + r"\s*=\s*(\d+)", text).group(1))
    bins = src("rsx_bins.hpp")
    assert num(bins, "kBinsLdsMax") == H.LDS_MAX and num(bins, "kBinsWavePrivateMax") == H.WAVE_PRIVATE_MAX
    assert 1 << num(bins, "kBinsDirectShift") == H.DIRECT_PIECE
    uniq = src("rsx_unique.hpp")
    assert num(uniq, "kUniqThreads") * num(uniq, "kUniqKpt") == H.TILE
    assert int(re.search(r"kNoBin\s*=\s*0x([0-9A-Fa-f]+)", src("rsx_bin_math.hpp")).group(1), 16) == NO_BIN
    import _compact_ref
    import test_search
    assert H.LENGTHS == test_search.LENGTHS and H.BIG_N == _compact_ref.BIG_N
    assert H.empties_layout()[0] == _compact_ref.empties_layout()[0] and np.array_equal(H.empties_layout()[1], _compact_ref.empties_layout()[1])


def small_case(dt, form, descending, rng):
    """a ragged case small enough for the loop: off[0] = 2, empty segments, ties with every edge (or lo and hi), specials for floats"""
    off = H.offsets_from([0, 1, 5, 0, 17, 33, 2, 0, 64, 3], start=2)
    n = int(off[-1]) + 3
    args = H.form_args(dt, form, descending, 7, rng)
    return H.case_keys(rng, dt, n, off, args), off, args


@pytest.mark.parametrize("form", ["even", "edges"])
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt", H.DTYPES)
def test_referee_forms_agree(dt, descending, form):
    """six dtypes x two directions x three forms (even is the integer or the float form by dtype)"""
    rng = np.random.default_rng(H.DTYPES.index(dt) * 4 + descending * 2 + (form == "edges"))
    keys, off, args = small_case(dt, form, descending, rng)
    a = histogram_oracle(keys, off, descending=descending, **args)
    b = histogram_loop(keys, off, descending=descending, **args)
    assert a.shape == (len(off) - 1, 7) and np.array_equal(a, b)
    assert np.all(a.sum(axis=1) <= np.diff(off.astype(np.int64)))
    assert a.sum() > 0 and a.sum() < int(off[-1] - off[0])          # something is counted, something is dropped
    if np.dtype(dt).kind != "f" or form == "edges":
        # descending: the even form numbers its bins backwards; reversed edges give reversed bins but for the closed end
        if form == "even":
            up = histogram_oracle(keys, off, descending=False, **args)
            assert np.array_equal(a, up[:, ::-1] if descending else up)


@pytest.mark.parametrize("dt", H.DTYPES)
def test_ascending_edges_equal_numpy_histogram(dt):
    rng = np.random.default_rng(50 + H.DTYPES.index(dt))
    dt = np.dtype(dt)
    for B in (1, 2, 7, 64):
        edges = H.sorted_edges(rng, dt, B, H.SPAN)
        if dt.kind == "f":
            edges = edges[np.isfinite(edges)]
        keys = H.random_keys(rng, dt, 3000, H.SPAN)
        keys[:edges.size] = edges                                  # ties on every edge
        if dt.kind == "f":
            keys = keys[np.isfinite(keys) & ~((keys == 0) & np.signbit(keys))]          # numpy orders by value: no NaN, no -0.0
        want = np.histogram(keys, bins=edges)[0]
        assert np.array_equal(histogram_oracle(keys, None, edges)[0], want), B


@pytest.mark.parametrize("dt", ["uint32", "int32", "uint64", "int64"])
def test_even_integer_form_equals_bincount(dt):
    rng = np.random.default_rng(60 + H.DTYPES.index(dt))
    x = rng.integers(0, 300, 5000).astype(dt)
    for B in (1, 17, 300, 1000):
        assert np.array_equal(histogram_oracle(x, None, B)[0], np.bincount(x.astype(np.int64), minlength=B)[:B]), B
    # a shift is a division of the distance from lo by a power of two
    assert np.array_equal(histogram_oracle(x, None, 4, lo=44, shift=5)[0], np.histogram(x.astype(np.int64), bins=[44, 76, 108, 140, 172 - 1e-9])[0])
    if np.dtype(dt).kind == "i":
        y = (x.astype(np.int64) - 150).astype(dt)
        assert np.array_equal(histogram_oracle(y, None, 300, lo=-150)[0], np.bincount(x.astype(np.int64), minlength=300))


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_even_float_form_equals_numpy_and_torch_on_exact_inputs(dt):
    """integer-valued floats on a power-of-two range: every operation is exact, so numpy, torch.histc and the referee agree"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(70 + H.DTYPES.index(dt))
    x = rng.integers(-40, 100, 4000).astype(dt)
    for B, lo, hi in ((64, 0.0, 64.0), (16, -32.0, 32.0), (128, 0.0, 64.0), (1, -8.0, 8.0)):
        got = histogram_oracle(x, None, B, lo=lo, hi=hi)[0]
        assert np.array_equal(got, np.histogram(x, bins=B, range=(lo, hi))[0]), (B, lo, hi)
        assert np.array_equal(got, torch.histc(torch.from_numpy(x), bins=B, min=lo, max=hi).numpy().astype(np.int64)), (B, lo, hi)


# -- the stand-alone program: the kernels' own functions on the CPU ----------------------------------------------------------------------------

def selftest_bins(tmp_path, keys, bins, lo=0, hi=0, shift=0, descending=False, expect=0):
    dt = keys.dtype
    u = UINT[dt.itemsize]
    even = np.isscalar(bins)
    edges = np.array([], dtype=dt) if even else np.ascontiguousarray(bins, dtype=dt)
    bits = lambda v: int(np.array([v], dtype=dt).view(u)[0])
    head = [dt.itemsize, {"u": 0, "i": 1, "f": 2}[dt.kind], int(descending), 0 if even else 2, int(bins) if even else edges.size - 1,
            bits(lo) if even else 0, bits(hi) if even and dt.kind == "f" else 0, shift, edges.size, keys.size]
    path = tmp_path / "case.txt"
    path.write_text(" ".join(str(v) for v in head) + "\n" + " ".join(str(int(v)) for v in edges.view(u)) + "\n" + " ".join(str(int(v)) for v in keys.view(u)) + "\n")
    proc = subprocess.run([SELFTEST, str(path)], capture_output=True, text=True)
    assert proc.returncode == expect, proc.stderr
    return np.array([int(v) for v in proc.stdout.split()], dtype=np.int64)


# (the cases are drawn in tests/_histogram_ref.py: tests/test_gpu_histogram_paths.py sends the same keys through the kernels)

@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt", H.DTYPES)
def test_selftest_edges_form(tmp_path, dt, descending):
    for B, edges, keys in H.edges_cases(dt, descending):
        want = bins_of(keys, edges, descending=descending)
        assert np.array_equal(selftest_bins(tmp_path, keys, edges, descending=descending), want), B
        assert np.any(want == NO_BIN) and np.any(want == B - 1) and np.any(want == 0)


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt", ["uint32", "int32", "uint64", "int64"])
def test_selftest_even_integer_form(tmp_path, dt, descending):
    dt = np.dtype(dt)
    for shift, lo, B, keys in H.even_int_cases(dt, descending):
        want = bins_of(keys, B, lo=lo, shift=shift, descending=descending)
        assert np.array_equal(selftest_bins(tmp_path, keys, B, lo=lo, shift=shift, descending=descending), want), (shift, lo, B)
    selftest_bins(tmp_path, np.zeros(1, dtype=dt), 4, shift=8 * dt.itemsize, expect=2)           # width_shift < 8 * key_bytes


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_selftest_even_float_form(tmp_path, dt, descending):
    dt = np.dtype(dt)
    for B, lo, hi, keys in H.even_float_cases(dt, descending):
        want = bins_of(keys, B, lo=lo, hi=hi, descending=descending)
        assert np.array_equal(selftest_bins(tmp_path, keys, B, lo=lo, hi=hi, descending=descending), want), (B, lo, hi)
        H.even_float_case_holds(keys, B, lo, hi, want, descending)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, np.inf), (np.nan, 1.0), (-np.finfo(dt).max, np.finfo(dt).max)):
        selftest_bins(tmp_path, np.zeros(1, dtype=dt), 4, lo=lo, hi=hi, expect=2)       # refused: not finite, not lo < hi, no finite scale


# -- the layouts of the GPU tests --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(H.LAYOUTS))
def test_layouts_reach_their_paths(name):
    layout, B, want = H.LAYOUTS[name]
    n, off = layout()
    paths = piece_paths(n, off, B)
    assert {p[3] for p in paths} == want, name
    o = H._offsets(n, off)
    assert sum(p[2] for p in paths) == int(o[-1] - o[0])            # the pieces are the live elements, once each
    if name == "big_one_segment":
        assert H.chunk_of(n) == 2 and sum(p[3] == "lds_first" for p in paths) == (n // H.TILE + 1 + 1) // 2      # one flush a workgroup, not one a tile
    if name == "big_boundaries":
        assert H.chunk_of(n) == 2
        by_tile = {}
        for t, s, L, path in paths:
            by_tile.setdefault(t, []).append((s, path))
        assert by_tile[3] == [(0, "lds_same"), (1, "lds_flush")]     # a flush in the middle of a workgroup's second tile
        assert by_tile[8] == [(1, "lds_first"), (2, "lds_flush")]
        assert by_tile[13] == [(2, "lds_same"), (3, "direct")] and by_tile[14][0] == (3, "direct")
    if name in ("pairs", "fifties"):
        assert max(p[2] for p in paths) < H.DIRECT_PIECE
    assert H.lds_layout(64) == "wave_private" and H.lds_layout(1024) == "wave_private" and H.lds_layout(1025) == "shared"
    assert H.lds_layout(4096) == "shared" and H.lds_layout(4097) == "none"


@pytest.mark.parametrize("form", ["even", "edges"])
@pytest.mark.parametrize("dt", H.DTYPES)
def test_matrix_cases_hold_what_they_promise(dt, form):
    """the ragged matrix of the GPU tests: out-of-range keys, ties with every edge, lo and hi occur inside the segments"""
    n, off = H.ragged_layout()
    o = off.astype(np.int64)
    for descending in (False, True):
        for B in H.MATRIX_BINS:
            rng = np.random.default_rng(1000 + H.DTYPES.index(dt) * 100 + B)
            args = H.form_args(dt, form, descending, B, rng)
            keys = H.case_keys(rng, dt, n, off, args)
            live = keys[o[0]:o[-1]]
            b = bins_of(live, descending=descending, **args)
            assert np.any(b == NO_BIN) and np.any(b != NO_BIN)
            u = UINT[np.dtype(dt).itemsize]
            if form == "edges":
                assert np.all(np.isin(args["bins"].view(u), live.view(u)))
            else:
                assert np.any(live == np.dtype(dt).type(args["lo"]))
                if np.dtype(dt).kind == "f":
                    assert np.any(live == np.dtype(dt).type(args["hi"])) and np.any(np.isnan(live)) and np.any(np.isinf(live))


# -- the layouts of tests/test_gpu_histogram_paths.py ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", H.DTYPES)
def test_arithmetic_cases_take_the_lds_and_the_direct_path(dt):
    """every case of the three selftests above, in the three forms the GPU test sends it in: as one segment and as two segments its keys
    are counted in LDS (but for B = 50257, the direct path by itself), cut into pieces of 255 keys they all go the direct way"""
    dt = np.dtype(dt)
    cases = 0
    for descending in (False, True):
        sized = [(B, keys.size) for B, _, keys in H.edges_cases(dt, descending)]
        if dt.kind == "f":
            sized += [(B, keys.size) for B, _, _, keys in H.even_float_cases(dt, descending)]
        else:
            sized += [(B, keys.size) for _, _, B, keys in H.even_int_cases(dt, descending)]
        for B, size in set(sized):
            forms = H.arith_forms(size)
            assert [f[0] for f in forms] == ["one segment", "two segments", "pieces of 255"]
            for name, n, off in forms:
                assert n >= size and n > 2 * H.DIRECT_PIECE
                pieces = piece_paths(n, off, B)
                assert sum(p[2] for p in pieces) == n
                if name == "pieces of 255" or B > H.LDS_MAX:
                    assert {p[3] for p in pieces} == {"direct"} and (name != "pieces of 255" or max(p[2] for p in pieces) == 255)
                elif name == "one segment":
                    assert pieces[0][3] == "lds_first" and pieces[0][2] > H.DIRECT_PIECE
                else:
                    cut = int(off[1])
                    assert cut % 2 == 1 and [p[3] for p in pieces if p[0] == cut // H.TILE] == ["lds_first", "lds_flush"]      # both sides of the cut in LDS
            cases += 1
        assert {B for B, _ in sized} >= ({1, 2, 13, 4096} | ({50257, 100} if dt.kind == "f" else {3, 64}))
    assert cases >= 10


def test_slot_layouts_reach_every_slot_and_the_direct_boundary():
    """the four piece-slot layouts, B = 64 and B = 4096: slots 0 .. 15 in one tile; pieces of 255, 256 and 257 keys; an LDS piece that
    ends with its tile before a tile inside another segment; and neighbouring segments' histograms differ"""
    rng = np.random.default_rng(2)
    for B in (64, 4096):
        got = {}
        for name, layout in H.SLOT_LAYOUTS.items():
            n, off = layout()
            assert (n + H.TILE - 1) // H.TILE <= 3 and H.chunk_of(n) == 1
            got[name] = piece_slots(n, off, B)
            o = off.astype(np.int64)
            assert sum(p[2] for p in got[name]) == int(o[-1] - o[0])
            assert all((p[4] is not None) == (p[3] != "direct") for p in got[name] if name != "ends_with_tile")
            counts = np.stack([np.bincount(b[b < B], minlength=B) for b in np.split(H.shifted_bins(rng, n, off, B)[o[0]:o[-1]], np.cumsum(np.diff(o))[:-1])])
            assert np.all(np.any(counts[1:] != counts[:-1], axis=1)) and counts.sum() < int(o[-1] - o[0])       # neighbours differ; some keys are dropped
        slots = lambda name, tile: [p[4] for p in got[name] if p[0] == tile and p[4] is not None]
        assert slots("slots16", 0) == list(range(16))                                  # 15 flushes inside one tile
        assert {p[2] for p in got["slots16"]} == {256}
        sh = got["slots16_shifted"]
        assert sh[0][2:4] == (255, "direct") and slots("slots16_shifted", 0) == list(range(15))
        assert [p[1:4] for p in sh if p[1] == 16] == [(16, 1, "direct"), (16, 255, "direct")]           # the piece over the tile edge: both parts short
        assert slots("slots16_shifted", 1) == [0] and sh[-1][2] == 256
        cyc = got["lengths_cycle"]
        assert {p[2] for p in cyc} == {255, 256, 257} and all((p[3] == "direct") == (p[2] == 255) for p in cyc)
        assert slots("lengths_cycle", 0) == slots("lengths_cycle", 1) == [0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15]
        end = got["ends_with_tile"]
        assert [(p[0], p[1], p[4]) for p in end] == [(0, 0, 0), (0, 1, 11), (1, 2, None), (2, 2, 0), (2, 3, 3)]
        assert end[1][2] == H.TILE - 3000 and all(p[3] != "direct" for p in end)       # the LDS piece of slot 11 ends with tile 0
    # the layouts from before reach slots {0, 1, 4, 7, 8, 11, 12} only and no piece within one key of the direct boundary
    old = set()
    for name, (layout, B, _) in H.LAYOUTS.items():
        if name.startswith("big") or B > H.LDS_MAX:
            continue
        pieces = piece_slots(*layout(), B)
        old |= {p[4] for p in pieces if p[4] is not None}
        assert not any(255 <= p[2] <= 257 for p in pieces if name != "ragged_lds")
    assert 15 not in old


def test_boundary_bins_and_zero_fill_sizes():
    assert [H.lds_layout(B) for B in H.BOUNDARY_BINS] == ["wave_private", "wave_private", "shared", "shared"]
    assert 4 * 1024 == H.LDS_MAX                                                       # four copies of 1024 counters fill cnt[] exactly
    # the zero fill: totals below one 16-byte store at every alignment, and one total with a second trip of the grid-stride loop
    assert sorted(H.ZERO_SMALL) == [1, 2, 3, 4, 5, 7, 8, 9] and all(S * B == total for total, (S, B) in H.ZERO_SMALL.items())
    for total in H.ZERO_SMALL:
        for align in H.ZERO_ALIGN:
            head = min(total, ((16 - align) % 16) // 4)
            nvec = (total - head) // 4
            assert nvec <= 2 and total - head - 4 * nvec <= 3
    assert any(min(t, ((16 - a) % 16) // 4) == t for t in H.ZERO_SMALL for a in H.ZERO_ALIGN)             # head = total: nothing but the head
    assert any((t - min(t, ((16 - a) % 16) // 4)) // 4 == 0 and t > 3 for t in H.ZERO_SMALL for a in H.ZERO_ALIGN)      # nvec == 0 with a head and a tail
    n, off = H.zero_big_layout()
    f_n, f_off = H.fifties_layout()
    assert len(off) == len(f_off) + 1 and np.array_equal(off[:-1], f_off) and n == f_n + 50
    total = (len(off) - 1) * H.ZERO_BIG_BINS
    assert total == 4259905 and total % 2 == 1 and total / 4 > 256 * 16 * 256
    grid, nvec, trips = H.zero_grid(total)
    assert grid == 16 * 256 and trips == 2 and H.zero_grid(1 << 20)[2] == 1              # (2^20 counters, the most before: one trip)
    assert {p[3] for p in piece_paths(n, off, H.ZERO_BIG_BINS)} == {"direct"}


# -- no GPU: the call and the helpers raise, nothing is computed on the CPU ------------------------------------------------------------------------

def test_no_cpu_path(rsx):
    torch = pytest.importorskip("torch")
    x = torch.arange(10, dtype=torch.int64)
    f = torch.arange(10, dtype=torch.float32)
    for call in (lambda: rsx.bincount(x), lambda: rsx.bincount(x, num_bins=4), lambda: rsx.bincount_rows(x.reshape(2, 5), 4),
                 lambda: rsx.histc(f, bins=4, min=0, max=8), lambda: rsx.histogram(f, 4, range=(0.0, 8.0)),
                 lambda: rsx.histogram(f, torch.tensor([0.0, 4.0, 8.0])), lambda: rsx.histogram_rows(f.reshape(2, 5), 4, range=(0.0, 8.0)),
                 lambda: rsx.segmented_histogram(x, None, 4)):
        with pytest.raises(ValueError, match="device tensor"):
            call()
    for bad in (torch.zeros(4, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.float16), torch.zeros(4, dtype=torch.bool)):
        for call in (lambda: rsx.bincount(bad), lambda: rsx.histc(bad), lambda: rsx.histogram(bad, 4), lambda: rsx.segmented_histogram(bad, None, 4),
                     lambda: rsx.bincount_rows(bad.reshape(2, 2), 4), lambda: rsx.histogram_rows(bad.reshape(2, 2), 4)):
            with pytest.raises(TypeError):
                call()
    with pytest.raises(TypeError):
        rsx.histc(x)                                                # integers have no histc
    with pytest.raises(TypeError):
        rsx.bincount(f)
    if torch.cuda.is_available():
        return                                                      # the no-device path cannot be observed; the GPU suite runs the call
    with pytest.raises(rsx.RadixSortError) as ei:
        rsx.Engine(np.uint32, 4096)
    assert ei.value.status == 2                                     # INITIALIZATION_FAILED: no device, no silent CPU path
    null = C.c_void_p()
    assert rsx.load_library().rsx_segmented_histogram(null, None, 0, None, 1, None, 0, 0, 0, 4, 0, None) == 4       # null engine
    assert b"rsx_segmented_histogram" in rsx.load_library().rsx_last_error()
