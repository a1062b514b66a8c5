"""CPU tests of the weighted histogram (rsx_segmented_weighted_histogram; tests/test_gpu_whistogram.py holds the GPU ones): the header,
the binding and the exports agree; the mass of a weight as the kernel adds it, unsigned and signed — csrc/rsx_mass_math.hpp through the
stand-alone whist_selftest, plain and under -fsanitize=address,undefined — against the referee tests/_whistogram_ref.py; the referee's
vectorised and loop forms against each other; the piece paths of every layout the GPU tests run, at 256 CUs and with THIS kernel's
constants; and the refusals of the torch helpers on host tensors and on weight dtypes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _histogram_ref as H
import _whistogram_ref as W
import _wselect_ref
from _whistogram_ref import mass_loop, signed_mass_np, whistogram_loop, whistogram_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "radix-sort_amd", "host", "bin")
SELFTESTS = {"plain": os.path.join(BIN, "whist_selftest"), "sanitized": os.path.join(BIN, "whist_selftest_san")}


def test_header_binding_and_exports_agree(rsx):
    header = open(os.path.join(ROOT, "include", "radixsort_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"int\s+rsx_segmented_weighted_histogram\s*\(([^;]*)\)\s*;", text)
    assert m, "rsx_segmented_weighted_histogram is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "const void* d_weights", "uint64_t n", "const uint64_t* d_offsets", "uint64_t num_segments",
                      "const void* d_edges", "uint64_t lo_bits", "uint64_t hi_bits", "uint32_t width_shift", "uint64_t num_bins", "uint32_t flags",
                      "uint32_t weight_kind", "int32_t weight_exp", "uint64_t* d_sums_out"]
    d = re.search(r"#define\s+RSX_WHIST_SIGNED\s+(\d+)", header)
    assert d and int(d.group(1)) == rsx.WHIST_SIGNED == W.WHIST_SIGNED == 256 and rsx.WSELECT_FRACTION == 128        # bit 8; bits 0-7 are taken
    assert "rsx_segmented_weighted_histogram" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_weighted_histogram
    P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert fn.argtypes == [P, P, P, U64, P, U64, P, U64, U64, U32, U64, U32, U32, C.c_int32, P]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_weighted_histogram\b", out)
    assert callable(rsx.segmented_weighted_histogram) and callable(rsx.Engine.segmented_weighted_histogram)


def test_kernel_constants_match_the_referee():
    src = open(os.path.join(ROOT, "radix-sort_amd", "csrc", "rsx_wbins.hpp")).read()
    for name, value in (("kWbinsLdsMax", W.LDS_MAX), ("kWbinsWavePrivateMax", W.WAVE_PRIVATE_MAX)):
        m = re.search(r"constexpr uint32_t " + name + r" = (\d+);", src)
        assert m and int(m.group(1)) == value, name
    assert "kWbinsEdgesMax = kBinsLdsMax" in src and W.EDGES_MAX == H.LDS_MAX and W.DIRECT_PIECE == H.DIRECT_PIECE
    assert W.LDS_MAX * 8 == H.LDS_MAX * 4                        # the same 16 KiB of counters


# -- the mass as the kernel adds it ---------------------------------------------------------------------------------------------------------------

def _bits(values, dtype):
    return np.asarray(values, dtype=dtype).view(np.uint32 if dtype == np.float32 else np.uint64)


def _mass_cases():
    """(kind, weight_exp, signed, bits): every exponent case of _wselect_ref.exponent_cases() with both signs of every weight, +-0, +-inf,
    NaNs of both signs and subnormals at a spread of exponents, the uint32 words"""
    cases = []
    for dtype, wexp, off, w in _wselect_ref.exponent_cases():
        kind = W.kind_of(w)
        picked = w[:: max(w.size // 400, 1)]
        both = np.concatenate([picked, -picked])
        cases += [(kind, wexp, s, int(b)) for s in (0, 1) for b in _bits(both, dtype)]
    for dtype, kind in ((np.float32, 1), (np.float64, 2)):
        f = np.finfo(dtype)
        vals = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, f.smallest_subnormal, -f.smallest_subnormal, f.tiny - f.smallest_subnormal,
                -(f.tiny - f.smallest_subnormal), f.smallest_subnormal * 3, f.tiny, -f.tiny, 1.0, -1.0, 0.75, -0.75, 2.0 ** -31, -(2.0 ** -31), 2.0 ** -32,
                -(2.0 ** -32), f.max, -f.max, 1 / 3, -1 / 3]
        nan_payloads = [0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF] if dtype == np.float32 else \
            [0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF]
        bits = [int(b) for b in _bits(vals, dtype)] + nan_payloads
        for wexp in list(range(-3, 4)) + [-2048, -1074, -1022, -149, -126, 127, 1023, 2048]:
            cases += [(kind, wexp, s, b) for s in (0, 1) for b in bits]
    cases += [(0, 0, 0, v) for v in (0, 1, 1 << 31, (1 << 32) - 1)]
    return cases


def _want(kind, wexp, signed, b):
    if kind == 0:
        return b
    w = np.array([b], dtype=np.uint32 if kind == 1 else np.uint64).view(np.float32 if kind == 1 else np.float64)
    return int(signed_mass_np(w, wexp, bool(signed))[0])


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_selftest_masses(tmp_path, which):
    exe = SELFTESTS[which]
    assert os.path.exists(exe), "run __graft_entry__.build()"
    cases = _mass_cases()
    assert len(cases) > 10000
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{k} {e} {s} {b}\n" for k, e, s, b in cases))
    proc = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, (proc.returncode, proc.stderr[-2000:])                 # 2: the header differs from its own ldexp form
    lines = proc.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    seen = set()
    for (kind, wexp, signed, b), line in zip(cases, lines):
        want = _want(kind, wexp, signed, b)
        assert line == str(want), (kind, wexp, signed, hex(b), line, want)
        seen.add((signed, (want > 0) - (want < 0), abs(want) == 1 << 31))
    # positive, negative and zero masses, saturated and not, occur; no unsigned mass is negative
    assert {(1, -1, True), (1, -1, False), (1, 1, True), (1, 0, False), (0, 1, True), (0, 1, False), (0, 0, False)} <= seen
    assert not any(s == 0 and sign < 0 for s, sign, _ in seen)


def test_selftest_refuses_bad_cases(tmp_path):
    for text in ("3 0 0 1\n", "1 0 0 4294967296\n", "0 0 1 5\n", "0 1 0 5\n", "1 0 2 5\n", "1 2049 0 5\n", "1 0 0\n", "x\n"):
        path = tmp_path / "bad.txt"
        path.write_text(text)
        assert subprocess.run([SELFTESTS["plain"], str(path)], capture_output=True).returncode == 1, text


def test_signed_mass_by_hand():
    w = np.array([np.nan, -np.nan, 0.0, -0.0, -1.0, 1.0, -2.0, np.inf, -np.inf, 0.5, -0.5, -(2.0 ** -31), 2.0 ** -32], dtype=np.float32)
    assert signed_mass_np(w, 0, True).tolist() == [0, 0, 0, 0, -(1 << 31), 1 << 31, -(1 << 31), 1 << 31, -(1 << 31), 1 << 30, -(1 << 30), -1, 0]
    assert signed_mass_np(w, 0, False).tolist() == [0, 0, 0, 0, 0, 1 << 31, 0, 1 << 31, 0, 1 << 30, 0, 0, 0]
    assert signed_mass_np(w, 1, True).tolist() == [0, 0, 0, 0, -(1 << 30), 1 << 30, -(1 << 31), 1 << 31, -(1 << 31), 1 << 29, -(1 << 29), 0, 0]
    assert signed_mass_np(np.array([3, 0, 0xFFFFFFFF], dtype=np.uint32), 0, True).tolist() == [3, 0, 0xFFFFFFFF]
    for dt in (np.float32, np.float64):
        for wexp in (-5, 0, 3):
            x = W.case_weights(np.random.default_rng(3), dt, 500, None, wexp)
            for signed in (False, True):
                assert mass_loop(x, wexp, signed) == signed_mass_np(x, wexp, signed).tolist()


# -- the referee's two forms ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["even", "edges"])
@pytest.mark.parametrize("dt", ["int32", "uint64", "float32"])
def test_referee_forms_agree_on_the_ragged_layout(dt, form):
    n, off = H.ragged_layout()
    for descending in (False, True):
        for wi, wdt in enumerate(W.WEIGHT_DTYPES):
            B = W.MATRIX_BINS[(wi + descending) % 3]                                    # 1, 64, 513: the loop form walks the edges linearly
            rng = np.random.default_rng(2000 + H.DTYPES.index(dt) * 100 + B + wi)
            args = W.form_args(dt, form, descending, B, rng)
            keys = H.case_keys(rng, dt, n, off, args)
            wexp = 0 if wdt == np.uint32 else (-3, 5)[wi - 1]
            w = W.case_weights(rng, wdt, n, off, wexp)
            for signed in ((False,) if wdt == np.uint32 else (False, True)):
                a = whistogram_oracle(keys, w, off, descending=descending, weight_exp=wexp, signed=signed, **args)
                b = whistogram_loop(keys, w, off, descending=descending, weight_exp=wexp, signed=signed, **args)
                assert a.shape == (len(off) - 1, B) and np.array_equal(a, b)
                assert np.any(a != 0) and (not signed or np.any(a < 0))
            # with weights of one unit the sums are the counts
            ones = np.ones(n, dtype=np.uint32)
            assert np.array_equal(whistogram_oracle(keys, ones, off, descending=descending, **args), H.histogram_oracle(keys, off, descending=descending, **args))


def test_case_weights_hold_what_the_matrix_needs():
    n, off = H.ragged_layout()
    o = off.astype(np.int64)
    for wdt in (np.float32, np.float64):
        for wexp in (-3, 0, 5):
            w = W.case_weights(np.random.default_rng(1), wdt, n, off, wexp)[o[0]:o[-1]]
            assert np.any(w < 0) and np.any((w == 0) & np.signbit(w)) and np.any((w == 0) & ~np.signbit(w))
            assert np.any(np.isnan(w) & np.signbit(w)) and np.any(np.isnan(w) & ~np.signbit(w)) and np.any(w == np.inf) and np.any(w == -np.inf)
            assert np.any(np.isfinite(w) & (w >= np.ldexp(1.0, wexp)))                  # one weight at or above 2^weight_exp
    d = W.dyadic_weights(np.random.default_rng(2), 1000)
    assert np.array_equal(signed_mass_np(d, 0, True), (d.astype(np.float64) * (1 << 31)).astype(np.int64)) and d.min() >= -1 and d.max() <= 1


# -- the paths: every layout of the GPU tests reaches the path it is named for, at 256 CUs ----------------------------------------------------------

@pytest.mark.parametrize("name", sorted(W.LAYOUTS))
def test_layouts_reach_their_paths(name):
    layout, B, want = W.LAYOUTS[name]
    n, off = layout()
    paths = W.piece_paths(n, off, B)
    assert {p[3] for p in paths} == want, name
    assert sum(p[2] for p in paths) == int(H._offsets(n, off)[-1] - H._offsets(n, off)[0])


def test_paths_by_bin_count():
    assert [W.lds_layout(B) for B in W.PATH_BINS + [4096, 50257]] == ["wave_private", "shared", "shared", "none", "none", "none"]
    assert [W.lds_layout(B) for B in (256, 2048)] == ["wave_private", "shared"]          # the two skew sizes
    # what the unweighted kernel counts in LDS, this one adds directly from 2049 bins on
    n, off = H.ragged_layout()
    assert {p[3] for p in H.piece_paths(n, off, 4096)} > {"direct"} and {p[3] for p in W.piece_paths(n, off, 4096)} == {"direct"}
    assert [p[:3] for p in W.piece_paths(n, off, 64)] == [p[:3] for p in H.piece_paths(n, off, 64)]


def test_slot_layouts_fill_their_slots():
    for name, layout in H.SLOT_LAYOUTS.items():
        n, off = layout()
        assert W.piece_slots(n, off, 16) == H.piece_slots(n, off, 16), name             # below both kernels' bounds the walk is the same
    slots = [p[4] for p in W.piece_slots(*H.slots16_layout(), 16)]
    assert slots == list(range(16))
    paths = {p[3] for p in W.piece_paths(*H.big_boundaries_layout(), 256)}
    assert paths == {"lds_first", "lds_same", "lds_flush", "direct"}


@pytest.mark.parametrize("cus", [256, 128, 304])
def test_two_tile_layout_reaches_carry_and_flush_with_shared_counters(cus):
    """the layout of tests/test_gpu_whistogram_paths.py: two tiles per workgroup at any CU count, every LDS path with one shared counter
    copy (513 and 2048 bins) and with the last wave-private size, and nothing but direct adds from 2049 bins on"""
    n, off = W.big_boundaries_layout(cus)
    assert n == (16 * cus + 1) * H.TILE + 5 and H.chunk_of(n, cus) == 2 and H.chunk_of(16 * cus * H.TILE, cus) == 1
    assert (n, off.tolist()) == (H.big_boundaries_layout()[0], H.big_boundaries_layout()[1].tolist()) or cus != 256
    for B, layout in ((512, "wave_private"), (513, "shared"), (2048, "shared")):
        paths = W.piece_paths(n, off, B, cus)
        assert W.lds_layout(B) == layout and {p[3] for p in paths} == {"lds_first", "lds_same", "lds_flush", "direct"}
        by_tile = {}
        for t, s, length, path in paths:
            by_tile.setdefault(t, []).append((s, path))
        assert by_tile[2] == [(0, "lds_first")] and by_tile[3] == [(0, "lds_same"), (1, "lds_flush")]         # carried into a second tile, flushed inside it
        assert by_tile[8] == [(1, "lds_first"), (2, "lds_flush")] and by_tile[9] == [(2, "lds_same")]         # flushed in a first tile, carried on
        assert by_tile[13] == [(2, "lds_same"), (3, "direct")]
    assert {p[3] for p in W.piece_paths(n, off, 2049, cus)} == {"direct"}


def test_first_suite_has_one_two_tile_case():
    """the gap that tests/test_gpu_whistogram_paths.py closes: test_carry_over_and_flush is the only case of tests/test_gpu_whistogram.py
    whose workgroups walk two tiles, and it has wave-private counters"""
    two_tile = [name for name, (layout, B, _) in W.LAYOUTS.items() if H.chunk_of(layout()[0]) > 1]
    assert two_tile == ["big_boundaries"] and W.LAYOUTS["big_boundaries"][1] == 256 and W.lds_layout(256) == "wave_private"
    assert H.chunk_of(H.SKEW_N) == 1 and H.chunk_of(1 << 16) == 1 and all(H.chunk_of(f()[0]) == 1 for f in H.SLOT_LAYOUTS.values())
    text = open(os.path.join(ROOT, "tests", "test_gpu_whistogram.py")).read()
    assert text.count("big_boundaries_layout") == 1 and text.count("BIG_N") == 0


# -- the torch helpers refuse host tensors and foreign weight dtypes ---------------------------------------------------------------------------------

def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    assert lib.rsx_segmented_weighted_histogram(None, None, None, 0, None, 1, None, 0, 0, 0, 1, 0, 1, 0, None) == 4     # a null engine
    assert lib.rsx_last_error() == b"rsx_segmented_weighted_histogram: null engine"
    torch = pytest.importorskip("torch")
    x = torch.randint(0, 8, (10,), dtype=torch.int64)
    f = torch.rand(10)
    w = torch.rand(10)
    off = torch.tensor([0, 4, 10], dtype=torch.int64)
    edges = torch.linspace(0, 1, 5)
    for call in (lambda: rsx.segmented_weighted_histogram(x, off, w, 8), lambda: rsx.segmented_weighted_histogram(f, None, w, edges),
                 lambda: rsx.segmented_weighted_histogram(x, off, w.double(), 8, weight_max=1.0, signed=False, return_mass=True),
                 lambda: rsx.segmented_weighted_histogram(x, off, torch.ones(10, dtype=torch.int32), 8),
                 lambda: rsx.bincount(x, weights=w), lambda: rsx.bincount(x, num_bins=8, weights=w, weight_max=1.0),
                 lambda: rsx.bincount_rows(x.reshape(2, 5), 8, weights=w.reshape(2, 5)),
                 lambda: rsx.histogram(f, edges, weight=w), lambda: rsx.histogram(f, 4, range=(0.0, 1.0), weight=w, weight_max=1.0),
                 lambda: rsx.histogram_rows(f.reshape(2, 5), edges, weight=w.reshape(2, 5))):
        with pytest.raises(ValueError):                            # host tensors: no CPU fallback
            call()


def test_weight_dtype_refusals(rsx):
    torch = pytest.importorskip("torch")
    x = torch.randint(0, 8, (10,), dtype=torch.int64)
    f = torch.rand(10)
    off = torch.tensor([0, 4, 10], dtype=torch.int64)
    edges = torch.linspace(0, 1, 5)
    for bad in (torch.ones(10, dtype=torch.float16), torch.ones(10, dtype=torch.bfloat16), torch.ones(10, dtype=torch.int64), torch.ones(10, dtype=torch.bool)):
        for call in (lambda: rsx.segmented_weighted_histogram(x, off, bad, 8), lambda: rsx.bincount(x, weights=bad),
                     lambda: rsx.bincount_rows(x.reshape(2, 5), 8, weights=bad.reshape(2, 5)), lambda: rsx.histogram(f, edges, weight=bad),
                     lambda: rsx.histogram_rows(f.reshape(2, 5), edges, weight=bad.reshape(2, 5))):
            with pytest.raises(TypeError, match=r"unsupported weight type .* \(float32, float64, or int32 / uint32 masses\)"):
                call()
    for call in (lambda: rsx.bincount(x, weights=[1.0] * 10), lambda: rsx.histogram(f, edges, weight=np.ones(10, dtype=np.float32))):
        with pytest.raises(TypeError, match="the weights must be a tensor"):
            call()
    # the key type still comes first where it did, and without weights nothing has changed
    with pytest.raises(TypeError, match="integer tensor"):
        rsx.bincount(f)
    with pytest.raises(TypeError, match="integer tensor"):
        rsx.bincount(f, weights=f)
    with pytest.raises(ValueError, match="device tensor"):
        rsx.bincount(x)
