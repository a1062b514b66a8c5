"""CPU checks of the weighted select (rsx_segmented_weighted_select): header, binding and exports agree; the referee of the GPU tests
(tests/_wselect_ref.py) against brute force with Python integers and against the two chains the call replaces; the mass function and
the target rule of csrc/rsx_mass_math.hpp — what the kernels call — through the stand-alone wselect_selftest, plain and under
-fsanitize=address,undefined, against the numpy form; the torch wrappers' refusals on host tensors; and the launch geometry at 256 CUs of
the layouts that tests/test_gpu_wselect_paths.py runs: each one still reaches the path it is there for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _segmented_ref as S
import _wselect_ref as W
from _wselect_ref import MASS_ONE, brute_force, mass_np, target_of, wselect_oracle
from test_gpu_float_keys import special

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "radix-sort_amd", "host", "bin")
SELFTESTS = {"plain": os.path.join(BIN, "wselect_selftest"), "sanitized": os.path.join(BIN, "wselect_selftest_san")}
HELPERS = ("segmented_weighted_select", "top_p", "weighted_quantile", "weighted_median")


def test_header_binding_and_exports_agree(rsx):
    header = open(os.path.join(ROOT, "include", "radixsort_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"int\s+rsx_segmented_weighted_select\s*\(([^;]*)\)\s*;", text)
    assert m, "rsx_segmented_weighted_select is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "const void* d_weights", "uint64_t n", "const uint64_t* d_offsets",
                      "uint64_t num_segments", "const void* d_targets", "uint32_t targets_per_segment", "uint32_t flags", "uint32_t weight_kind",
                      "int32_t weight_exp", "void* d_keys_out", "uint32_t* d_index_out", "uint32_t* d_rank_out", "uint64_t* d_mass_out",
                      "uint64_t* d_total_out"]
    for name, value in (("RSX_WEIGHT_UINT32", rsx.WEIGHT_UINT32), ("RSX_WEIGHT_FLOAT32", rsx.WEIGHT_FLOAT32), ("RSX_WEIGHT_FLOAT64", rsx.WEIGHT_FLOAT64),
                        ("RSX_WSELECT_FRACTION", rsx.WSELECT_FRACTION)):
        d = re.search(r"#define\s+" + name + r"\s+(\d+)", header)
        assert d and int(d.group(1)) == value, name
    assert rsx.WSELECT_FRACTION == 128 and rsx.EXPAND_GATHER == 64           # bit 7; bits 0-6 are taken
    assert "rsx_segmented_weighted_select" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_weighted_select
    P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert fn.argtypes == [P, P, P, U64, P, U64, P, U32, U32, U32, C.c_int32, P, P, P, P, P]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_weighted_select\b", out)
    for name in HELPERS:
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_weighted_select)
    import radix_sort_amd._tensor_args as args
    assert args.WEIGHT_KINDS == {"uint32": 0, "int32": 0, "float32": 1, "float64": 2}


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    assert lib.rsx_segmented_weighted_select(None, None, None, 0, None, 1, None, 1, 0, 1, 0, None, None, None, None, None) == 4     # a null engine
    assert lib.rsx_last_error() == b"rsx_segmented_weighted_select: null engine"
    torch = pytest.importorskip("torch")
    x = torch.rand(10)
    w = torch.rand(10)
    off = torch.tensor([0, 4, 10], dtype=torch.int64)
    fr = torch.tensor([0.5, 0.9], dtype=torch.float64)
    for call in (lambda: rsx.segmented_weighted_select(x, off, w, fractions=fr), lambda: rsx.segmented_weighted_select(x, off, fractions=fr),
                 lambda: rsx.top_p(x, 0.9), lambda: rsx.top_p(x.reshape(2, 5), torch.tensor([0.5, 0.9])),
                 lambda: rsx.weighted_quantile(x, w, 0.5), lambda: rsx.weighted_quantile(x, w, [0.1, 0.9], weight_max=1.0),
                 lambda: rsx.weighted_median(x, w), lambda: rsx.weighted_median(x, torch.ones(10, dtype=torch.int32)),
                 lambda: rsx.top_p(x.to(torch.bfloat16), 0.9)):
        with pytest.raises(ValueError):                            # host tensors: no CPU fallback
            call()


# -- the referee ---------------------------------------------------------------------------------------------------------------------------

def test_referee_against_brute_force():
    rng = np.random.default_rng(1)
    for trial in range(120):
        L = int(rng.integers(1, 40))
        dtype = [np.int32, np.uint64, np.float32, np.float64][trial % 4]
        x = rng.integers(0, 4, L).astype(dtype) if trial % 3 else special(dtype, L, rng) if np.dtype(dtype).kind == "f" else rng.integers(0, 99, L).astype(dtype)
        kind = trial % 3
        wexp = int(rng.integers(-3, 4)) if kind else 0
        if kind == 0:
            w = rng.integers(0, 5, L).astype(np.uint32)
            w[rng.integers(0, L)] = 0xFFFFFFFF
        else:
            w = (rng.random(L) * 3 - 0.5).astype(np.float32 if kind == 1 else np.float64)
            w[rng.integers(0, L)] = np.nan
        desc = bool(trial & 8)
        total = int(mass_np(w, wexp).sum())
        for T in {0, 1, total // 2, max(total - 1, 0), total, total + 1, int(rng.integers(0, total + 2))}:
            k, p, r, m, written, tot, valid = wselect_oracle(x, [0, L], w, [T], False, desc, wexp)
            bp, br, bm, btot = brute_force(x, w, T, desc, wexp)
            assert valid[0] and int(tot[0]) == btot == total
            if bp is None or T > total:
                assert not written[0, 0], (trial, T)
            else:
                assert written[0, 0] and (int(p[0, 0]), int(r[0, 0]), int(m[0, 0])) == (bp, br, bm), (trial, T)
                assert int(mass_np(w, wexp)[bp]) > 0                                   # the answer has mass
                assert k[0, 0] == x.view(k.dtype)[bp]


def test_fraction_targets():
    assert target_of(0, 0.5, True) == 0 and target_of(10, float("nan"), True) == 0
    assert target_of(10, 0.0, True) == 1 and target_of(10, -3.0, True) == 1 and target_of(10, float("-inf"), True) == 1
    assert target_of(10, 1.0, True) == 10 and target_of(10, 7.5, True) == 10 and target_of(10, float("inf"), True) == 10
    assert target_of(10, 0.5, True) == 5 and target_of(10, 0.51, True) == 6 and target_of(3, 1 / 3, True) == 1
    big = (1 << 62) + 12345                                                            # (double)total rounds: the clamp holds
    assert target_of(big, 1.0, True) == big and 1 <= target_of(big, 0.999999999, True) <= big
    assert target_of(10, 0, False) == 0 and target_of(10, 11, False) == 0 and target_of(10, 10, False) == 10


def test_top_p_equals_sort_cumsum_lower_bound_on_dyadic_rows():
    """Keys as weights, descending, fraction p: the same element as "stable descending sort, float64 cumsum, lower bound of p" on dyadic
    probabilities (multiples of 2^-24 summing to 1, p a multiple of 1/1024).  300 of 300 rows, none excluded."""
    rng = np.random.default_rng(2)
    for row in range(300):
        L = int(rng.integers(1, 400))
        cuts = np.sort(rng.integers(0, (1 << 24) + 1, L - 1))
        parts = np.diff(np.concatenate([[0], cuts, [1 << 24]]))                        # L non-negative integers summing to 2^24
        dtype = np.float32 if row % 2 else np.float64
        probs = (parts / float(1 << 24)).astype(dtype)
        assert float(probs.astype(np.float64).sum()) == 1.0
        p = int(rng.integers(1, 1025)) / 1024.0
        k, pos, r, m, written, tot, _ = wselect_oracle(probs, [0, L], None, np.array([p]), True, True, 0)
        assert int(tot[0]) == MASS_ONE and written[0, 0]
        order = np.argsort(-probs.astype(np.float64), kind="stable")
        cdf = np.cumsum(probs[order].astype(np.float64))
        want = int(np.searchsorted(cdf, p, side="left"))
        assert int(r[0, 0]) == want and int(pos[0, 0]) == int(order[want]), row
        assert float(int(m[0, 0])) / MASS_ONE == cdf[want]


def test_integer_weights_equal_a_plain_select_of_the_repeated_keys():
    """Integer weights: the element a plain select names at rank T - 1 of np.repeat(x, w).  200 of 200, none excluded."""
    rng = np.random.default_rng(3)
    for trial in range(200):
        L = int(rng.integers(1, 200))
        x = rng.integers(-20, 20, L).astype(np.int64 if trial % 2 else np.int32)
        w = rng.integers(0, 6, L).astype(np.uint32)
        total = int(w.sum())
        desc = bool(trial & 4)
        if total == 0:
            _, _, _, _, written, tot, _ = wselect_oracle(x, [0, L], w, [1], False, desc)
            assert not written[0, 0] and int(tot[0]) == 0
            continue
        T = int(rng.integers(1, total + 1))
        k, pos, r, m, written, tot, _ = wselect_oracle(x, [0, L], w, [T], False, desc)
        rep = np.repeat(x, w)
        src = np.repeat(np.arange(L), w)
        order = np.argsort(-rep if desc else rep, kind="stable")
        assert written[0, 0] and int(pos[0, 0]) == int(src[order[T - 1]]) and k[0, 0] == rep[order[T - 1:T]].view(k.dtype)[0], trial


# -- the mass function and the target rule the kernels call -----------------------------------------------------------------------------------

def _bits(values, dtype):
    u = np.uint32 if dtype == np.float32 else np.uint64
    return np.asarray(values, dtype=dtype).view(u)


def _mass_cases():
    """(kind, weight_exp, bits) over the specials and every weight_exp in -40 .. 40."""
    cases = []
    for dtype, kind in ((np.float32, 1), (np.float64, 2)):
        f = np.finfo(dtype)
        one = dtype(1.0)
        vals = [np.nan, -np.nan, 0.0, -0.0, -1.0, -f.tiny, f.smallest_subnormal, f.smallest_subnormal * 3, f.tiny, f.tiny / 2, 2.0 ** -31, 2.0 ** -32,
                2.0 ** -33, 1.0, np.nextafter(one, dtype(0)), np.nextafter(one, dtype(2)), 2.0, 0.75, 1 / 3, 1e-7, 12345.678, f.max, np.inf, -np.inf,
                2.0 ** 31, 2.0 ** 40 * 1.5, 2.0 ** -40 * 1.75]
        bits = list(_bits(vals, dtype)) + list(_bits(np.random.default_rng(5).random(40) * 2, dtype))
        for wexp in range(-40, 41):
            cases += [(kind, wexp, int(b)) for b in bits]
        for wexp in (-149, -126, -1074, -1022, 127, 1023, 2048, -2048):                   # the ends of both exponent ranges
            cases += [(kind, wexp, int(b)) for b in bits]
    cases += [(0, 0, v) for v in (0, 1, 7, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)]
    return cases


def _target_cases():
    cases = [(0, tot, t) for tot in (0, 1, 10, (1 << 63) - 1) for t in (0, 1, 5, 10, 11, (1 << 63) - 1, 1 << 63, (1 << 64) - 1)]
    fr = [0.0, -0.0, 1.0, 0.5, 1 / 3, 0.999999999, 1e-300, -1.0, 2.0, np.inf, -np.inf, np.nan, np.nextafter(1.0, 0.0), 1 / 1024, 0.9]
    for tot in (0, 1, 2, 3, 10, 1 << 31, (1 << 31) * 50257, (1 << 53) + 1, (1 << 62) + 12345, (1 << 63) - 1):
        cases += [(1, tot, int(b)) for b in _bits(fr, np.float64)]
    return cases


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_selftest_mass_and_targets(tmp_path, which):
    exe = SELFTESTS[which]
    assert os.path.exists(exe), "run __graft_entry__.build()"
    masses, targets = _mass_cases(), _target_cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"m {k} {e} {b}\n" for k, e, b in masses) + "".join(f"t {f} {tot} {b}\n" for f, tot, b in targets))
    proc = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, (proc.returncode, proc.stderr[-2000:])                 # 2: the header differs from its own ldexp form
    lines = proc.stdout.split("\n")[:-1]
    assert len(lines) == len(masses) + len(targets)
    for (kind, wexp, b), line in zip(masses, lines):
        if kind == 0:
            want = b
        else:
            w = np.array([b], dtype=np.uint32 if kind == 1 else np.uint64).view(np.float32 if kind == 1 else np.float64)
            want = int(mass_np(w, wexp)[0])
        assert line == f"m {want}", (kind, wexp, hex(b), line)
    for (f, tot, b), line in zip(targets, lines[len(masses):]):
        t = b if not f else float(np.array([b], dtype=np.uint64).view(np.float64)[0])
        assert line == f"t {target_of(tot, t, bool(f))}", (f, tot, hex(b), line)


def test_mass_np_by_hand():
    w = np.array([np.nan, 0.0, -0.0, -1.0, 1.0, 2.0, np.inf, 0.5, 2.0 ** -31, 2.0 ** -32, np.nextafter(np.float32(1), np.float32(0))], dtype=np.float32)
    assert mass_np(w).tolist() == [0, 0, 0, 0, 1 << 31, 1 << 31, 1 << 31, 1 << 30, 1, 0, (1 << 31) - 128]
    assert mass_np(w, 1).tolist() == [0, 0, 0, 0, 1 << 30, 1 << 31, 1 << 31, 1 << 29, 0, 0, (1 << 30) - 64]
    assert mass_np(np.array([3, 0, 0xFFFFFFFF], dtype=np.uint32)).tolist() == [3, 0, 0xFFFFFFFF]


def test_selftest_refuses_bad_cases(tmp_path):
    for text in ("m 3 0 1\n", "m 1 0 4294967296\n", "x 1 2 3\n", "t 2 1 1\n", "m 1 0\n"):
        path = tmp_path / "bad.txt"
        path.write_text(text)
        assert subprocess.run([SELFTESTS["plain"], str(path)], capture_output=True).returncode == 1, text


# -- the layouts of tests/test_gpu_wselect_paths.py reach their paths at 256 CUs ----------------------------------------------------------------

def test_geometry_hand_made_case():
    """Four segments from 3, three of them large; every figure below is worked out by hand from the offsets."""
    off = S.offsets_from([5000, 9000, 300, 4097], start=3)              # 3, 5003, 14003, 14303, 18400
    n = int(off[-1]) + 5                                                # 18405
    # seg_shape: max_large = min(4, 18405 / 4097) = 4, max_tiles = ceil(18405 / 4096) + 4 = 9.  Tiles on the 4096-key grid: [3, 5003) 2,
    # [5003, 14003) grid tiles 1..3: 3, [14303, 18400) grid tiles 3..4: 2; tstart = 0, 2, 5, 7
    g = W.wselect_geometry(off, n, 3, cus=1)                            # 8 groups wanted: gtiles = ceil(9 / 8) = 2
    assert (g["gtiles"], g["groups"], g["switches"]) == (2, 5, 1)       # tstart 5 is odd: segment 3 begins inside group 2
    assert (g["nlarge"], g["items"], g["pick_grid"]) == (3, 9, 2) and (g["tiles"], g["tie_grid"], g["max_segment_tiles"]) == (7, 8, 3)
    assert g["count"] == [0, 1, 0] and g["sort_grid"] == [4, 4, 4] and g["trips"] == [0, 1, 0]
    g = W.wselect_geometry(off, n, 4)
    assert (g["gtiles"], g["groups"], g["switches"], g["items"], g["pick_grid"], g["tie_grid"]) == (1, 9, 0, 12, 16, 9)
    assert W.answer_tiles(off, 1, [0, 3188, 3189, 8999]) == [0, 0, 1, 2]      # 5003 = 4096 + 907: 3189 keys in its first tile
    assert W.answer_tiles(off, 0, [4092, 4093]) == [0, 1]
    assert "gtiles=1" in W.summary(g) and "items=12/16" in W.summary(g)


def test_the_first_suite_stays_on_one_group_and_one_trip():
    """The state the path tests were written against: the LENGTHS layout of tests/test_gpu_wselect.py runs one tile per group, no
    workgroup of any kernel takes a second item, and no segment has more than one chunk of tiles.  If the sizing formulas of
    capi_wselect.inc change, this and the layout tests below fail first."""
    from test_gpu_wselect import LENGTHS
    off = S.offsets_from(LENGTHS, start=3)
    g = W.wselect_geometry(off, int(off[-1]) + 5, 4)
    print(W.summary(g))
    assert g["gtiles"] == 1 and g["switches"] == 0 and max(g["trips"]) <= 1
    assert g["items"] <= g["pick_grid"] and g["tiles"] <= g["tie_grid"] and g["max_segment_tiles"] <= W.FIND_CHUNK


def test_layout_many_large_shares_groups_and_strides():
    """many_large: gtiles >= 2 with at least `cus` large segments beginning inside a group; at R = 4 more than twice as many items as
    workgroups on the pick grid; more tiles than workgroups on the tie grid; at every R at least a second item per workgroup"""
    n, off = W.many_large()
    lens = np.diff(off.astype(np.int64))
    assert int(off[0]) == 3 and n == int(off[-1]) + 5 and np.count_nonzero(lens > W.TILE) == 4 * W.CUS and lens.max() <= 8000
    assert set(lens[lens <= W.TILE].tolist()) == set(W.MANY_SMALL) and n < 6500000
    g = W.wselect_geometry(off, n, 4)
    print(W.summary(g))
    assert g["gtiles"] >= 2 and g["switches"] >= W.CUS and g["items"] > 2 * g["pick_grid"] and g["tiles"] > g["tie_grid"]
    for R in (1, 2, 3):
        g = W.wselect_geometry(off, n, R)
        assert g["gtiles"] >= 2 and g["items"] >= 2 * g["pick_grid"]


@pytest.mark.parametrize("cus", [256, 304, 64])
@pytest.mark.parametrize("cls", [0, 1, 2])
def test_layout_stride_reaches_the_second_item_of_every_class(cls, cus):
    """stride_layout: trips[cls] >= 2 for the selects' LDS sorts too, and every second item is the shorter one; the layouts of classes 1
    and 2 are those the segmented sort's tests have always run"""
    n, off = S.stride_layout(cls, cus)
    g = W.wselect_geometry(off, n, 4, cus)
    print(W.summary(g))
    assert g["trips"][cls] >= 2 and g["count"][cls] > g["sort_grid"][cls] == cus * S.PER_CU[cls] and W.second_items_are_shorter(g, off, cls)
    assert g["nlarge"] == 0 and sum(g["count"]) == g["count"][cls] == len(off) - 1
    lens = np.diff(off.astype(np.int64))
    assert lens.min() >= S.MIN_LEN[cls] and lens.max() <= (S.CLASS0_MAX, S.CLASS1_MAX, S.TILE)[cls]
    if cus == 256 and cls:
        assert (n, int(off.sum())) == {1: (2900122, 6722358991), 2: (3129694, 2032199116)}[cls]


def test_layout_long_segment_has_a_second_chunk():
    n, off = W.long_segment()
    g = W.wselect_geometry(off, n, 4)
    print(W.summary(g))
    assert g["max_segment_tiles"] == 1031 > W.FIND_CHUNK and g["nlarge"] == 3 and int(off[0]) == 3
    assert W.long_targets(1030) == [1025, 515, 1025, 1]


def test_exponent_cases_reach_both_ends_of_the_mass_function():
    """exponent_cases: at least ten of the sixteen have an answer, a segment weighs nothing in one, every positive weight is saturated in
    another, and between the ends the masses take every size"""
    answered = zero_total = all_saturated = 0
    bits = set()
    for dtype, wexp, off, w in W.exponent_cases():
        assert w.dtype == dtype and np.isnan(w).any() and np.isinf(w).any() and (w < 0).any() and not np.isposinf(w[:int(off[1])]).any()
        tiny = np.finfo(dtype).tiny
        assert ((w > 0) & (w < tiny)).any()                                             # denormals
        m = mass_np(w, wexp)
        totals = [int(m[int(a):int(b)].sum()) for a, b in zip(off[:-1], off[1:])]
        answered += any(totals)
        zero_total += 0 in totals
        all_saturated += bool((m[w > 0] == MASS_ONE).all())
        bits |= {int(v).bit_length() for v in m[(m > 0) & (m < MASS_ONE)]}
    assert answered >= 10 and zero_total >= 1 and all_saturated >= 1
    assert bits == set(range(1, 32))
