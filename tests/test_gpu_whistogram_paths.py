"""rsx_segmented_weighted_histogram on the launch paths of rsx_wbins.hpp that tests/test_gpu_whistogram.py never reaches:

  A  workgroups of wbins_tile_kernel that walk two tiles — the sums carried from tile to tile, the flush at a segment change and at the
     workgroup's end — with the single shared counter copy (513 and 2048 bins), with the edges staged in LDS beside the counters, with
     8-byte weights off the 16-byte grid (guarded loads on both tiles of a walk) and with the last wave-private size;
     test_carry_over_and_flush of the first suite, the only two-tile case there, has 256 bins, the even integer form and aligned
     float32 weights (tests/test_whistogram.py pins that);
  B  the masses of wbins_load_masses, unsigned and signed, at the ends of both exponent ranges.

The layout comes from _whistogram_ref.big_boundaries_layout for the device's own CU count (tests/test_whistogram.py checks its paths on
the CPU at three CU counts); each test prints its geometry and asserts the path again before it compares.  Every comparison is exact
int64 equality with whistogram_oracle through run_check of tests/test_gpu_whistogram.py: sums pre-filled with the sentinel, a guard band
behind them.  Every engine a test creates is closed by the test.
"""
import numpy as np
import pytest

import _histogram_ref as H
import _whistogram_ref as W
import _wselect_ref as WS
from _whistogram_ref import signed_mass_np, whistogram_oracle
from test_gpu_whistogram import run_check
from test_gpu_wselect_paths import device_cus

pytestmark = pytest.mark.gpu

ALL_PATHS = {"lds_first", "lds_same", "lds_flush", "direct"}
CASES = ["uint64-edges-513-float64-skew1-signed", "float32-even-2048-uint32", "int32-descending-even-512-float32-signed"]


def segment_bins(rng, n, off, B, dtype):
    """_histogram_ref.shifted_bins for 2^24 keys (one random byte a key): segment s holds the bins s, s + 1 and s + 2, every 50th key
    the bin B + 1, which no form has; outside the segments the bins 0 .. 2"""
    b = rng.integers(0, 3, n, dtype=np.uint8).astype(dtype)
    o = off.astype(np.int64)
    for s in range(len(o) - 1):
        b[o[s]:o[s + 1]] += dtype(s)
    b[int(o[0]) + 7:int(o[-1]):50] = B + 1
    return b


def two_tile_case(which, n, off, rng):
    """(keys, weights, B, keywords of run_check).  Keys that fall outside every bin occur in each case; where the keys come from
    segment_bins a sum credited to a neighbouring segment shows."""
    if which == 0:
        B = 513
        step = np.uint64(H.SLOT_EDGE_STEP)
        edges = np.arange(B + 1, dtype=np.uint64) * step
        keys = segment_bins(rng, n, off, B, np.uint64) * step + step // np.uint64(2)          # (bin B + 1 lies behind the last edge)
        return keys, W.large_case_weights(rng, np.float64, n, off, 0), B, dict(bins=edges, signed=True, skew=1)
    if which == 1:
        B = 2048
        keys = (rng.random(n, dtype=np.float32) * np.float32(3.0) - np.float32(0.5))      # a third of them outside [0, 2]
        w = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        w[rng.random(n, dtype=np.float32) < 0.5] = 0xFFFFFFFF
        w[::10] = 0
        return keys, w, B, dict(bins=B, lo=0.0, hi=2.0)
    B = 512
    b = segment_bins(rng, n, off, B, np.int32)
    keys = np.where(b < B, B - 1 - b, b).astype(np.int32)                            # descending: bin b holds the key B - 1 - b; B + 1 is dropped
    return keys, W.large_case_weights(rng, np.float32, n, off, 0), B, dict(bins=B, lo=0, descending=True, signed=True)


@pytest.mark.parametrize("which", range(3), ids=CASES)
def test_two_tile_walk_carries_and_flushes(rsx, which):
    cus = device_cus()
    n, off = W.big_boundaries_layout(cus)
    rng = np.random.default_rng(700 + which)
    keys, w, B, kw = two_tile_case(which, n, off, rng)
    paths = W.piece_paths(n, off, B, cus)
    print(f"cus {cus} n {n} tiles {(n + H.TILE - 1) // H.TILE} tiles per workgroup {H.chunk_of(n, cus)} B {B} counters {W.lds_layout(B)} "
          f"pieces {len(paths)} flushes at a segment change {sum(p[3] == 'lds_flush' for p in paths)}")
    assert H.chunk_of(n, cus) == 2 and {p[3] for p in paths} == ALL_PATHS and W.lds_layout(B) == ("wave_private" if B == 512 else "shared")
    assert [(p[1], p[3]) for p in paths if p[0] == 3] == [(0, "lds_same"), (1, "lds_flush")]          # carried into a second tile and flushed there
    got, eng = run_check(rsx, keys, w, off, CASES[which], weight_exp=0, **kw)
    eng.sync()
    eng.close()
    o = off.astype(np.int64)
    dropped = H.bins_of(keys[o[0]:o[0] + 100000], kw["bins"], kw.get("lo", 0), kw.get("hi", 0), 0, kw.get("descending", False)) == H.NO_BIN
    assert dropped.any() and not dropped.all() and np.count_nonzero(got) >= 3 * len(got)
    if which != 1:                                                               # segment s has sums in the bins s .. s + 2 and nowhere else
        assert all(set(np.flatnonzero(row).tolist()) <= {s, s + 1, s + 2} for s, row in enumerate(got))
    if kw.get("signed"):
        assert (got < 0).any()


def signed_exponent_case(dtype, off, w, rng):
    """(keys, weights) of the signed form: about half of the weights negated; both infinities under every key of segment 2; segment 1's
    infinities all negative; and bin 7 of segment 0 holds +inf and -inf and nothing else: 2^31 - 2^31"""
    n = int(off[-1])
    o = off.astype(np.int64)
    w = np.where(rng.random(n) < 0.5, -w, w).astype(dtype)
    keys = rng.integers(0, 8, n).astype(np.uint32)
    seg1 = slice(int(o[1]), int(o[2]))
    w[seg1] = np.where(np.isinf(w[seg1]), -np.inf, w[seg1])
    at = int(o[2]) + rng.choice(int(o[3] - o[2]), 16, replace=False)
    keys[at] = np.repeat(np.arange(8), 2)
    w[at] = np.tile([np.inf, -np.inf], 8)
    first = slice(0, int(o[1]))
    keys[first] = np.where(keys[first] == 7, 3, keys[first])
    w[first] = np.where(np.isinf(w[first]), dtype(-0.0), w[first])                    # (segment 0: no infinity but the planted pair)
    at = rng.choice(int(o[1]), 5, replace=False)
    w[at[:3]] = [-np.finfo(dtype).smallest_subnormal, -0.0, -np.finfo(dtype).tiny / 2]
    keys[at[3:]] = 7
    w[at[3:]] = [np.inf, -np.inf]
    return keys, w


def test_weight_exponents_on_the_device(rsx):
    """_wselect_ref.exponent_cases through wbins_load_masses and signed_addend: float32 and float64 weights at weight_exp from -2048 to
    2048, 8 bins.  Unsigned: the weights as they are (a negative weighs nothing).  Signed: about half negated, -inf, negative denormals
    and -0.0 among them, both signs of a saturated mass under every key, negative sums, and one bin whose masses cancel to exactly 0."""
    rng = np.random.default_rng(720)
    eng = rsx.Engine(np.uint32, 4096)
    B = 8
    for dtype, wexp, off, w in WS.exponent_cases():
        what = f"{np.dtype(dtype).name} weight_exp={wexp}"
        keys = rng.integers(0, B, w.size).astype(np.uint32)
        got, _ = run_check(rsx, keys, w, off, what + " unsigned", eng=eng, bins=B, weight_exp=wexp)
        assert (got >= 0).all() and (got > 0).any()
        keys, ws = signed_exponent_case(dtype, off, w, rng)
        m = signed_mass_np(ws, wexp, True)
        print(what, "masses: negative", int((m < 0).sum()), "zero", int((m == 0).sum()), "positive", int((m > 0).sum()),
              "saturated", int((np.abs(m) == WS.MASS_ONE).sum()))
        assert all((m[keys == b] > 0).any() and (m[keys == b] < 0).any() for b in range(B))                  # every bin receives both signs
        assert np.isneginf(ws).any() and (np.signbit(ws) & (ws == 0)).any() and ((ws < 0) & (np.abs(ws) < np.finfo(dtype).tiny)).any()
        in7 = np.flatnonzero(keys[:int(off[1])] == 7)
        assert sorted(m[in7].tolist()) == [-WS.MASS_ONE, WS.MASS_ONE]
        want = whistogram_oracle(keys, ws, off, B, weight_exp=wexp, signed=True)
        assert (want < 0).any() and want[0, 7] == 0
        got, _ = run_check(rsx, keys, ws, off, what + " signed", eng=eng, bins=B, weight_exp=wexp, signed=True)
        assert np.array_equal(got, want)
    eng.sync()
    eng.close()
