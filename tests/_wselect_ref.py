"""Host referee of the weighted-select tests (rsx_segmented_weighted_select): the stable argsort of the order-mapped keys (seg_oracle, as
tests/_select_ref.py), the mass function in numpy, a uint64 cumsum of the masses in sorted order, searchsorted, and the target rule.

mass_np         mass(w) = 0 unless w > 0, else min(floor(w * 2^(31 - weight_exp)), 2^31); the stored word for the uint32 kind.
target_of       the target of one slot as a mass in [1, total], 0 for "no answer" (absolute and fraction form).
wselect_oracle  (keys [S, R] unsigned words, pos [S, R] uint32, rank [S, R] uint32, mass [S, R] uint64, written [S, R] bool,
                total [S] uint64, valid [S] bool): `written` marks the slots the call writes, `valid` the segments whose total it writes.
Referee         wselect_oracle in two steps: the sort and the running masses once per upload, then the answers of any targets.
brute_force     the same answer with Python integers and a plain loop, for the referee's own test.

For the path tests (tests/test_gpu_wselect_paths.py; tests/test_wselect.py checks on the CPU, at 256 CUs, that each layout reaches the
path it is there for):
wselect_geometry  a mirror of what wselect_enqueue of capi_wselect.inc launches, from n and the offsets; summary() puts it on one line.
many_large, long_segment, exponent_weights   the layouts and inputs of their own; _segmented_ref.stride_layout is the fourth.
"""
import math

import numpy as np

import _segmented_ref as S
import _topk_ref
from test_gpu_float_keys import UINT
from test_gpu_segmented import seg_oracle

WEIGHT_UINT32, WEIGHT_FLOAT32, WEIGHT_FLOAT64 = 0, 1, 2
MASS_ONE = 1 << 31


def kind_of(weights: np.ndarray) -> int:
    return {np.dtype(np.uint32): WEIGHT_UINT32, np.dtype(np.float32): WEIGHT_FLOAT32, np.dtype(np.float64): WEIGHT_FLOAT64}[weights.dtype]


def mass_np(w: np.ndarray, weight_exp: int = 0) -> np.ndarray:
    """uint64 masses of a uint32 / float32 / float64 weight array."""
    w = np.asarray(w)
    if w.dtype == np.uint32:
        return w.astype(np.uint64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        s = np.floor(np.ldexp(w.astype(np.float64), 31 - int(weight_exp)))      # exact: a power-of-two scaling (an underflow is below 1 either way)
        s = np.minimum(s, float(MASS_ONE))
    return np.where(w > 0, s, 0.0).astype(np.uint64)


def target_of(total: int, t, fraction: bool) -> int:
    if not fraction:
        t = int(t)
        return t if 1 <= t <= total else 0
    f = float(t)
    if math.isnan(f) or total == 0:
        return 0
    td = float(total)                       # round to nearest
    x = td * f
    if not x > 1.0:
        return 1
    if x >= td:
        return total
    return int(math.ceil(x))


class Referee:
    """wselect_oracle with the work that does not depend on the targets done once per upload: the stable argsort, the masses in sorted
    order and their running sum.  Referee(x, off, weights, descending, weight_exp)(targets, fraction) is wselect_oracle's tuple;
    `total` [S] uint64 and `valid` [S] bool are there before any call (the tests form their targets from the totals)."""

    def __init__(self, x: np.ndarray, off, weights, descending: bool = False, weight_exp: int = 0):
        n = x.size
        self.x = x
        self.off = np.asarray(off, dtype=np.int64)
        self.order = seg_oracle(x, self.off, n, descending)
        m = mass_np(x if weights is None else weights, weight_exp)
        # masses in sorted order, summed over the whole array: a segment's running masses are run[a:b] - run[a - 1] (n <= 2^31 masses
        # of at most 2^32 - 1: below 2^63)
        self.run = np.cumsum(m[self.order], dtype=np.uint64)
        a, b = self.off[:-1], self.off[1:]
        self.valid = (a <= b) & (b <= n)
        ends = np.concatenate([[np.uint64(0)], self.run])
        self.total = np.where(self.valid, ends[np.where(self.valid, b, 0)] - ends[np.where(self.valid, a, 0)], 0).astype(np.uint64)

    def __call__(self, targets, fraction: bool = False):
        x, off = self.x, self.off
        nseg = len(off) - 1
        tt = np.asarray(targets).reshape(nseg, -1)
        R = tt.shape[1]
        u = UINT[x.dtype]
        xu = x.view(u)
        keys = np.zeros((nseg, R), dtype=u)
        pos = np.zeros((nseg, R), dtype=np.uint32)
        rank = np.zeros((nseg, R), dtype=np.uint32)
        mass = np.zeros((nseg, R), dtype=np.uint64)
        written = np.zeros((nseg, R), dtype=bool)
        for s in np.flatnonzero(self.valid & (self.total > 0)):
            a, b = int(off[s]), int(off[s + 1])
            tot = int(self.total[s])
            base = int(self.run[a - 1]) if a else 0
            for q in range(R):
                T = target_of(tot, tt[s, q], fraction)
                if T == 0:
                    continue
                r = int(np.searchsorted(self.run[a:b], np.uint64(base + T), side="left"))
                src = int(self.order[a + r])
                keys[s, q] = xu[src]
                pos[s, q] = src - a
                rank[s, q] = r
                mass[s, q] = int(self.run[a + r]) - base
                written[s, q] = True
        return keys, pos, rank, mass, written, self.total.copy(), self.valid.copy()


def wselect_oracle(x: np.ndarray, off, weights, targets, fraction: bool = False, descending: bool = False, weight_exp: int = 0):
    return Referee(x, off, weights, descending, weight_exp)(targets, fraction)


def brute_force(x: np.ndarray, weights, T: int, descending: bool = False, weight_exp: int = 0):
    """One segment, one absolute target, Python integers: (position, rank, mass so far, total) or (None, None, None, total)."""
    from test_gpu_float_keys import enc
    e = enc(x)
    if descending:
        e = ~e
    idx = sorted(range(x.size), key=lambda i: (int(e[i]), i))
    m = [int(v) for v in mass_np(x if weights is None else weights, weight_exp)]
    total = sum(m)
    run = 0
    for r, i in enumerate(idx):
        run += m[i]
        if T >= 1 and run >= T:
            return i, r, run, total
    return None, None, None, total


def random_targets(total: np.ndarray, R: int, rng) -> np.ndarray:
    """[S, R] uint64: random targets in [1, total] with the edge targets 0, 1, total, total + 1 and duplicates mixed in."""
    S = len(total)
    out = np.empty((S, R), dtype=np.uint64)
    for s in range(S):
        tot = int(total[s])
        row = [int(rng.integers(1, tot + 1)) if tot else 0 for _ in range(R)]
        edge = [0, 1, tot, tot + 1, row[0], tot // 2]
        for q in range(R):
            if rng.random() < 0.4:
                row[q] = edge[int(rng.integers(0, len(edge)))]
        out[s] = row
    return out


# -- launch geometry of the chain (mirrors wselect_enqueue of capi_wselect.inc) ---------------------------------------------------------------

TILE = _topk_ref.TILE     # rsx::kSegTileKeys
CUS = _topk_ref.CUS       # MI355X compute units: the engine's cus when it asks the device
PICK_PER_CU = 2           # pgrid = min(max_large * R, cus * 2): wselect_pick_kernel, wselect_find_kernel, wselect_locate_kernel
TIE_PER_CU = 8            # tgrid = min(max_tiles, cus * 8): wselect_tie_kernel
FIND_CHUNK = 1024         # rsx::kWselFindThreads: tiles of one segment that wselect_find_kernel scans at a time


def wselect_geometry(off, n: int, R: int, cus: int = CUS) -> dict:
    """What one rsx_segmented_weighted_select over these (valid) offsets launches, from _topk_ref.select_geometry (the group width and
    the large segments that begin inside a group) and _segmented_ref.seg_geometry (seg_shape's bounds, the three LDS classes):
      gtiles, groups      tiles per workgroup of wselect_hist_kernel (topk_group_tiles); its grid, ceil(max_tiles / gtiles)
      switches            large segments that begin inside a group: each makes the hist kernel flush, step on and reload the state
      nlarge, items       large segments; items = nlarge * R of the pick, find and locate kernels, on pick_grid = min(max_large * R, 2 * cus)
      tiles, tie_grid     tiles of the large segments; wselect_tie_kernel's grid min(max_tiles, 8 * cus)
      max_segment_tiles   the tiles of the longest segment (wselect_find_kernel walks them 1024 at a time)
      count[3], sort_grid[3], trips[3], lists[3]   the LDS classes: members, wselect_sort_kernel's grids, items of the busiest workgroup"""
    sel = _topk_ref.select_geometry(off, n, cus)
    seg = S.seg_geometry(off, n, cus)
    assert seg["first_bad"] is None and seg["chain_ok"] == 1 and sel["nlarge"] == seg["nlarge"] and sel["tiles"] == seg["tiles"]
    o = np.asarray(off, dtype=np.int64)
    la, lb = o[seg["large"]], o[seg["large"] + 1]
    per_segment = (lb + TILE - 1) // TILE - la // TILE
    gtiles = sel["gtiles"]
    return {
        "n": int(n), "nseg": len(o) - 1, "R": int(R), "cus": int(cus),
        "gtiles": gtiles, "groups": (seg["max_tiles"] + gtiles - 1) // gtiles, "switches": sel["switches"],
        "nlarge": seg["nlarge"], "items": seg["nlarge"] * R, "pick_grid": min(seg["max_large"] * R, PICK_PER_CU * cus),
        "tiles": seg["tiles"], "tie_grid": min(seg["max_tiles"], TIE_PER_CU * cus),
        "max_segment_tiles": int(per_segment.max()) if per_segment.size else 0,
        "count": seg["count"], "sort_grid": seg["grid"], "trips": seg["trips"], "lists": seg["lists"],
    }


def summary(g: dict) -> str:
    """the figures of wselect_geometry on one line (what the GPU tests print before they assert their path condition)"""
    return (f"n={g['n']} segments={g['nseg']} R={g['R']} cus={g['cus']} gtiles={g['gtiles']} groups={g['groups']} switches={g['switches']} "
            f"items={g['items']}/{g['pick_grid']} tiles={g['tiles']}/{g['tie_grid']} max_segment_tiles={g['max_segment_tiles']} "
            f"count={g['count']} sort_grid={g['sort_grid']} trips={g['trips']}")


def second_items_are_shorter(g: dict, off, cls: int) -> bool:
    """every item a workgroup of wselect_sort_kernel / select_sort_kernel takes after its first (item i + grid) is shorter than item i"""
    lens = np.diff(np.asarray(off, dtype=np.int64))
    order, grid = g["lists"][cls], g["sort_grid"][cls]
    second = np.arange(grid, g["count"][cls])
    return second.size > 0 and bool(np.all(lens[order[second]] < lens[order[second - grid]]))


# -- layouts of the path tests ---------------------------------------------------------------------------------------------------------------

MANY_SMALL = (0, 1, 2, 255, 257, 1025, 4096)


def many_large(cus: int = CUS, seed: int = 0):
    """4 * cus large segments of 4097..8000 keys, after every third one a small segment drawn from MANY_SMALL (empty, one key, every LDS
    class); off[0] = 3, n = off[-1] + 5.  Path (at R = 4): gtiles >= 2, at least `cus` large segments begin inside a group, more than
    twice as many (segment, target) items as workgroups of the pick grid, more tiles than workgroups of the tie grid.  Returns (n, off)."""
    rng = np.random.default_rng(700 + seed)
    lens = []
    for i in range(4 * cus):
        lens.append(int(rng.integers(TILE + 1, 8001)))
        if i % 3 == 2:
            lens.append(int(rng.choice(MANY_SMALL)))
    off = S.offsets_from(lens, start=3)
    return int(off[-1]) + 5, off


LONG_LENGTHS = [5000, 1030 * TILE + 17, 300, TILE + 1]
LONG_SEGMENT = 1


def long_segment():
    """LONG_LENGTHS from off[0] = 3: segment 1 has 1031 tiles, more than one chunk of wselect_find_kernel.  Returns (n, off)."""
    off = S.offsets_from(LONG_LENGTHS, start=3)
    return int(off[-1]), off


def long_targets(total: int) -> list:
    """the long segment's targets: the carry into the second chunk decides the first and the third (all keys equal), the first (0..6)"""
    return [total - 5, total // 2, total * 1025 // 1030, 1]


def answer_tiles(off, s: int, pos) -> list:
    """index within segment s of the tile (on the global 4096-key grid) that holds each position of `pos`"""
    a = int(np.asarray(off, dtype=np.int64)[s])
    return [(a + int(p)) // TILE - a // TILE for p in pos]


EXP_LENGTHS = [300, 5000, 20000]
WEIGHT_EXPS = (-2048, -1074, -149, -126, 0, 127, 1023, 2048)


def exponent_cases():
    """(weight dtype, weight_exp, off, weights) for float32 and float64 weights at every exponent of WEIGHT_EXPS, with fixed seeds"""
    off = S.offsets_from(EXP_LENGTHS)
    for d, dtype in enumerate((np.float32, np.float64)):
        for i, wexp in enumerate(WEIGHT_EXPS):
            yield dtype, wexp, off, exponent_weights(dtype, off, wexp, np.random.default_rng(900 + 16 * d + i))


def exponent_weights(dtype, off, weight_exp: int, rng) -> np.ndarray:
    """Weights for the segments of `off` (from 0) around 2^weight_exp.  Even positions: ldexp(s, weight_exp - k) with s in [0.5, 1) and k in
    0..40, i.e. masses of 31 - k significant bits just below saturation, wherever `dtype` holds that value as a finite non-zero number;
    all other positions: random bit patterns of the type (either sign, every exponent: NaNs, denormals, huge and tiny values).  Planted
    on top: infinities, NaNs and zeros of both signs and the smallest and largest denormal, +inf beyond segment 0 only, so that segment
    0 can weigh nothing when weight_exp lies above every finite weight."""
    dtype = np.dtype(dtype)
    u = UINT[dtype]
    n = int(off[-1])
    w = rng.integers(0, np.iinfo(u).max, size=n, dtype=u, endpoint=True).view(dtype)
    with np.errstate(over="ignore", under="ignore"):
        v = np.ldexp(0.5 + rng.random(n) / 2, int(weight_exp) - rng.integers(0, 41, n)).astype(dtype)
    ok = np.isfinite(v) & (v != 0)
    ok[1::2] = False
    w[ok] = v[ok]
    tiny = np.finfo(dtype).smallest_subnormal
    plant = np.array([np.inf, -np.inf, np.nan, -np.nan, 0.0, -0.0, tiny, np.finfo(dtype).tiny - tiny, -tiny], dtype=dtype)
    for lo, hi in ((int(off[1]), int(off[2])), (int(off[2]), n)):
        w[rng.choice(np.arange(lo, hi), plant.size, replace=False)] = plant
    w[rng.choice(int(off[1]), plant.size - 1, replace=False)] = plant[1:]
    return w
