"""Helpers of the segmented-sort path tests (tests/test_gpu_segmented_paths.py): a mirror of what one rsx_segmented_sort launches and
classifies, a checker of the covered positions that does not loop over the segments, the key sets that starve the ranking of digits,
and the layouts the GPU tests run, held here with fixed seeds so that tests/test_segmented.py can check on the CPU that each one
still reaches the path it is named for.

seg_geometry restates seg_shape / segmented_enqueue of capi_segmented.inc (grids from n and the segment count alone) and
seg_classify_kernel / seg_scan_kernel / seg_tile of rsx_segmented.hpp (validity, classes, block sums, the chain's bounds, tiles on the
global grid clipped at segment ends).  Every constant is written out beside the name it has in the C++.
"""
import numpy as np

import _topk_ref as R
from test_gpu_float_keys import UINT, random_bits

TILE = 4096               # rsx::kSegTileKeys: tiles of the large-segment chain, on the global 4096-key grid
CLASS0_MAX = 256          # rsx::kSegClass0Max: class 0 = 2..256 keys (64 threads x 4 keys)
CLASS1_MAX = 1024         # rsx::kSegClass1Max: class 1 = 257..1024 keys (64 x 16); class 2 = 1025..4096 (256 x 16)
SEG_PER_BLOCK = 2048      # rsx::kSegPerBlock = kSegClassifyThreads (256) x kSegPerThread (8): segments per classify workgroup
SCAN_THREADS = 256        # rsx::kSegScanThreads: each thread of seg_scan_kernel takes `per` consecutive classify blocks
MIN_LEN = (2, CLASS0_MAX + 1, CLASS1_MAX + 1)      # min_len[] of segmented_enqueue: the shortest segment of each small class
PER_CU = (32, 16, 4)      # per_cu[] of segmented_enqueue: resident workgroups of seg_small_sort_kernel per CU, by class
CHAIN_PER_CU = 8          # the chain's grid: min(max_tiles, cus * 8)
CUS = 256                 # MI355X compute units: the engine's cus when it asks the device


def covered(off, n: int) -> np.ndarray:
    """Positions inside valid segments, as covered() of tests/test_gpu_segmented.py gives them, without a loop over the segments: +1
    at every valid a, -1 at every valid b, a running sum (valid segments may overlap when the offsets fold back)."""
    off = np.asarray(off, dtype=np.int64)
    a, b = off[:-1], off[1:]
    ok = (a <= b) & (b <= n)
    d = np.zeros(n + 1, dtype=np.int64)
    np.add.at(d, a[ok], 1)
    np.add.at(d, b[ok], -1)
    return np.cumsum(d[:n]) > 0


def _ceil(a: int, b: int) -> int:
    return (a + b - 1) // b


def seg_geometry(off, n: int, cus: int = CUS) -> dict:
    """What one rsx_segmented_sort call over these offsets launches and where every segment goes.
      valid / bad / first_bad        seg_classify_kernel: b < a or b > n is bad (first_bad None when there is none)
      ones, count[3], large          one-key copies, the three LDS classes, the segments of more than 4096 keys (indices, in order)
      lists[3]                       the class lists in the order seg_classify_kernel<true> writes them (segment order)
      nblocks, per                   classify workgroups; blocks per thread of seg_scan_kernel
      large_blocks, last_large_block distinct classify blocks that hold a large segment, and the highest of them
      grid[3], trips[3]              seg_small_sort_kernel's grids and how many items its busiest workgroup walks
      max_large, max_tiles           seg_shape: what the host sizes the chain's scratch by
      tot_large, tot_tiles, tot_keys what seg_scan_kernel adds up; chain_ok is its comparison with the bounds
      nlarge, tiles                  SegHeader: the totals, or 0 when chain_ok is 0
      chain_grid                     workgroups of seg_histogram_kernel / seg_reorder_kernel
      first_tile, last_tile          per large segment, the keys of its first and last tile (seg_tile)"""
    off = np.asarray(off, dtype=np.int64)
    nseg = len(off) - 1
    a, b = off[:-1], off[1:]
    valid = (b >= a) & (b <= n)
    bad = np.flatnonzero(~valid)
    lens = np.where(valid, b - a, 0)
    cls = np.where(lens <= CLASS0_MAX, 0, np.where(lens <= CLASS1_MAX, 1, np.where(lens <= TILE, 2, 3)))
    sortable = lens >= 2
    lists = [np.flatnonzero(sortable & (cls == c)) for c in range(3)]
    large = np.flatnonzero(sortable & (cls == 3))
    la, lb = a[large], b[large]
    tiles = (lb + TILE - 1) // TILE - la // TILE                      # seg_tiles
    nblocks = _ceil(nseg, SEG_PER_BLOCK)
    max_large = min(nseg, n // (TILE + 1))
    max_tiles = _ceil(n, TILE) + max_large if max_large else 0
    tot_large, tot_tiles, tot_keys = int(large.size), int(tiles.sum()), int((lb - la).sum())
    chain_ok = tot_large <= max_large and tot_tiles <= max_tiles and tot_keys <= n
    grid = [min(nseg, n // MIN_LEN[c], cus * PER_CU[c]) for c in range(3)]
    count = [int(l.size) for l in lists]
    blocks = np.unique(large // SEG_PER_BLOCK)
    return {
        "valid": valid, "bad": bad, "first_bad": int(bad[0]) if bad.size else None,
        "ones": int(np.count_nonzero(lens == 1)), "count": count, "large": large, "lists": lists,
        "nblocks": nblocks, "per": _ceil(nblocks, SCAN_THREADS),
        "large_blocks": int(blocks.size), "last_large_block": int(blocks[-1]) if blocks.size else None,
        "grid": grid, "trips": [_ceil(count[c], grid[c]) if grid[c] else 0 for c in range(3)],
        "max_large": max_large, "max_tiles": max_tiles, "tot_large": tot_large, "tot_tiles": tot_tiles, "tot_keys": tot_keys,
        "chain_ok": int(chain_ok), "nlarge": tot_large if chain_ok else 0, "tiles": tot_tiles if chain_ok else 0,
        "chain_grid": min(max_tiles, cus * CHAIN_PER_CU),
        "first_tile": (np.minimum(lb, (la // TILE + 1) * TILE) - la).tolist(),
        "last_tile": (lb - np.maximum(la, (lb - 1) // TILE * TILE)).tolist(),
    }


def summary(g: dict) -> str:
    """the figures of seg_geometry on one line (what the GPU tests print before they assert their path condition)"""
    return (f"count={g['count']} grid={g['grid']} trips={g['trips']} nblocks={g['nblocks']} per={g['per']} large_blocks={g['large_blocks']} "
            f"last_large_block={g['last_large_block']} nlarge={g['nlarge']}/{g['max_large']} tiles={g['tiles']}/{g['max_tiles']} "
            f"chain_ok={g['chain_ok']} chain_grid={g['chain_grid']} bad={g['bad'].size}")


def offsets_from(lengths, start=0):
    return np.concatenate([[start], start + np.cumsum(lengths)]).astype(np.uint64)


# -- 1, 2. sparse large segments over many classify blocks ---------------------------------------------------------------------------------

SPARSE_SEGMENTS = 600000
SPARSE_FORCED = (2047, 2048, SPARSE_SEGMENTS - 1)      # the last segment of classify block 0, the first of block 1, the last of all
SPARSE_SPIKES = (550002, 580001)                       # beyond segment 524288: in blocks the scan's threads reach with per == 2 only


def sparse_large(seed: int = 1):
    """600000 segments of 0..3 keys; about 40 of 4097..9000 keys at seeded indices and at 2047, 2048 and 599999; a few of 300 and of
    2000 keys; off[0] = 3, off[S] = n.  Path: per == 2 (more than 256 classify blocks), large segments in at least 30 distinct
    blocks, the last block among them: the block prefixes of SF_LARGE / SF_TILES / SF_KEYS, SegLarge::dest and tstart[] are non-zero
    almost everywhere.  Returns (n, off)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 4, SPARSE_SEGMENTS)
    where = rng.choice(SPARSE_SEGMENTS, 60, replace=False)
    lens[where[:40]] = rng.integers(TILE + 1, 9001, 40)
    lens[where[40:50]] = 300
    lens[where[50:]] = 2000
    lens[list(SPARSE_FORCED)] = rng.integers(TILE + 1, 9001, len(SPARSE_FORCED))
    off = offsets_from(lens, start=3)
    return int(off[-1]), off


def sparse_large_bad(seed: int = 1):
    """sparse_large with one offset spiked to n + 7 at two places beyond segment 524288: segments 550001 / 550002 and 580000 / 580001
    are bad (one ends past n, the next one decreases), every other segment is as before, so no valid segment overlaps another.
    Path: the first bad segment comes out of the second block of a scan thread; large segments follow the spikes.  Returns (n, off)."""
    n, off = sparse_large(seed)
    off = off.copy()
    for s in SPARSE_SPIKES:
        off[s] = n + 7
    return n, off


# -- 3. more segments of class 1 / class 2 than workgroups ---------------------------------------------------------------------------------

def stride_layout(cls: int, cus: int = CUS, seed: int = 0):
    """32 * cus + 400 segments of 2..256 keys (cls 0), 16 * cus + 400 of 257..1024 keys (cls 1) or 4 * cus + 200 of 1025..4096 keys
    (cls 2), contiguous from off[0] = 1.  Wherever a workgroup has a second item (item i + grid after item i), the second one is the
    shorter of the two, so its pads lie over the image of a longer segment.  Path: trips[cls] >= 2.  Returns (n, off); few_distinct()
    makes the keys.  (Class 0 serves the selects' LDS sorts; the segmented sort's own tests run classes 1 and 2.)"""
    rng = np.random.default_rng(300 + seed + cls)
    lo, hi = ((2, CLASS0_MAX), (CLASS0_MAX + 1, CLASS1_MAX), (CLASS1_MAX + 1, TILE))[cls]
    grid = cus * PER_CU[cls]
    extra = 200 if cls == 2 else 400
    lens = rng.integers(lo, hi, grid + extra, endpoint=True)
    first, second = lens[:extra].copy(), lens[grid:].copy()
    lens[:extra] = np.maximum(np.maximum(first, second), lo + 1)
    lens[grid:] = np.minimum(np.minimum(first, second), lens[:extra] - 1)
    off = offsets_from(lens, start=1)
    return int(off[-1]), off


def few_distinct(dtype, off, n: int, rng) -> np.ndarray:
    """every other segment holds the values 0..6 only (long runs of ties: few digits in every pass), the rest random bits"""
    x = random_bits(dtype, n, rng)
    off = np.asarray(off, dtype=np.int64)
    lens = np.diff(off)
    seg = np.repeat(np.arange(lens.size), lens)
    few = np.zeros(n, dtype=bool)
    few[int(off[0]):int(off[-1])] = seg % 2 == 0
    x[few] = rng.integers(0, 7, int(few.sum())).astype(dtype)
    return x


# -- 4. one digit per pass, and pads -------------------------------------------------------------------------------------------------------

DIGIT_LENGTHS = [5, 200, 257, 1000, 1025, 4096, 4097, 30000, 2, 70001]
DIGIT_SETS = ("equal", "digits_7_8", "digits_0_15", "window", "low", "straddle", "pad_heavy", "sorted", "reversed")


def nibble_words(u, n: int, rng, lo: int, hi: int) -> np.ndarray:
    """words whose 4-bit digits are all lo or hi, each chosen at random"""
    bits = np.dtype(u).itemsize * 8
    o = np.zeros(n, dtype=u)
    for j in range(bits // 4):
        o |= np.where(rng.integers(0, 2, n) == 1, u(hi), u(lo)).astype(u) << u(4 * j)
    return o


def digit_keys(kind: str, dtype, off, n: int, rng, descending: bool) -> np.ndarray:
    """The key sets of case 4, built in the call's order (R.from_order: the digits named are those of the order-mapped key, whichever
    the direction).
      equal         one key everywhere: one digit in every pass, the order is the index order
      digits_7_8    every digit is 7 or 8: the two counters that share a dword's halves, and the low total carried into the high half
      digits_0_15   every digit is 0 or 15: the first counter and the pads' own
      window / low / straddle   R.digit_local: only one byte, or the low bytes, differ inside a segment
      pad_heavy     R.pad_heavy: most real keys ARE the pad key (all ones in the call's order)
      sorted / reversed         random keys with ties, every segment already in the call's order / in the opposite one"""
    u = UINT[np.dtype(dtype)]
    if kind == "equal":
        return R.from_order(np.full(n, R._words(u, 1, rng)[0], dtype=u), dtype, descending)
    if kind == "digits_7_8":
        return R.from_order(nibble_words(u, n, rng, 7, 8), dtype, descending)
    if kind == "digits_0_15":
        return R.from_order(nibble_words(u, n, rng, 0, 15), dtype, descending)
    if kind in ("window", "low", "straddle"):
        return R.digit_local(dtype, off, n, rng, kind, descending)
    if kind == "pad_heavy":
        return R.pad_heavy(dtype, off, n, rng, descending)
    assert kind in ("sorted", "reversed")
    o = R._words(u, n, rng)
    o[rng.integers(0, n, n // 3)] = o[rng.integers(0, n, n // 3)]           # ties
    off = np.asarray(off, dtype=np.int64)
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        o[a:b] = np.sort(o[a:b]) if kind == "sorted" else np.sort(o[a:b])[::-1]
    return R.from_order(o, dtype, descending)


# -- 5. the chain's tiles against the 4096-key grid ------------------------------------------------------------------------------------------

# (first tile, last tile) of the six large segments of grid_layout, in order
GRID_TILES = [(1, 1), (TILE, TILE), (TILE, 1), (TILE - 1, 905), (3191, 2809), (986, 1)]


def grid_layout():
    """Contiguous segments from 0 to n = 12 * 4096 + 1, small and empty ones between six large ones:
      [4095, 8193)    a % 4096 == 4095, 4098 keys: tiles of 1, 4096 and 1 keys
      [12288, 20480)  starts and ends on grid lines: two whole tiles
      [20480, 24577)  4097 keys from a grid line: a whole tile and one key
      [24577, 29577) and [29577, 35577)   two large segments that meet inside grid tile 7
      [35878, 49153)  ends at off[S] == n, n % 4096 == 1: a last tile of one key
    Path: GRID_TILES.  Returns (n, off)."""
    lens = [4095, 4098, 0, 3, 4092, 8192, 4097, 5000, 6000, 0, 1, 300, 13275]
    off = offsets_from(lens)
    return int(off[-1]), off


def full_house_layout():
    """37 segments of 4097 keys from 0, n = off[S]: as many large segments as n keys can hold.  Path: nlarge == max_large (the last
    rows of seg_large and seg_tstart are used, and tstart[nlarge] is the last element of its buffer).  Returns (n, off)."""
    off = offsets_from([TILE + 1] * 37)
    return int(off[-1]), off


# -- 6. one payload engine, growing then shrinking -------------------------------------------------------------------------------------------

ENGINE_CAPACITY = 1 << 22


def engine_sequence():
    """the calls of case 6 in order, (lengths, off[0]): one segment of the whole capacity, 200 large ones, a mix from 9000, 3000 of
    class 1, then shapes that use the first rows only of everything the larger calls left behind"""
    return [([ENGINE_CAPACITY], 0), ([TILE + 1] * 200, 0), ([70000, TILE + 1, 3], 9000), ([300] * 3000, 0), ([5000, 100], 0), ([17], 0)]


# -- 8. offsets that fold back ---------------------------------------------------------------------------------------------------------------

FOLD_LARGE = (5000, np.array([0, 5000, 0, 5000, 0, 5000], dtype=np.uint64))
FOLD_SMALL = (300, np.array([0, 300, 0, 300, 0, 300, 0, 300], dtype=np.uint64))
