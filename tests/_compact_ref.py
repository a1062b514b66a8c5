"""Host referee of rsx_segmented_compact (no GPU, no library): two independent forms of the same definition, the grid the kernels state
at the top of radix-sort_amd/csrc/rsx_compact.hpp, and the layouts the GPU tests run (so that the CPU suite can check, from the layout
alone, that each reaches the path it is named after).

Element i of segment s = [off[s], off[s+1]) is KEPT iff mask[i] != 0 (mask form) or iff its key does not come after bounds[s] in the
engine's order — unsigned order of _search_ref.order_map — (bound form; strict: comes strictly before); invert flips either.  With K(i)
the kept elements in [off[0], i):
  compact mode     kept element i -> keys_out[K(i)], index_out[K(i)] = i - off[s]; nothing else is written
  partition mode   inside [off[s], off[s+1]) the kept elements first, the rejected behind them, both in input order; index_out holds where
                   each came from, relative to off[s]; positions outside [off[0], off[S]) are not written
  koff[s] = K(off[s]) in both.

  compact_oracle   numpy, vectorised
  compact_loop     a plain loop over the elements (small inputs)
Both return (keys_out, index_out, koff, written): arrays of n entries, `written` marking the positions the call must write (every other
position must keep what it held).

The grid: tiles of TILE = 4096 consecutive positions, 256 threads x 16; the table has tiles + 1 entries padded to a multiple of 16; a
workgroup walks ceil(padded / (16 x CUs)) consecutive tiles; the table is scanned as 16 rows by workgroups of SCAN_BLOCK entries a row.
"""
import numpy as np

from _search_ref import order_map

TILE = 4096
THREADS = 256
SCAN_BLOCK = 256           # kScanTiles
PARTITION, INVERT, STRICT = 8, 16, 32
LENGTHS = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 9000, 0, 3, 20011]       # test_search.LENGTHS
MASK_BYTES = np.array([0, 1, 2, 0x80, 0xFF], dtype=np.uint8)


def _offsets(n, off):
    return np.array([0, n], dtype=np.int64) if off is None else np.asarray(off).astype(np.int64)


def keep_flags(keys, off, mask=None, bounds=None, descending=False, strict=False, invert=False) -> np.ndarray:
    """the predicate of every element of [0, n) (elements outside the segments included: the callers cut them off)"""
    assert (mask is None) != (bounds is None), "exactly one of mask and bounds"
    o = _offsets(keys.size, off)
    if mask is not None:
        assert not strict, "strict belongs to the bound form"
        keep = np.asarray(mask).view(np.uint8) != 0
    else:
        seg = np.repeat(np.arange(o.size - 1), np.diff(o))
        k, b = order_map(keys, descending), order_map(np.asarray(bounds, dtype=keys.dtype), descending)
        keep = np.zeros(keys.size, dtype=bool)
        live = k[o[0]:o[-1]]
        keep[o[0]:o[-1]] = (live < b[seg]) if strict else (live <= b[seg])
    return ~keep if invert else keep


def compact_oracle(keys, off, mask=None, bounds=None, descending=False, strict=False, invert=False, partition=False):
    n = keys.size
    o = _offsets(n, off)
    lo, hi = int(o[0]), int(o[-1])
    keep = keep_flags(keys, off, mask, bounds, descending, strict, invert)
    keep[:lo] = False
    keep[hi:] = False
    K = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    koff = K[o]
    pos = np.arange(n, dtype=np.int64)
    seg = np.repeat(np.arange(o.size - 1), np.diff(o))
    start = np.zeros(n, dtype=np.int64)
    start[lo:hi] = o[seg]
    keys_out, index_out, written = np.zeros(n, dtype=keys.dtype), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    if not partition:
        total = int(K[-1])
        keys_out[:total] = keys[keep]
        index_out[:total] = (pos - start)[keep]
        written[:total] = True
        return keys_out, index_out, koff, written
    live = np.zeros(n, dtype=bool)
    live[lo:hi] = True
    kept_before = np.zeros(n, dtype=np.int64)                  # kept elements of the own segment before i
    kept_before[lo:hi] = K[lo:hi] - koff[seg]
    kept_s = np.zeros(n, dtype=np.int64)
    kept_s[lo:hi] = (koff[1:] - koff[:-1])[seg]
    rel = pos - start
    dest = np.where(keep, start + kept_before, start + kept_s + rel - kept_before)
    keys_out[dest[live]] = keys[live]
    index_out[dest[live]] = rel[live]
    written[lo:hi] = True
    return keys_out, index_out, koff, written


def compact_loop(keys, off, mask=None, bounds=None, descending=False, strict=False, invert=False, partition=False):
    """the definition, element by element"""
    n = keys.size
    o = [int(v) for v in _offsets(n, off)]
    k = [int(v) for v in order_map(keys, descending)]
    b = None if bounds is None else [int(v) for v in order_map(np.asarray(bounds, dtype=keys.dtype), descending)]
    m = None if mask is None else [int(v) for v in np.asarray(mask).view(np.uint8)]
    keys_out, index_out, written = np.zeros(n, dtype=keys.dtype), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    koff, total = [], 0
    for s in range(len(o) - 1):
        koff.append(total)
        yes, no = [], []
        for i in range(o[s], o[s + 1]):
            keep = (m[i] != 0) if m is not None else (k[i] < b[s] if strict else k[i] <= b[s])
            (yes if keep != bool(invert) else no).append(i)
        if partition:
            for j, i in enumerate(yes + no):
                keys_out[o[s] + j], index_out[o[s] + j], written[o[s] + j] = keys[i], i - o[s], True
        else:
            for j, i in enumerate(yes):
                keys_out[total + j], index_out[total + j], written[total + j] = keys[i], i - o[s], True
        total += len(yes)
    koff.append(total)
    return keys_out, index_out, np.array(koff, dtype=np.int64), written


# -- the grid ---------------------------------------------------------------------------------------------------------------------------

def grid(n, cus=256):
    """(tiles, padded table entries, tiles a workgroup walks, scan workgroups a table row) of a call of n elements"""
    tiles = (n + TILE - 1) // TILE
    npad = (tiles + 1 + 15) // 16 * 16
    chunk = (npad + 16 * cus - 1) // (16 * cus)
    return tiles, npad, chunk, (npad // 16 + SCAN_BLOCK - 1) // SCAN_BLOCK


def tile_facts(n, off, keep=None):
    """per tile of the grid: 'dead' (no element of [off[0], off[S])), else the number of segments its live elements belong to; and, with
    the keep flags, the survivors of every tile"""
    o = _offsets(n, off)
    lo, hi = int(o[0]), int(o[-1])
    tiles = (n + TILE - 1) // TILE
    seg = np.full(n, -1, dtype=np.int64)
    seg[lo:hi] = np.repeat(np.arange(o.size - 1), np.diff(o))
    spans, kept = [], []
    for t in range(tiles):
        a, e = max(t * TILE, lo), min((t + 1) * TILE, hi)
        spans.append("dead" if a >= e else int(seg[e - 1] - seg[a]) + 1 if seg[a] != seg[e - 1] else 1)
        if keep is not None:
            kept.append(int(np.count_nonzero(keep[a:e])) if a < e else 0)
    return spans, kept


# -- the layouts of tests/test_gpu_compact.py -------------------------------------------------------------------------------------------------

def offsets_from(lengths, start=0):
    return np.concatenate([[start], start + np.cumsum(lengths)]).astype(np.uint64)


def ragged_layout():
    """(n, off): the issue's lengths, off[0] = 3 and 5 trailing elements"""
    off = offsets_from(LENGTHS, start=3)
    return int(off[-1]) + 5, off


PATTERN_N = 3 * TILE + 17
PATTERNS = ["zeros", "ones", "alternating", "half", "sparse", "last_of_tile", "first_of_tile", "hole"]


def pattern_mask(name, rng):
    """mask bytes over one segment of 3 x 4096 + 17 elements"""
    n = PATTERN_N
    some = lambda k: MASK_BYTES[1:][rng.integers(0, 4, k)]
    m = np.zeros(n, dtype=np.uint8)
    if name == "ones":
        m[:] = some(n)
    elif name == "alternating":
        m[::2] = some((n + 1) // 2)
    elif name == "half":
        m[:] = np.where(rng.integers(0, 2, n) == 1, some(n), 0)
    elif name == "sparse":
        m[:] = np.where(rng.integers(0, 64, n) == 0, some(n), 0)
    elif name == "last_of_tile":
        m[2 * TILE - 1] = 0x80
    elif name == "first_of_tile":
        m[TILE] = 2
    elif name == "hole":
        m[:TILE] = some(TILE)
        m[2 * TILE:3 * TILE] = some(TILE)
        m[3 * TILE:] = some(17)
    return m


BIG_N = (1 << 24) + TILE + 5


def big_layout():
    """(n, off): 2^24 + 4096 + 5 elements; on 256 CUs a workgroup walks two tiles, and segment 1 starts inside the second tile of workgroup 0"""
    return BIG_N, np.array([0, TILE + 1000, BIG_N - 3], dtype=np.uint64)


def empties_layout():
    """(n, off): 5000 empty segments at one position, inside a tile"""
    return 12000, np.concatenate([[0], np.full(5001, 7000), [12000]]).astype(np.uint64)


def mid_tile_layout():
    """(n, off): off[0] and off[S] in the middle of a tile, tiles before and after that hold no live element"""
    return 5 * TILE, np.array([TILE + 1000, TILE + 1000 + 700, 3 * TILE + 50], dtype=np.uint64)


def nothing_layout():
    """(n, off): segments, but no element in range"""
    return 5000, np.array([100, 100, 100], dtype=np.uint64)
