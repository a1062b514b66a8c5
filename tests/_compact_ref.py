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
  compact_tiled    the kernels' own arithmetic tile by tile, with three named slips in what a workgroup carries between tiles
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


def workgroups(n, cus=256):
    """the tiles of every workgroup of compact_write_kernel: [[t, t + 1, ...], ...], `chunk` consecutive tiles each"""
    tiles, _, chunk, _ = grid(n, cus)
    return [list(range(t0, min(t0 + chunk, tiles))) for t0 in range(0, tiles, chunk)]


# -- the kernels' arithmetic, tile by tile -------------------------------------------------------------------------------------------------

FAULTS = ("gallop", "boundary", "stale_stage")
LAST_WAVE = (THREADS - 64) * (TILE // THREADS)          # the tile position of the first element of the workgroup's last wave


def _seg_upper(o, start, x):
    """compact_seg_upper: the first s in [start, S] with off[s] > x, S + 1 if there is none"""
    return start + int(np.searchsorted(o[start:], x, side="right"))


def compact_tiled(keys, off, mask=None, bounds=None, descending=False, strict=False, invert=False, partition=False, cus=256, fault=None):
    """The arithmetic that the top of radix-sort_amd/csrc/rsx_compact.hpp documents, numpy per tile and a plain loop over the tiles:
      count   per workgroup a gallop start carried from tile to tile (`start`, `wstart`); per tile the live range [a, e), the segments of
              a and of e - 1, the segment of every live element between those two, the kept count -> table[tile]; for every off[s] inside
              the tile the kept elements of the tile before it -> koff[s]
      scan    the flat exclusive scan of the table; koff[s] += table[off[s] >> 12]
      write   per tile again: K(i) = table[tile] + rank; compact mode and a partition tile inside one segment stage in LDS by rank and
              leave as one or two runs, a partition tile that spans segments stores per element by the partition formula
    and returns what compact_oracle returns.  With fault=None the two are equal on every layout here (tests/test_compact.py).

    Three named faults, each a slip in what a workgroup carries from tile to tile, to show which layouts would notice:
      "gallop"       a workgroup's second and later tiles start their segment search one segment too far
      "boundary"     an offset equal to a tile's start is counted by the tile before it (all of that tile's kept elements lie before
                     it), while the scanned table entry added to it stays that of its own tile
      "stale_stage"  in a workgroup's second and later tiles the copy-out does not wait for the staging stores of the workgroup's last
                     wave: those slots still hold what the tile before staged there (zeros where it staged nothing)"""
    assert fault is None or fault in FAULTS
    n = keys.size
    o = _offsets(n, off)
    S = o.size - 1
    lo, hi = int(o[0]), int(o[-1])
    tiles, npad, chunk, _ = grid(n, cus)
    k = order_map(keys, descending)
    b = None if bounds is None else order_map(np.asarray(bounds, dtype=keys.dtype), descending)
    m = None if mask is None else np.asarray(mask).view(np.uint8)
    assert (m is None) != (b is None) and not (m is not None and strict)

    def tile(t, start, later):
        """(a, e, segment of every live element, keep flags, the next gallop start), or None for a tile without a live element"""
        a, e = max(t * TILE, lo), min((t + 1) * TILE, hi)
        if a >= e:
            return None
        if fault == "gallop" and later:
            start = min(start + 1, S)                             # (clipped to the last segment: the mirror stays inside the offsets)
        s_first = _seg_upper(o, start, a) - 1
        s_last = _seg_upper(o, s_first + 1, e - 1) - 1
        i = np.arange(a, e, dtype=np.int64)
        seg = s_first + np.maximum(np.searchsorted(o[s_first:s_last + 1], i, side="right") - 1, 0)       # search_segment_of in [s_first, s_last]
        if m is not None:
            keep = m[a:e] != 0
        else:
            keep = (k[a:e] < b[seg]) if strict else (k[a:e] <= b[seg])
        return a, e, seg, (~keep if invert else keep), s_last + 1

    # count
    table = np.zeros(npad, dtype=np.int64)
    koff = np.zeros(S + 1, dtype=np.int64)
    for t0 in range(0, tiles + 1, chunk):
        start = wstart = 0
        for t in range(t0, min(t0 + chunk, tiles + 1)):
            before = np.zeros(TILE + 1, dtype=np.int64)           # kept elements of the tile before tile position x
            got = tile(t, start, t > t0)
            if got is not None:
                a, e, _, keep, start = got
                before[a - t * TILE + 1:e - t * TILE + 1] = np.cumsum(keep)
                before[e - t * TILE + 1:] = before[e - t * TILE]
            table[t] = before[TILE]
            edge = fault == "boundary"                            # (then the tile owns (start, start + 4096], not [start, start + 4096))
            wstart = _seg_upper(o, wstart, t * TILE - (0 if edge else 1)) if t else 0
            s_end = wstart + int(np.searchsorted(o[wstart:], (t + 1) * TILE, side="right" if edge else "left"))
            own = np.arange(wstart, s_end)
            koff[own] = before[o[own] - t * TILE]
    # scan
    scanned = np.concatenate([[0], np.cumsum(table)[:-1]])
    koff += scanned[o >> 12]
    # write
    keys_out, index_out, written = np.zeros(n, dtype=keys.dtype), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)

    def store(d, kk, ii):
        keys_out[d], index_out[d], written[d] = kk, ii, True

    for t0 in range(0, tiles, chunk):
        start = 0
        skey, sidx = np.zeros(TILE, dtype=keys.dtype), np.zeros(TILE, dtype=np.int64)        # the staging area: what the tile before left
        for t in range(t0, min(t0 + chunk, tiles)):
            got = tile(t, start, t > t0)
            if got is None:
                continue
            a, e, seg, keep, start = got
            i = np.arange(a, e, dtype=np.int64)
            rank = np.cumsum(keep) - keep
            total = int(keep.sum())
            tbase = int(scanned[t])
            rel = i - o[seg]
            if not partition or seg[0] == seg[-1]:
                slot = np.where(keep, rank, total + (i - a) - rank)
                put = keep.copy() if not partition else np.ones(e - a, dtype=bool)
                if fault == "stale_stage" and t > t0:
                    put &= i - t * TILE < LAST_WAVE
                skey[slot[put]], sidx[slot[put]] = keys[a:e][put], rel[put]
                count = e - a if partition else total
                r = np.arange(count)
                if partition:
                    s0 = int(seg[0])
                    k0, kept_s = int(koff[s0]), int(koff[s0 + 1] - koff[s0])
                    dk = int(o[s0]) + (tbase - k0)
                    dr = int(o[s0]) + kept_s + (a - int(o[s0])) - (tbase - k0)
                    d = np.where(r < total, dk + r, dr + (r - total))
                else:
                    d = tbase + r
                store(d, skey[:count], sidx[:count])
            else:
                kb = tbase + rank - koff[seg]                     # kept before i in its segment
                kept_s = koff[seg + 1] - koff[seg]
                store(o[seg] + np.where(keep, kb, kept_s + rel - kb), keys[a:e], rel)
    return keys_out, index_out, koff, written


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


def burst(count):
    """`count` short segment lengths cycling through 0, 1, 2, 15, 16, 17, 0, 3 (54 elements a cycle: thread, vector and empty edges)"""
    return [(0, 1, 2, 15, 16, 17, 0, 3)[i % 8] for i in range(count)]


def walk_layout(cus=256):
    """(n, off): 4096 x 16 x CUs + 4096 + 5 elements, so that a workgroup walks two tiles (2w and 2w + 1) on a device of `cus` CUs, and
    1322 segments placed for what a workgroup carries from its first tile to its second (tests/test_compact.py asserts each from the
    layout alone).  With T = 4096:
      off[0] = 3T + 1000        workgroup 0 dead; workgroup 1 = (dead, live inside one segment with a dead front)
      a segment to 4T
      600 short segments        in tile 4, the first of workgroup 2: the gallop of tile 5 starts beyond 600
      a segment to 5T           ends on the edge between the two tiles of workgroup 2
      300 offsets equal to 5T   empty segments exactly at the start of a workgroup's second tile
      400 short segments        more than 256 offsets inside that second tile
      a segment to 6T + 123, one to 9T + 623     workgroup 3 = (spans segments, inside one), workgroup 4 = (inside one, spans segments)
      a segment to (tiles - 24) T + 77           covers whole workgroups
      LENGTHS
      a segment to (tiles - 4) T + 2000          off[S] in the first tile of a workgroup: (live, dead); the next workgroup is dead"""
    T = TILE
    n = T * 16 * cus + T + 5
    tiles = grid(n, cus)[0]
    ends = [4 * T]
    pos = 4 * T
    for L in burst(600):
        pos += L
        ends.append(pos)
    assert pos < 5 * T
    ends += [5 * T] * 301
    pos = 5 * T
    for L in burst(400):
        pos += L
        ends.append(pos)
    assert pos < 6 * T
    ends += [6 * T + 123, 9 * T + 623, (tiles - 24) * T + 77]
    pos = ends[-1]
    for L in LENGTHS:
        pos += L
        ends.append(pos)
    assert pos < (tiles - 4) * T
    ends.append((tiles - 4) * T + 2000)
    return n, np.array([3 * T + 1000] + ends, dtype=np.uint64)


def nothing_layout():
    """(n, off): segments, but no element in range"""
    return 5000, np.array([100, 100, 100], dtype=np.uint64)
