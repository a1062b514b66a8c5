"""Host referee of rsx_segmented_expand: owners, ranks and values from numpy and plain loops, the named layouts the GPU tests run, and for
every layout a path proof: which path of expand_tile_kernel (rsx_expand.hpp) each tile of the absolute 4096-position grid takes, derived
from the offsets alone.  Nothing in here touches the library."""
import numpy as np

TILE = 4096
THREADS = 256
WALK = 4 * THREADS          # offsets per trip of the walk: four loads in flight per thread
NONE, FILL, GENERAL = "none", "fill", "general"


def offsets_from(lengths, start=0):
    return np.concatenate([[start], start + np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uint64)


def valid(off, n, starts=None, num_values=None):
    """the index of the first bad segment, or None: off[s+1] < off[s] or off[s+1] > n; in gather form starts[s] + len > num_values"""
    o = [int(x) for x in off]
    for s in range(len(o) - 1):
        if o[s + 1] < o[s] or o[s + 1] > n:
            return s
        if starts is not None and int(starts[s]) + o[s + 1] - o[s] > num_values:
            return s
    return None


def owners(off):
    """(segment, rank) of every position of [off[0], off[S]), via np.repeat: position off[0] + j is row j"""
    o = np.asarray(off).astype(np.int64)
    lens = np.diff(o)
    seg = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    rank = np.arange(int(o[0]), int(o[-1]), dtype=np.int64) - o[:-1][seg] if len(lens) else np.zeros(0, dtype=np.int64)
    return seg, rank


def owners_searchsorted(off):
    """the same through the owner rule itself: the largest s with off[s] <= i"""
    o = np.asarray(off).astype(np.int64)
    pos = np.arange(int(o[0]), int(o[-1]), dtype=np.int64)
    seg = np.searchsorted(o, pos, side="right") - 1
    return seg, pos - o[seg]


def owners_brute(off):
    """plain loops, for small cases"""
    o = [int(x) for x in off]
    seg, rank = [], []
    for i in range(o[0], o[-1]):
        s = max(k for k in range(len(o)) if o[k] <= i)
        assert s < len(o) - 1
        seg.append(s)
        rank.append(i - o[s])
    return np.array(seg, dtype=np.int64), np.array(rank, dtype=np.int64)


def expand_oracle(off, n, values=None, starts=None, sentinel=None):
    """What a call leaves in buffers of n elements that held `sentinel` words: (values or None, segment uint32, rank uint32, written bool).
    values: one per segment (fill form) or the source of the ranged gather (starts given)."""
    o = np.asarray(off).astype(np.int64)
    seg, rank = owners(off)
    lo, hi = int(o[0]), int(o[-1])
    written = np.zeros(n, dtype=bool)
    written[lo:hi] = True
    sout = np.full(n, 0xC3C3C3C3 if sentinel is None else sentinel, dtype=np.uint32)
    rout = sout.copy()
    sout[lo:hi] = seg
    rout[lo:hi] = rank
    vout = None
    if values is not None:
        vout = np.frombuffer(bytes([0xC3]) * (n * values.dtype.itemsize), dtype=values.dtype).copy()
        src = seg if starts is None else np.asarray(starts).astype(np.int64)[seg] + rank
        vout[lo:hi] = values[src]
    return vout, sout, rout, written


# -- the kernel's paths, from the offsets alone -----------------------------------------------------------------------------------------------

def tile_paths(off, n):
    """per tile of the absolute grid over [0, n): (path, starts inside the tile, trips of the offsets walk).  NONE: nothing of
    [off[0], off[S]) in the tile; FILL: no offset inside the tile; GENERAL: the LDS marks and the max-scan."""
    o = np.asarray(off).astype(np.int64)
    lo, hi = int(o[0]), int(o[-1])
    res = []
    for t in range((n + TILE - 1) // TILE):
        ts, te = t * TILE, (t + 1) * TILE
        if max(ts, lo) >= min(te, hi):
            res.append((NONE, 0, 0))
            continue
        s_lo, s_hi = int(np.searchsorted(o, ts, side="left")), int(np.searchsorted(o, te, side="left"))
        k = s_hi - s_lo
        res.append((FILL, 0, 0) if k == 0 else (GENERAL, k, (k + WALK - 1) // WALK))
    return res


def tiles_per_workgroup(n, cus=256):
    ntiles = (n + TILE - 1) // TILE
    return (ntiles + cus * 16 - 1) // (cus * 16)


def paths(off, n, cus=256):
    """the set of named paths a layout reaches"""
    tp = tile_paths(off, n)
    o = np.asarray(off).astype(np.int64)
    lo, hi = int(o[0]), int(o[-1])
    got = set()
    for t, (p, k, steps) in enumerate(tp):
        got.add(p)
        if p == GENERAL:
            if k == TILE:
                got.add("4096 starts in a tile")
            if k > TILE:
                got.add("more offsets than slots")
            if steps > 1:
                got.add("the walk loops")
            if np.any(o % TILE == 0) and np.any((o // TILE == t) & (o % TILE == 0)):
                got.add("start on a tile edge")
        if p != NONE and (lo > t * TILE or hi < (t + 1) * TILE):
            got.add("ragged end inside a tile")
    if len(o) > 1 and np.any(np.diff(o) == 0):
        got.add("empty segments")
    if tiles_per_workgroup(n, cus) > 1:
        got.add("several tiles per workgroup")
    if lo > 0:
        got.add("untouched prefix")
    if hi < n:
        got.add("untouched suffix")
    return got


# -- the named layouts: (n, offsets) --------------------------------------------------------------------------------------------------------

def layout_one(length):
    return length, np.array([0, length], dtype=np.uint64)


def layout_all_ones(n=2 * TILE + 3):
    return n, np.arange(n + 1, dtype=np.uint64)


def layout_alternating(n=TILE + 77):
    return n, offsets_from([k & 1 for k in range(2 * n)])


def layout_edges(empties, tiles=3, tail=5):
    """segments that start exactly at 4096 * k, with `empties` empty segments sharing each such offset"""
    lens = []
    for _ in range(tiles):
        lens += [0] * empties + [TILE]
    lens += [0] * empties + [tail]
    off = offsets_from(lens)
    return int(off[-1]), off


def layout_empties(where, count=9):
    """`count` empty segments first, last, or nothing else at all"""
    body = [5, TILE, 1, 300]
    lens = {"first": [0] * count + body, "last": body + [0] * count, "all": [0] * count}[where]
    off = offsets_from(lens, start=0 if where != "all" else 17)
    return max(int(off[-1]), 17) + (0 if where != "all" else 100), off


def layout_dense_empties(count=TILE + 300):
    """two elements with `count` empty segments between them, inside one tile: more offsets than slots, the walk loops"""
    off = offsets_from([1] + [0] * count + [1], start=7)
    return 100, off


def layout_ragged_ends():
    n = 2 * TILE + 11
    return n, offsets_from([1, 0, 4000, 300, 0, 0, n - 8 - 4301], start=5)


def layout_zipf(total=1 << 18, seed=5):
    rng = np.random.default_rng(seed)
    lens = []
    left = total
    while left > 0:
        k = int(min(rng.zipf(1.3), 20000, left))
        lens.append(k)
        left -= k
        if rng.integers(0, 4) == 0:
            lens += [0] * int(rng.integers(1, 4))
    off = offsets_from(lens, start=3)
    return int(off[-1]) + 2, off


def layout_multi_tile(nseg=4099):
    """2^24 + 4099 elements in 4099 segments: 4098 tiles, two per workgroup on 256 CUs"""
    n = (1 << 24) + 4099
    lens = np.full(nseg, n // nseg, dtype=np.int64)
    lens[: n - int(lens.sum())] += 1
    return n, offsets_from(lens)


def layout_many_segments(nseg=(1 << 20) + 4099, seed=9):
    """mostly empty: every 64th segment has elements"""
    rng = np.random.default_rng(seed)
    lens = np.zeros(nseg, dtype=np.int64)
    live = np.arange(0, nseg, 64)
    lens[live] = rng.integers(1, 40, live.size)
    off = offsets_from(lens)
    return int(off[-1]), off


LAYOUTS = {
    "one of 1": (lambda: layout_one(1), {GENERAL}),                           # (off[0] = 0 is a start inside tile 0)
    "one of 4095": (lambda: layout_one(TILE - 1), {GENERAL}),
    "one of 4096": (lambda: layout_one(TILE), {GENERAL}),
    "one of 4097": (lambda: layout_one(TILE + 1), {GENERAL, "ragged end inside a tile"}),
    "one of 3 tiles + 5": (lambda: layout_one(3 * TILE + 5), {GENERAL, FILL}),
    "all ones": (layout_all_ones, {GENERAL, "4096 starts in a tile", "the walk loops"}),
    "alternating 0 and 1": (layout_alternating, {GENERAL, "empty segments", "more offsets than slots"}),
    "edges, 0 empty": (lambda: layout_edges(0), {GENERAL, "start on a tile edge"}),
    "edges, 1 empty": (lambda: layout_edges(1), {GENERAL, "start on a tile edge", "empty segments"}),
    "edges, 7 empty": (lambda: layout_edges(7), {GENERAL, "start on a tile edge", "empty segments"}),
    "empties first": (lambda: layout_empties("first"), {GENERAL, "empty segments"}),
    "empties last": (lambda: layout_empties("last"), {GENERAL, "empty segments"}),
    "all empty": (lambda: layout_empties("all"), {NONE, "empty segments"}),
    "dense empties": (layout_dense_empties, {GENERAL, "more offsets than slots", "the walk loops", "empty segments"}),
    "ragged ends": (layout_ragged_ends, {GENERAL, "ragged end inside a tile", "untouched prefix", "untouched suffix", "empty segments"}),
    "zipf": (layout_zipf, {GENERAL, FILL, "empty segments", "untouched prefix", "untouched suffix"}),
}
BIG_LAYOUTS = {
    "multi tile": (layout_multi_tile, {GENERAL, "several tiles per workgroup"}),
    "many segments": (layout_many_segments, {GENERAL, "empty segments", "more offsets than slots", "the walk loops"}),
}
