"""Host referee of the unique tests (rsx_segmented_unique), per segment, on the unsigned image of the key under the engine's order map (enc of
tests/test_gpu_float_keys.py, complemented for descending engines: the map _topk_ref / _select_ref use), in two forms.

unique_oracle   the numpy form: np.unique(image, return_index, return_inverse, return_counts) per segment in sorted mode (numpy's
                return_index is the FIRST occurrence), a != on neighbours in consecutive mode.
slow_unique     the same answer from a dict / a loop over the elements, to check the fast form against.
flat_unique     the same answer from ONE stable sort of (segment id, image) over [off[0], off[S]): for millions of segments.  Its dict also
                holds "order" (the original position of every grouped element, off[0] first) and "heads" (the grouped positions that
                begin a run, as positions on the global grid): what tests/_reduce_ref.py reduces over.
All return a dict: keys (packed distinct keys, unsigned words of the INPUT bits), run_offsets (S + 1 uint64), counts, first (uint32,
packed like keys), inverse (uint32, n entries) and written (bool, n entries: the positions of inverse the call writes, i.e. [off[0], off[S])).
off None = one segment [0, n).

The tile grid of the grouping chain (unique_groups_enqueue in capi_unique.inc) is mirrored by tile_grid, and the layouts of
tests/test_gpu_unique_reduce_paths.py are held here with fixed seeds; tests/test_unique.py checks that each still reaches its path.
"""
import numpy as np

from test_gpu_float_keys import UINT, enc


def _image(x, descending):
    e = enc(x)
    return ~e if descending else e


def _offsets(off, n):
    return np.array([0, n], dtype=np.int64) if off is None else np.asarray(off, dtype=np.int64)


def _pack(x, off, parts):
    n = x.size
    u = UINT[x.dtype]
    nseg = len(off) - 1
    keys, counts, first = [], [], []
    inverse = np.zeros(n, dtype=np.uint32)
    written = np.zeros(n, dtype=bool)
    uoff = np.zeros(nseg + 1, dtype=np.uint64)
    for s, (k, c, f, inv) in enumerate(parts):
        a, b = int(off[s]), int(off[s + 1])
        keys.append(k)
        counts.append(c)
        first.append(f)
        inverse[a:b] = inv
        written[a:b] = True
        uoff[s + 1] = uoff[s] + np.uint64(len(k))
    cat = lambda parts_, dt: np.concatenate(parts_).astype(dt) if parts_ else np.zeros(0, dtype=dt)
    return {"keys": cat(keys, u), "run_offsets": uoff, "counts": cat(counts, np.uint32), "first": cat(first, np.uint32), "inverse": inverse,
            "written": written}


def unique_oracle(x: np.ndarray, off=None, descending: bool = False, consecutive: bool = False):
    n = x.size
    off = _offsets(off, n)
    xu = x.view(UINT[x.dtype])
    img = _image(x, descending)
    parts = []
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        assert 0 <= a <= b <= n, "the referee takes valid offsets only"
        seg = img[a:b]
        if consecutive:
            head = np.ones(b - a, dtype=bool)
            head[1:] = seg[1:] != seg[:-1]
            f = np.flatnonzero(head)
            c = np.diff(np.append(f, b - a))
            inv = np.cumsum(head) - 1
        else:
            _, f, inv, c = np.unique(seg, return_index=True, return_inverse=True, return_counts=True)
            inv = inv.reshape(-1)
        parts.append((xu[a:b][f], c, f, inv))
    return _pack(x, off, parts)


def slow_unique(x: np.ndarray, off=None, descending: bool = False, consecutive: bool = False):
    n = x.size
    off = _offsets(off, n)
    xu = x.view(UINT[x.dtype])
    img = _image(x, descending).tolist()
    parts = []
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        runs = []                                   # [image, first position, count]
        inv = []
        if consecutive:
            for i in range(a, b):
                if i == a or img[i] != img[i - 1]:
                    runs.append([img[i], i - a, 0])
                runs[-1][2] += 1
                inv.append(len(runs) - 1)
        else:
            seen = {}
            for i in range(a, b):
                r = seen.get(img[i])
                if r is None:
                    r = seen[img[i]] = [img[i], i - a, 0]
                r[2] += 1
            runs = sorted(seen.values())
            rank = {r[0]: j for j, r in enumerate(runs)}
            inv = [rank[img[i]] for i in range(a, b)]
        f = np.array([r[1] for r in runs], dtype=np.int64)
        parts.append((xu[a:b][f] if len(runs) else xu[:0], np.array([r[2] for r in runs], dtype=np.int64), f, np.array(inv, dtype=np.int64)))
    return _pack(x, off, parts)


FIELDS = ("keys", "run_offsets", "counts", "first", "inverse", "written")


def same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in FIELDS)


def flat_unique(x: np.ndarray, off=None, descending: bool = False, consecutive: bool = False):
    n = x.size
    off = _offsets(off, n)
    lens = np.diff(off)
    assert off[0] >= 0 and off[-1] <= n and (lens >= 0).all(), "the referee takes valid offsets only"
    nseg = len(lens)
    lo, hi = int(off[0]), int(off[-1])
    m = hi - lo
    u = UINT[x.dtype]
    img = _image(x, descending)[lo:hi]
    seg = np.repeat(np.arange(nseg, dtype=np.int64), lens)
    if consecutive:
        order = np.arange(m, dtype=np.int64)
    elif img.dtype.itemsize == 4:
        # (segment, image) in one 64-bit word: the segment ids are non-decreasing already, a stable sort keeps equal keys in place
        order = np.argsort((seg.astype(np.uint64) << np.uint64(32)) | img.astype(np.uint64), kind="stable")
    else:
        order = np.lexsort((img, seg))
    simg = img[order]
    head = np.zeros(m, dtype=bool)
    head[(off[:-1] - lo)[lens > 0]] = True                      # the start of every non-empty segment
    head[1:] |= simg[1:] != simg[:-1]
    hp = np.flatnonzero(head)
    gid = np.cumsum(head) - 1
    uoff = np.searchsorted(hp, off - lo).astype(np.uint64)      # heads before off[s]
    inverse = np.zeros(n, dtype=np.uint32)
    inverse[lo + order] = (gid - uoff[seg].astype(np.int64)).astype(np.uint32)
    written = np.zeros(n, dtype=bool)
    written[lo:hi] = True
    # a stable sort leaves the first occurrence at the head of its run
    first = order[hp] - (off[:-1] - lo)[seg[hp]]
    return {"keys": x.view(u)[lo:hi][order[hp]].astype(u), "run_offsets": uoff, "counts": np.diff(np.append(hp, m)).astype(np.uint32),
            "first": first.astype(np.uint32), "inverse": inverse, "written": written, "order": order + lo, "heads": hp + lo}


# -- the tile grid and the layouts of tests/test_gpu_unique_reduce_paths.py --------------------------------------------------------------

TILE = 4096          # rsx::kUniqTileKeys
CUS = 256            # MI355X compute units: the engine's cus when it asks the device
SMALL = [0, 1, 2, 255, 256, 257, 1024, 1025, 4096, 4097, 9000, 0, 3, 20011]          # LENGTHS of tests/test_gpu_unique.py


def tile_grid(n: int, cus: int = CUS, tile: int = TILE) -> dict:
    """unique_groups_enqueue's launch shape: workgroup b walks the tiles [b * chunk, (b + 1) * chunk) of a table of ntiles + 1 entries
    padded to a multiple of 16"""
    ntiles = (n + tile - 1) // tile
    npad = (ntiles + 1 + 15) // 16 * 16
    chunk = (npad + cus * 16 - 1) // (cus * 16)
    return {"ntiles": ntiles, "npad": npad, "chunk": chunk, "tgrid": (npad + chunk - 1) // chunk}


def offsets_per_tile(off, n: int, tile: int = TILE) -> np.ndarray:
    """how many off[s] (s = 0 .. S) fall into every tile of the table (the extra tile at n included)"""
    return np.bincount(np.asarray(off, dtype=np.int64) // tile, minlength=(n + tile - 1) // tile + 1)


def run_keys(n: int, rng, tile: int = TILE) -> np.ndarray:
    """keys from an alphabet of four in runs of 1 .. 3 tiles: runs cross tiles and segment borders, and sorted segments repeat keys"""
    lens = rng.choice([1, 2, 3, 17, tile // 13, tile + 5, 3 * tile + 1], size=n // 3 + 16, p=[0.3, 0.2, 0.2, 0.2, 0.06, 0.03, 0.01])
    lens = lens[:int(np.searchsorted(np.cumsum(lens), n)) + 1]
    assert int(lens.sum()) >= n
    return np.repeat(rng.integers(0, 4, lens.size), lens)[:n].astype(np.uint32)


def ragged_layout(chunk: int, tile: int = TILE, cus: int = CUS, seed: int = 0, wg: int = 40, long_tiles: int = 70):
    """n just above the first size whose workgroups walk `chunk` tiles; long segments (several tiles), SMALL ones, empty ones, segment
    ends on and one off tile edges, off[0] = 5 and a tail after off[S].  One run of `long_tiles` tiles and a bit begins mid-tile in the last
    tile of workgroup `wg`'s range.  Returns (n, off, keys, (start, length) of that run)."""
    rng = np.random.default_rng(1000 + seed + chunk)
    n = ((chunk - 1) * cus * 16 + 3) * tile + 77                 # 2^24 and 2^25 and a bit on 256 CUs and 4096-key tiles
    assert tile_grid(n, cus, tile)["chunk"] == chunk
    start = (wg * chunk + chunk - 1) * tile + tile // 4          # mid-tile, in the last tile of workgroup wg
    length = long_tiles * tile + 123 * tile // TILE
    small = [v * tile // TILE if v > 3 else v for v in SMALL]
    lens = []
    pos = 5

    def fill(upto):
        nonlocal pos
        while pos < upto:
            kind = rng.integers(0, 6)
            if kind == 0:
                step = [int(rng.integers(2, 9)) * tile + int(rng.integers(0, tile))]
            elif kind == 1:
                step = [tile - pos % tile, 0, 0, tile, 1, tile - 1, tile + 1, tile - 2]      # ends on and one off tile edges
            elif kind == 2:
                step = [0] * int(rng.integers(1, 5))
            else:
                step = [small[i] for i in rng.permutation(len(small))[:int(rng.integers(1, len(small)))]]
            for v in step:
                v = min(int(v), upto - pos)
                lens.append(v)
                pos += v

    fill(start - tile // 8)
    lens.append(start - tile // 8 + length + tile // 2 - pos)    # one segment around the long run
    pos += lens[-1]
    fill(n - 2 * tile - 9)
    off = np.concatenate([[5], 5 + np.cumsum(lens)]).astype(np.uint64)
    keys = run_keys(n, rng, tile)
    keys[start - tile // 8:start] = 9
    keys[start:start + length] = 8
    keys[start + length:start + length + tile // 2] = 9
    return n, off, keys, (start, length)


def dense_layout(kind: str, tile: int = TILE, cus: int = CUS, seed: int = 0):
    """segments of 1 .. 3 keys all over, three blocks of 1000 empty segments: mid-tile, on a tile edge, at off[S].
    kind "ragged": n = 1024 tiles + 1234 keys, off[0] = 3, off[S] = n - 77.  "aligned": n = 1024 tiles, off[0] = 0, off[S] = n (the
    block sits in the table's extra entry).  "chunk2": the ragged form at the first size whose workgroups walk two tiles.
    Returns (n, off, keys)."""
    rng = np.random.default_rng(2000 + seed + ["ragged", "aligned", "chunk2"].index(kind))
    tiles = 1024 if kind != "chunk2" else cus * 16
    n = tiles * tile + (0 if kind == "aligned" else 1234 * tile // TILE)
    lo, hi = (0, n) if kind == "aligned" else (3, n - 77 * tile // TILE)
    lens = rng.integers(1, 4, (hi - lo) // 2 + (hi - lo) // 50 + 64)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), hi - lo)) + 1]
    ends = lo + np.cumsum(lens)
    ends[-1] = hi
    empties = np.zeros(1000, dtype=np.int64)
    a = int(np.searchsorted(ends, tiles * 3 // 10 * tile + tile // 3))
    b = int(np.searchsorted(ends, tiles * 7 // 10 * tile))
    ends[b] = tiles * 7 // 10 * tile                                         # a segment end exactly on a tile edge: the block sits on it
    off = np.concatenate([[lo], ends[:a + 1], ends[a] + empties, ends[a + 1:b + 1], ends[b] + empties, ends[b + 1:], hi + empties])
    assert (np.diff(off) >= 0).all() and (np.diff(off) <= 5).all()
    keys = rng.integers(0, 3, n).astype(np.uint32)
    return n, off.astype(np.uint64), keys


def deep_layout(kind: str, tile: int = TILE, seed: int = 0):
    """off[0] in the fourth tile or later and off[S] three tiles or more before n, on 40 tiles and a bit.  kind "mid": off[0] and off[S]
    mid-tile; "edge": both on tile edges; "none": off[0] == off[S] mid-tile, no run at all; "none_edge": the same on an edge.
    Returns (n, off, keys)."""
    rng = np.random.default_rng(3000 + seed + ["mid", "edge", "none", "none_edge"].index(kind))
    n = 40 * tile + 100
    lo, hi = {"mid": (3 * tile + 777 * tile // TILE, n - 3 * tile - 50), "edge": (5 * tile, 36 * tile), "none": (6 * tile + 5, 6 * tile + 5),
              "none_edge": (7 * tile, 7 * tile)}[kind]
    small = [v * tile // TILE if v > 3 else v for v in SMALL]
    lens = []
    while sum(lens) < hi - lo:
        lens += [small[i] for i in rng.permutation(len(small))] + [int(rng.integers(1, 4)) * tile]
    ends = np.minimum(lo + np.cumsum(lens), hi) if hi > lo else np.full(7, lo)
    off = np.concatenate([[lo], ends]).astype(np.uint64)
    keys = run_keys(n, rng, tile)
    keys[:lo] = keys[lo]                                         # a key read from outside the range would lengthen a run
    keys[hi:] = keys[hi - 1]
    return n, off, keys
