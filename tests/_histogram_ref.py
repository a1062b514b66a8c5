"""Host referee of rsx_segmented_histogram (no GPU, no library): the bin of every key in a vectorised and in an element-by-element form,
the S x B counters, and — from the layout alone — the path every piece of every tile takes in radix-sort_amd/csrc/rsx_bins.hpp.

Bins are numbered in the engine's order.  Edges form: with j = the number of edges that do not come after key k in that order (the
RSX_SEARCH_RIGHT position of _search_ref), bin j - 1 for 1 <= j <= B, bin B - 1 for j == B + 1 when k has the bits of edges[B], dropped
otherwise.  Even form, integers: bin (k - lo) >> shift on the ascending-mapped words, dropped before lo and from bin B on.  Even form,
floats: bin min(B - 1, floor((x - lo) * scale)) for lo <= x <= hi by IEEE comparison, scale = dtype(B) / (hi - lo), every operation in
the key's dtype and rounded once.  A descending engine numbers the even forms' bins backwards.

  bins_of            vectorised (numpy searchsorted / numpy arithmetic in the key's dtype); NO_BIN for a dropped key
  bins_loop          one key at a time, with Python integers and a linear walk of the edges
  histogram_oracle   S x B counts from bins_of; histogram_loop the same from bins_loop
  piece_paths        [(tile, segment, length, path)] for a layout; piece_slots adds the LDS slot a piece gets in a tile of several pieces
The cases of the bin arithmetic (edges_cases, even_int_cases, even_float_cases) are drawn here once for the CPU selftest and the GPU tests.
"""
import numpy as np

from _search_ref import UINT, order_map, order_unmap

NO_BIN = 0xFFFFFFFF
TILE = 4096
LDS_MAX = 4096               # kBinsLdsMax
WAVE_PRIVATE_MAX = 1024      # kBinsWavePrivateMax
DIRECT_PIECE = 256           # kBinsDirectPiece
DTYPES = ["uint32", "int32", "uint64", "int64", "float32", "float64"]


def _offsets(n, off):
    return np.array([0, n], dtype=np.int64) if off is None else np.asarray(off).astype(np.int64)


def bins_of(keys, bins, lo=0, hi=0, shift=0, descending=False) -> np.ndarray:
    """the bin of every key of the array (int64; NO_BIN: dropped).  bins: an int (even form) or the array of B + 1 edges."""
    keys = np.ascontiguousarray(keys)
    dt = keys.dtype
    if not np.isscalar(bins):
        edges = np.ascontiguousarray(bins, dtype=dt)
        B = edges.size - 1
        k, e = order_map(keys, descending), order_map(edges, descending)
        j = np.searchsorted(e, k, side="right").astype(np.int64)
        out = np.where((j >= 1) & (j <= B), j - 1, NO_BIN)
        return np.where((j == B + 1) & (k == e[B]), B - 1, out).astype(np.int64)
    B = int(bins)
    if dt.kind == "f":
        lo_, hi_ = dt.type(lo), dt.type(hi)
        scale = dt.type(dt.type(B) / dt.type(hi_ - lo_))
        with np.errstate(invalid="ignore", over="ignore"):
            inside = (lo_ <= keys) & (keys <= hi_)
            t = ((np.where(inside, keys, lo_) - lo_).astype(dt) * scale).astype(dt)
        b = np.where(t >= dt.type(B - 1), B - 1, np.minimum(t, dt.type(B)).astype(np.int64))
    else:
        u = UINT[dt.itemsize]
        k, l = order_map(keys), order_map(np.array([lo], dtype=dt))[0]
        d = (k - l).astype(u) >> u(shift)          # (wraps below lo: masked next)
        inside = (k >= l) & (d < u(min(B, int(np.iinfo(u).max))))
        b = np.where(inside, d, 0).astype(np.int64)
    b = (B - 1 - b) if descending else b
    return np.where(inside, b, NO_BIN).astype(np.int64)


def bins_loop(keys, bins, lo=0, hi=0, shift=0, descending=False) -> list:
    """bins_of, key by key"""
    keys = np.ascontiguousarray(keys)
    dt = keys.dtype
    out = []
    if not np.isscalar(bins):
        e = [int(v) for v in order_map(np.ascontiguousarray(bins, dtype=dt), descending)]
        B = len(e) - 1
        for k in (int(v) for v in order_map(keys, descending)):
            j = 0
            while j <= B and e[j] <= k:         # (sorted edges: the first edge after k)
                j += 1
            out.append(j - 1 if 1 <= j <= B else B - 1 if j == B + 1 and k == e[B] else NO_BIN)
        return out
    B = int(bins)
    if dt.kind == "f":
        lo_, hi_ = dt.type(lo), dt.type(hi)
        scale = dt.type(dt.type(B) / dt.type(hi_ - lo_))
        for x in keys:
            if not (lo_ <= x <= hi_):
                out.append(NO_BIN)
                continue
            t = dt.type(dt.type(x - lo_) * scale)
            b = min(B - 1, int(np.floor(t)))
            out.append(B - 1 - b if descending else b)
        return out
    l = int(order_map(np.array([lo], dtype=dt))[0])
    for k in (int(v) for v in order_map(keys)):
        b = (k - l) >> shift if k >= l else B
        out.append(NO_BIN if b >= B else B - 1 - b if descending else b)
    return out


def _count(bins_per_key, n, off, B):
    o = _offsets(n, off)
    S = o.size - 1
    b = np.asarray(bins_per_key, dtype=np.int64)
    seg = np.repeat(np.arange(S, dtype=np.int64), np.diff(o))
    live = b[o[0]:o[-1]]
    ok = live != NO_BIN
    return np.bincount(seg[ok] * B + live[ok], minlength=S * B).reshape(S, B).astype(np.int64)


def histogram_oracle(keys, off, bins, lo=0, hi=0, shift=0, descending=False) -> np.ndarray:
    B = int(bins) if np.isscalar(bins) else len(bins) - 1
    return _count(bins_of(keys, bins, lo, hi, shift, descending), keys.size, off, B)


def histogram_loop(keys, off, bins, lo=0, hi=0, shift=0, descending=False) -> np.ndarray:
    B = int(bins) if np.isscalar(bins) else len(bins) - 1
    o = [int(v) for v in _offsets(keys.size, off)]
    b = bins_loop(keys, bins, lo, hi, shift, descending)
    counts = np.zeros((len(o) - 1, B), dtype=np.int64)
    for s in range(len(o) - 1):
        for i in range(o[s], o[s + 1]):
            if b[i] != NO_BIN:
                counts[s, b[i]] += 1
    return counts


# -- the paths --------------------------------------------------------------------------------------------------------------------------

def chunk_of(n, cus=256):
    """tiles a workgroup walks"""
    tiles = (n + TILE - 1) // TILE
    return max((tiles + 16 * cus - 1) // (16 * cus), 1)


def piece_paths(n, off, B, cus=256):
    """[(tile, segment, length, path)] of every piece (a non-empty segment cut to a tile) in the order the kernel meets them.  path:
    'direct'      B > LDS_MAX or fewer than DIRECT_PIECE keys: one global add per key
    'lds_first'   counted in LDS; the workgroup's counters were empty
    'lds_same'    counted in LDS on top of the same segment's counts from an earlier tile of the workgroup: no flush in between
    'lds_flush'   counted in LDS after the counters of ANOTHER segment were flushed: a flush at a segment boundary"""
    o = _offsets(n, off)
    chunk = chunk_of(n, cus)
    out = []
    acc, acc_group = None, None
    starts, ends = o[:-1], o[1:]
    for t in range((n + TILE - 1) // TILE):
        group = t // chunk
        if group != acc_group:
            acc, acc_group = None, group
        t0, t1 = t * TILE, (t + 1) * TILE
        first = int(np.searchsorted(ends, t0, side="right"))
        last = int(np.searchsorted(starts, t1, side="left"))
        for s in range(first, last):
            a, e = max(int(starts[s]), t0), min(int(ends[s]), t1)
            if a >= e:
                continue
            if B > LDS_MAX or e - a < DIRECT_PIECE:
                out.append((t, s, e - a, "direct"))
                continue
            out.append((t, s, e - a, "lds_first" if acc is None else "lds_same" if acc == s else "lds_flush"))
            acc = s
    return out


def piece_slots(n, off, B, cus=256):
    """[(tile, segment, length, path, slot)]: piece_paths with the slot of sh.piece_seg that an LDS piece is numbered by, (piece start -
    tile start) >> 8, in a tile of several pieces; None for a direct piece and for the one piece of a tile inside one segment (that
    branch has no slots)"""
    paths = piece_paths(n, off, B, cus)
    o = _offsets(n, off)
    per_tile = np.bincount([p[0] for p in paths], minlength=1)
    out = []
    for t, s, L, path in paths:
        start = max(int(o[s]), t * TILE)
        out.append((t, s, L, path, None if path == "direct" or per_tile[t] == 1 else (start - t * TILE) // DIRECT_PIECE))
    return out


def lds_layout(B):
    """'wave_private' or 'shared' or 'none': the counters of the LDS path for B bins"""
    return "none" if B > LDS_MAX else "wave_private" if B <= WAVE_PRIVATE_MAX else "shared"


# -- inputs -----------------------------------------------------------------------------------------------------------------------------

def random_keys(rng, dtype, n, span=None):
    """n keys of the dtype; integers in [-span, span) (unsigned: [0, 2 span)), floats normal * span / 4; span None: the whole type"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.standard_normal(n) * ((span or 1000.0) / 4)).astype(dt)
    if span is None:
        return rng.integers(0, 1 << (8 * dt.itemsize), n, dtype=UINT[dt.itemsize]).view(dt)
    lo = -span if dt.kind == "i" else 0
    return rng.integers(lo, lo + 2 * span, n, dtype=np.int64).astype(dt)


def sorted_edges(rng, dtype, B, span, descending=False):
    """B + 1 distinct edges inside the keys' range, sorted in the engine's order"""
    dt = np.dtype(dtype)
    e = np.array([], dtype=dt)
    while np.unique(e.view(UINT[dt.itemsize])).size < B + 1:
        e = np.concatenate([e, random_keys(rng, dt, 2 * (B + 1), span)])
        e = e.view(UINT[dt.itemsize])
        e = e[np.sort(np.unique(e, return_index=True)[1])].view(dt)
    e = e[:B + 1]
    return e[np.argsort(order_map(e, descending), kind="stable")]


# -- the cases and layouts of the GPU tests (tests/test_histogram.py checks from them alone that each reaches its path) ---------------------

SPAN = 4000                                       # integer keys in [-4000, 4000) / [0, 8000), floats about normal * 1000
MATRIX_BINS = [1, 2, 64, 257, 4096]
EVEN_SHIFT = {1: 5, 2: 5, 64: 3, 257: 1, 4096: 0}   # integer even form: B << shift values from lo on
FLOAT_LO, FLOAT_HI = -1024.0, 1536.0


def special_floats(dt):
    """NaNs of both signs, +-0, +-inf"""
    dt = np.dtype(dt)
    return np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf], dtype=dt)


def scatter_into(rng, keys, off, values):
    """`values` written over random distinct positions inside [off[0], off[S]) (all of them when there is room)"""
    o = _offsets(keys.size, off)
    lo, hi = int(o[0]), int(o[-1])
    count = min(len(values), hi - lo)
    pos = lo + rng.permutation(hi - lo)[:count]
    keys[pos] = values[:count]
    return keys


def form_args(dt, form, descending, B, rng):
    """the arguments of one call: dict(bins=, lo=, hi=, shift=) for the referee and the GPU harness alike"""
    dt = np.dtype(dt)
    if form == "edges":
        return dict(bins=sorted_edges(rng, dt, B, SPAN * 3 // 4, descending), lo=0, hi=0, shift=0)      # (narrower than the keys: some fall outside)
    if dt.kind == "f":
        return dict(bins=B, lo=FLOAT_LO, hi=FLOAT_HI, shift=0)
    return dict(bins=B, lo=-300 if dt.kind == "i" else 3700, hi=0, shift=EVEN_SHIFT.get(B, 0))


def case_keys(rng, dt, n, off, args):
    """random keys (also outside the segments) with, inside the segments, every edge or lo and hi themselves and, for floats, the specials"""
    dt = np.dtype(dt)
    keys = random_keys(rng, dt, n, SPAN)
    ties = np.asarray(args["bins"], dtype=dt) if not np.isscalar(args["bins"]) else np.array([args["lo"], args["hi"] if dt.kind == "f" else args["lo"] - 1], dtype=dt)
    extra = np.concatenate([ties, special_floats(dt)]) if dt.kind == "f" else ties
    return scatter_into(rng, keys, off, extra)


def offsets_from(lengths, start=0):
    return np.concatenate([[start], start + np.cumsum(lengths)]).astype(np.uint64)


LENGTHS = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 9000, 0, 3, 20011]       # test_search.LENGTHS
BIG_N = (1 << 24) + TILE + 5                       # _compact_ref.BIG_N: a workgroup walks two tiles on 256 CUs
SKEW_N = 3 * TILE + 17


def ragged_layout():
    """(n, off): test_search.LENGTHS from off[0] = 3, 5 trailing elements"""
    off = offsets_from(LENGTHS, start=3)
    return int(off[-1]) + 5, off


def big_boundaries_layout():
    """(n, off): BIG_N elements; off[0] and off[S] in mid-tile, and boundaries in the middle of a workgroup's SECOND tile (tile 3: both
    pieces long), of its first tile (tile 8) and a short piece at a tile's end (tile 13)"""
    T = TILE
    return BIG_N, np.array([1000, 3 * T + 2000, 8 * T + 300, 13 * T + 4000, 14 * T + 50, BIG_N - 3], dtype=np.uint64)


def pairs_layout():
    """(n, off): 2049 segments of 2 keys from position 5 on"""
    return 5 + 2 * 2049 + 3, offsets_from([2] * 2049, start=5)


def empties_layout():
    """(n, off): _compact_ref.empties_layout: 5000 empty segments at one position inside a tile"""
    return 12000, np.concatenate([[0], np.full(5001, 7000), [12000]]).astype(np.uint64)


def fifties_layout():
    """(n, off): 2^16 segments of 50 keys"""
    S = 1 << 16
    return 50 * S, (np.arange(S + 1, dtype=np.uint64) * np.uint64(50))


# name -> (layout, B, the paths its pieces must take: exactly this set)
LAYOUTS = {
    "ragged_lds": (ragged_layout, 64, {"direct", "lds_first", "lds_flush"}),                    # (one tile a workgroup: nothing carries over)
    "ragged_direct_4097": (ragged_layout, 4097, {"direct"}),
    "ragged_direct_50257": (ragged_layout, 50257, {"direct"}),
    "one_segment_three_tiles": (lambda: (SKEW_N, None), 256, {"lds_first", "direct"}),          # (the 17-key tail is a short piece)
    "big_one_segment": (lambda: (BIG_N, None), 256, {"lds_first", "lds_same", "direct"}),
    "big_boundaries": (big_boundaries_layout, 256, {"lds_first", "lds_same", "lds_flush", "direct"}),
    "pairs": (pairs_layout, 16, {"direct"}),
    "empties": (empties_layout, 16, {"lds_first", "lds_flush"}),
    "fifties": (fifties_layout, 16, {"direct"}),
}


# -- the cases of the bin arithmetic: tests/test_histogram.py sends them through host/bin/bins_selftest (g++), ------------------------------
# -- tests/test_gpu_histogram_paths.py through the kernels; both draw them here, from the same seeds ------------------------------------------

def around(dt, values):
    """every value, the key before and the key after it in ascending order"""
    v = order_map(np.array(values, dtype=dt))
    one = v.dtype.type(1)
    return np.concatenate([order_unmap(v - one, dt), order_unmap(v, dt), order_unmap(v + one, dt)])


def edges_cases(dt, descending):
    """(B, edges, keys): every edge and the keys next to it, random keys, the float specials; B = 13 has -0.0 and +0.0 as two edges"""
    dt = np.dtype(dt)
    rng = np.random.default_rng(80 + DTYPES.index(dt.name) * 2 + descending)
    for B in (1, 2, 13, 4096):
        edges = sorted_edges(rng, dt, B, SPAN if B < 4096 else None, descending)
        if dt.kind == "f" and B == 13:                              # -0.0 next to +0.0 as two edges
            edges[:2] = [0.0, -0.0]
            edges = edges[np.argsort(order_map(edges, descending), kind="stable")]
            assert np.unique(edges.view(UINT[dt.itemsize])).size == B + 1
        keys = np.concatenate([around(dt, edges), random_keys(rng, dt, 500, SPAN)] + ([special_floats(dt)] if dt.kind == "f" else []))
        yield B, edges, keys


def even_int_cases(dt, descending):
    """(shift, lo, B, keys): lo at info.min and at info.max - 70, width_shift up to width - 1; the keys around every bin boundary"""
    dt = np.dtype(dt)
    rng = np.random.default_rng(90 + DTYPES.index(dt.name) * 2 + descending)
    info = np.iinfo(dt)
    width = 8 * dt.itemsize
    for shift in (0, 5, width - 1):
        for lo in ([0, 1000, info.max - 70] if dt.kind == "u" else [-1000, -1, 0, info.min, info.max - 70]):
            for B in (1, 3, 64):
                edge = [lo + (b << shift) for b in range(B + 2) if lo + (b << shift) <= info.max]
                keys = np.concatenate([around(dt, edge), around(dt, [info.min, info.max, 0]), random_keys(rng, dt, 200, None),
                                       random_keys(rng, dt, 200, 2000)])
                yield shift, lo, B, keys


def even_float_cases(dt, descending):
    """(B, lo, hi, keys): keys whose product (x - lo) * scale lies one ulp either side of an integer: x = lo + b / scale and its
    neighbours, twice over; lo and hi and theirs; the specials.  A subnormal x - lo is unspecified: no key has one."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(95 + DTYPES.index(dt.name) * 2 + descending)
    for B, lo, hi in ((1, -1.0, 1.0), (7, -3.0, 11.0), (64, 0.0, 64.0), (100, 0.1, 0.7), (4096, -1024.0, 1536.0), (50257, 1.0, 3.0)):
        lo_, hi_ = dt.type(lo), dt.type(hi)
        scale = dt.type(dt.type(B) / dt.type(hi_ - lo_))
        b = np.unique(rng.integers(0, B + 1, 40))
        near = (lo_ + (b.astype(dt) / scale).astype(dt)).astype(dt)
        keys = np.concatenate([around(dt, around(dt, near)), around(dt, [lo_, hi_]), special_floats(dt),
                               (rng.standard_normal(300) * (hi - lo)).astype(dt) + lo_])
        sub = np.abs((keys - lo_).astype(dt))
        keys = keys[~((sub > 0) & (sub < np.finfo(dt).tiny))]       # a subnormal x - lo is unspecified: no test rests on it
        yield B, lo, hi, keys


def even_float_case_holds(keys, B, lo, hi, want, descending):
    """what a float case must hold, from the referee's bins `want` alone: products that are whole numbers and products that are not,
    dropped keys, lo in the first bin and hi in the last"""
    dt = keys.dtype
    lo_, hi_ = dt.type(lo), dt.type(hi)
    scale = dt.type(dt.type(B) / dt.type(hi_ - lo_))
    t = ((keys - lo_).astype(dt) * scale).astype(dt)
    inside = want != NO_BIN
    assert np.any(inside & (t != np.floor(t))) and np.any(inside & (t == np.floor(t))) and np.any(~inside)
    top = B - 1 if not descending else 0
    assert want[np.flatnonzero(keys == hi_)[0]] == top and want[np.flatnonzero(keys == lo_)[0]] == B - 1 - top


# How the GPU test sends one case (its keys once, in this order): [(name, n, off)] with the keys repeated up to n.
ARITH_MIN_KEYS = 2 * DIRECT_PIECE + 100            # both halves of the two-segment form are LDS pieces


def arith_forms(nkeys):
    """one segment (LDS up to 4096 bins); two segments cut at an odd position; pieces of 255 keys (all direct)"""
    n = max(nkeys, ARITH_MIN_KEYS)
    cut = (n // 2) | 1
    return [("one segment", n, None), ("two segments", n, np.array([0, cut, n], dtype=np.uint64)),
            ("pieces of 255", n, np.minimum(np.arange(0, n + 255, 255, dtype=np.uint64), np.uint64(n)))]


# -- the piece-slot layouts: every one at most 3 tiles (one tile a workgroup) -----------------------------------------------------------------

def slots16_layout():
    """(n, off): 16 segments of exactly 256 keys on the tile's grid: slots 0 .. 15 of one tile"""
    return TILE, np.arange(17, dtype=np.uint64) * np.uint64(DIRECT_PIECE)


def slots16_shifted_layout():
    """(n, off): a 255-key segment, then 17 of 256 keys: piece starts 255 + 256 i; the one from 4095 has one key in tile 0 and 255 in tile 1"""
    off = np.concatenate([[0], 255 + DIRECT_PIECE * np.arange(18)]).astype(np.uint64)
    return int(off[-1]) + 5, off


def lengths_cycle_layout():
    """(n, off): lengths 255, 256, 257, 256 eight times: two tiles, every piece a whole segment"""
    return 2 * TILE, offsets_from([255, 256, 257, 256] * 8)


def ends_with_tile_layout():
    """(n, off): tile 0 ends with an LDS piece of a segment that ends with the tile; tile 1 lies inside the next segment, which goes on into tile 2"""
    return 3 * TILE, np.array([5, 3000, TILE, 9000, 3 * TILE - 7], dtype=np.uint64)


SLOT_LAYOUTS = {"slots16": slots16_layout, "slots16_shifted": slots16_shifted_layout, "lengths_cycle": lengths_cycle_layout,
                "ends_with_tile": ends_with_tile_layout}


def shifted_bins(rng, n, off, B):
    """the bin of every key, as numbers: segment s holds bins (s + {0, 1, 2}) % B, so that neighbours' histograms differ; one key in 50
    has bin B + 1 (dropped); outside the segments anything in [0, B + 2)"""
    o = _offsets(n, off)
    seg = np.repeat(np.arange(o.size - 1, dtype=np.int64), np.diff(o))
    b = rng.integers(0, B + 2, n)
    live = (seg + rng.integers(0, 3, seg.size)) % B
    b[int(o[0]):int(o[-1])] = np.where(rng.integers(0, 50, seg.size) == 0, B + 1, live)
    return b


SLOT_EDGE_STEP = 1 << 40                           # the uint64 edges of the B = 4096 form: step * arange(B + 1); a key of bin b is b * step + step / 2


# -- the counter layout boundary and the zero fill ------------------------------------------------------------------------------------------------

BOUNDARY_BINS = [1023, 1024, 1025, 4095]           # the last wave-private size, cnt[4096] filled exactly by four copies, the first shared size; the last-but-one
ZERO_SMALL = {1: (1, 1), 2: (2, 1), 3: (3, 1), 4: (2, 2), 5: (1, 5), 7: (7, 1), 8: (2, 4), 9: (3, 3)}      # S * B -> (S, B)
ZERO_ALIGN = [0, 4, 8, 12]                         # bytes from a 16-byte boundary to the first counter
ZERO_BIG_BINS = 65


def zero_small_layout(S):
    """(n, off): S segments of 0, 1, 2, 0, 1, 2 ... keys from position 1, one trailing key"""
    off = offsets_from([s % 3 for s in range(S)], start=1)
    return int(off[-1]) + 1, off


def zero_big_layout():
    """(n, off): fifties_layout plus one segment: 2^16 + 1 segments of 50 keys"""
    S = (1 << 16) + 1
    return 50 * S, (np.arange(S + 1, dtype=np.uint64) * np.uint64(50))


def zero_grid(total, cus=256):
    """(workgroups of bins_zero_kernel, 16-byte stores at most, trips of the grid-stride loop) for `total` counters"""
    nvec = total // 4
    grid = min((nvec + 255) // 256 + 1, 16 * cus)
    return grid, nvec, (nvec + grid * 256 - 1) // (grid * 256)
