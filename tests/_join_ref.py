"""Host referee of rsx_segmented_join (no GPU, no library), the grid its kernels state at the top of radix-sort_amd/csrc/rsx_join.hpp, and
the layouts of tests/test_gpu_join.py, each with the path it is there for.

For A element i of segment s (relative to aoff[s]), lb and ub the lower and upper bound of its key in B_s in the engine's order
(tests/_search_ref.py: order_map) and c = ub - lb:  INNER the rows (i, lb + r), r < c;  LEFT the same and (i, none) where c == 0;  SEMI
(i, lb) iff c > 0;  ANTI (i, -) iff c == 0.  Rows by segment, i, B position.  "none" is -1 here (0xFFFFFFFF on the device).

  join_oracle   np.searchsorted left / right per segment, np.repeat and arange (needs sorted segments)
  join_brute    the double loop over bit equality (small cases)
  model         what the kernels do with a layout: rows per absolute A position, R(j) = tbase[j >> 12] + pre[j], and per tile of 4096 output
                rows the A positions that start in it, its path (FILL: none starts in it, one owner; MARK: the LDS marks), and the named
                events of `paths`
"""
import numpy as np

from _search_ref import UINT, order_map, sort_engine_order

TILE = 4096
INNER, LEFT, SEMI, ANTI = 0, 1, 2, 3
KINDS = {"inner": INNER, "left": LEFT, "semi": SEMI, "anti": ANTI}
DTYPES = ("uint32", "int32", "uint64", "int64", "float32", "float64")
FILL, MARK = "fill", "mark"
# the events a layout can be there for
PURE_FILL, MARK_TILE, ZERO_A_TILE_IN_WALK, SPANS_3_TILES, SEGMENT_START_INSIDE = "pure fill", "mark tile", "zero A tile in a walk", "3 output tiles", "segment start inside"


def bounds(n, off):
    """[(start, end)] of the segments; off None: the one segment [0, n)"""
    if off is None:
        return [(0, n)]
    o = np.asarray(off).astype(np.int64)
    return [(int(o[s]), int(o[s + 1])) for s in range(o.size - 1)]


def effective(c, op):
    c = np.asarray(c, dtype=np.int64)
    return c if op == INNER else np.maximum(c, 1) if op == LEFT else (c > 0).astype(np.int64) if op == SEMI else (c == 0).astype(np.int64)


def counts(a, aoff, b, boff, descending=False):
    """(lb, c) per A element of [aoff[0], aoff[S]), concatenated over the segments; int64"""
    ka, kb = order_map(a, descending), order_map(b, descending)
    lbs, cs = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for (a0, a1), (b0, b1) in zip(bounds(ka.size, aoff), bounds(kb.size, boff)):
        lb = np.searchsorted(kb[b0:b1], ka[a0:a1], side="left").astype(np.int64)
        ub = np.searchsorted(kb[b0:b1], ka[a0:a1], side="right").astype(np.int64)
        lbs.append(lb)
        cs.append(ub - lb)
    return np.concatenate(lbs), np.concatenate(cs)


def join_oracle(a, aoff, b, boff, op, descending=False):
    """(ia, ib, keys, out_offsets): int64 indices relative to their segments (ib -1: none; all -1 for ANTI), the A keys, S + 1 offsets"""
    a = np.ascontiguousarray(a)
    lb, c = counts(a, aoff, b, boff, descending)
    e = effective(c, op)
    segs = bounds(a.size, aoff)
    lo = segs[0][0] if segs else 0
    rel = np.concatenate([np.arange(a1 - a0, dtype=np.int64) for a0, a1 in segs] + [np.zeros(0, dtype=np.int64)])
    start = np.concatenate([[0], np.cumsum(e)]).astype(np.int64)                     # rows before every A element
    owner = np.repeat(np.arange(e.size, dtype=np.int64), e)
    rank = np.arange(int(start[-1]), dtype=np.int64) - start[:-1][owner]
    first = np.where(c == 0, -1, lb)
    ia = rel[owner]
    ib = np.where(first[owner] < 0, -1, first[owner] + rank) if op != ANTI else np.full(owner.size, -1, dtype=np.int64)
    ends = np.array([a1 - lo for _, a1 in segs], dtype=np.int64)
    ooff = np.concatenate([[0], start[ends]]).astype(np.uint64) if segs else np.zeros(1, dtype=np.uint64)
    return ia, ib, a[lo + owner], ooff


def join_brute(a, aoff, b, boff, op):
    """the definition by a double loop over bit equality; on sorted segments the order of the rows is the oracle's"""
    ua, ub = np.ascontiguousarray(a).view(UINT[a.dtype.itemsize]), np.ascontiguousarray(b).view(UINT[b.dtype.itemsize])
    ia, ib, ooff = [], [], [0]
    for (a0, a1), (b0, b1) in zip(bounds(ua.size, aoff), bounds(ub.size, boff)):
        for i in range(a0, a1):
            partners = [j - b0 for j in range(b0, b1) if ub[j] == ua[i]]
            if op == INNER or (op == LEFT and partners):
                ia += [i - a0] * len(partners)
                ib += partners
            elif op == LEFT or (op == ANTI and not partners):
                ia.append(i - a0)
                ib.append(-1)
            elif op == SEMI and partners:
                ia.append(i - a0)
                ib.append(partners[0])
        ooff.append(len(ia))
    return np.array(ia, dtype=np.int64), np.array(ib, dtype=np.int64), np.array(ooff, dtype=np.uint64)


# -- the kernels' grid ------------------------------------------------------------------------------------------------------------------------

def model(a, aoff, b, boff, op, descending=False, capacity=None):
    """dict: cnt (rows per absolute A position, padding to whole tiles included), R (rows before every position, one more entry), ttot,
    total, tiles = [(path, s_lo, s_hi)] of the output tiles that write a row, ooff"""
    na = np.asarray(a).size
    segs = bounds(na, aoff)
    lo = segs[0][0] if segs else 0
    _, c = counts(a, aoff, b, boff, descending)
    ntiles = -(-na // TILE)
    cnt = np.zeros(ntiles * TILE, dtype=np.int64)
    cnt[lo:lo + c.size] = effective(c, op)
    R = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    total = int(R[-1])
    written = total if capacity is None else min(total, capacity)
    tiles = []
    for u in range(-(-written // TILE)):
        s_lo = int(np.searchsorted(R[:-1], u * TILE, side="left"))
        s_hi = int(np.searchsorted(R[:-1], (u + 1) * TILE, side="left"))
        tiles.append((FILL if s_lo == s_hi else MARK, s_lo, s_hi))
    starts = np.array([R[a0] for a0, _ in segs], dtype=np.int64)
    return {"cnt": cnt, "R": R, "ttot": cnt.reshape(-1, TILE).sum(axis=1) if ntiles else np.zeros(0, dtype=np.int64), "total": total, "written": written,
            "tiles": tiles, "starts": starts}


def paths(a, aoff, b, boff, op, descending=False, capacity=None):
    """the named events that the layout reaches"""
    m = model(a, aoff, b, boff, op, descending, capacity)
    got = set()
    for path, s_lo, s_hi in m["tiles"]:
        got.add(PURE_FILL if path == FILL else MARK_TILE)
        if path == MARK and any(m["ttot"][t] == 0 for t in range(s_lo // TILE, (s_hi - 1) // TILE + 1)):
            got.add(ZERO_A_TILE_IN_WALK)
    live = m["cnt"] > 0
    first, last = m["R"][:-1][live], m["R"][1:][live] - 1
    if np.any(last // TILE - first // TILE >= 2):
        got.add(SPANS_3_TILES)
    inner = m["starts"][1:]
    if np.any((inner % TILE != 0) & (inner < m["written"])):
        got.add(SEGMENT_START_INSIDE)
    return got


# -- layouts: (a, aoff, b, boff) of uint32 keys, ascending; tests cast and re-sort them --------------------------------------------------------

def offsets_from(lengths, start=0):
    return np.concatenate([[start], start + np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uint64)


def ragged_lengths():
    """37 segments of 0 .. 9000 keys a side: empties on A only, on B only and on both; short, tile-sized and multi-tile segments"""
    la = [0, 5, 0, 1, 4095, 4096, 4097, 9000, 17, 0, 300, 2, 8193, 1, 0, 64, 1000, 3, 0, 4100, 7, 50, 0, 129, 2500, 1, 0, 33, 4096, 9, 0, 777, 5000, 2, 0, 61, 8999]
    lb = [3, 0, 0, 4097, 1, 9000, 4096, 10, 0, 0, 4095, 8, 5, 1, 0, 3000, 1000, 0, 6, 20, 7, 0, 0, 8193, 1, 64, 12, 0, 4096, 9, 0, 300, 2, 5000, 1, 0, 9000]
    return la, lb


def layout_ragged(seed=0):
    """keys of segment s drawn from max(L, 1) x (1 .. 3) values, L the longer side: c takes 0, 1 and several"""
    rng = np.random.default_rng(seed)
    la, lb = ragged_lengths()
    a, b = [], []
    for s, (x, y) in enumerate(zip(la, lb)):
        span = max(x, y, 1) * (1 + s % 3)
        a.append(np.sort(rng.integers(0, span, x, dtype=np.uint32)))
        b.append(np.sort(rng.integers(0, span, y, dtype=np.uint32)))
    return np.concatenate(a), offsets_from(la), np.concatenate(b), offsets_from(lb)


def layout_all_equal(na, nb):
    return np.full(na, 7, dtype=np.uint32), None, np.full(nb, 7, dtype=np.uint32), None


def layout_total(P):
    """one segment, P rows: max(P, 3) distinct A keys of which the first P have one partner each"""
    a = np.arange(max(P, 3), dtype=np.uint32) * 2
    return a, None, a[:P].copy(), None


def layout_one_partner(na):
    a = np.arange(na, dtype=np.uint32) * 3 + 1
    return a, None, a.copy(), None


SPARSE_MATCHES = (3, 10, 20, 8200, 8300, 12288, 12292)


def layout_sparse():
    """3 x 4096 + 5 keys a side, 7 of them common, none in A tile 1: INNER's one output tile walks an A tile without a row"""
    n = 3 * TILE + 5
    a = np.arange(n, dtype=np.uint32) * 2
    b = a + 1
    b[list(SPARSE_MATCHES)] -= 1
    return a, None, b, None


def layout_many_segments(seed=1):
    """4096 segments of 3 .. 50 keys a side over few values"""
    rng = np.random.default_rng(seed)
    la, lb = rng.integers(3, 51, 4096), rng.integers(3, 51, 4096)
    a = [np.sort(rng.integers(0, 40, x, dtype=np.uint32)) for x in la]
    b = [np.sort(rng.integers(0, 40, y, dtype=np.uint32)) for y in lb]
    dead = lambda k: np.full(k, 1, dtype=np.uint32)               # keys outside [off[0], off[S]): never read as keys of a segment
    return np.concatenate([dead(5)] + a + [dead(3)]), offsets_from(la, 5), np.concatenate([dead(2)] + b + [dead(1)]), offsets_from(lb, 2)


def layout_zipf(seed=2, total=1 << 16):
    """Zipf lengths, about 2^16 keys a side in all, with empty segments on either side"""
    rng = np.random.default_rng(seed)

    def lengths():
        out, left = [], total
        while left > 0:
            k = min(int(rng.zipf(1.3)) - 1, left, 20000)
            out.append(k)
            left -= k
        return out

    la, lb = lengths(), lengths()
    S = max(len(la), len(lb))                                     # (the side with fewer segments ends in empty ones)
    la, lb = la + [0] * (S - len(la)), lb + [0] * (S - len(lb))
    a = [np.sort(rng.integers(0, max(x, y, 1) + 3, x, dtype=np.uint32)) for x, y in zip(la, lb)]
    b = [np.sort(rng.integers(0, max(x, y, 1) + 3, y, dtype=np.uint32)) for x, y in zip(la, lb)]
    return np.concatenate(a), offsets_from(la), np.concatenate(b), offsets_from(lb)


# name -> (generator, kind, the events it must reach)
LAYOUTS = {
    "ragged": (layout_ragged, INNER, {MARK_TILE, SEGMENT_START_INSIDE}),
    "all equal 5000 x 3": (lambda: layout_all_equal(5000, 3), INNER, {MARK_TILE}),
    "all equal 3 x 10000": (lambda: layout_all_equal(3, 10000), INNER, {PURE_FILL, MARK_TILE, SPANS_3_TILES}),
    "all equal 4096 x 1": (lambda: layout_all_equal(4096, 1), INNER, {MARK_TILE}),
    "all equal 1 x 8193": (lambda: layout_all_equal(1, 8193), INNER, {PURE_FILL, SPANS_3_TILES}),
    "sparse inner": (layout_sparse, INNER, {MARK_TILE, ZERO_A_TILE_IN_WALK}),
    "sparse left": (layout_sparse, LEFT, {MARK_TILE}),
    "many segments": (layout_many_segments, INNER, {MARK_TILE, SEGMENT_START_INSIDE}),
    "zipf": (layout_zipf, INNER, {MARK_TILE, SEGMENT_START_INSIDE}),
}
TOTALS = (0, 1, 4095, 4096, 4097, 8192)
ONE_PARTNER = (1, 4095, 4096, 4097, 8193)


def typed(a, aoff, b, boff, dtype, descending):
    """the layout's keys as `dtype` (shifted so that signed and float types get negative keys; floats: A's zeros at odd positions become
    -0.0, which joins nothing of B's +0.0), every segment sorted in the engine's order"""
    dt = np.dtype(dtype)

    def cast(x, minus_zero):
        y = x.astype(np.int64) - (0 if dt.kind == "u" else 11)
        y = y.astype(dt)
        if dt.kind == "f" and minus_zero:
            z = np.flatnonzero(y == 0)
            y[z[1::2]] = -0.0
        return y

    def resort(x, off):
        out = x.copy()
        for s0, s1 in bounds(x.size, off):
            out[s0:s1] = sort_engine_order(x[s0:s1], descending)
        return out

    return resort(cast(a, True), aoff), aoff, resort(cast(b, False), boff), boff
