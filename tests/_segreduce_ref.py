"""Referee of the segmented reduction (rsx_segmented_reduce): plain numpy, no GPU and no library.

reduce_oracle   op over every segment, one slice at a time.  Integer sums wrap; float sums are taken in a wider format (float64 for
                float32, numpy's extended precision for float64) and returned in it; float min / max give NaN if the segment holds one;
                the arg ops give the FIRST position of the extreme, a NaN beating every number.  Empty segments: the identity, index -1.
model_sum       the association written at the top of rsx_segreduce.hpp, transcribed for float32 / float64 from the values, the offsets
                and n alone: the bits the kernels must produce.
reduce_terms    per segment: the elements folded and the sum of their magnitudes, for the any-order error bound.
reduce_fast, terms_fast   the same two by ufunc.reduceat, without a Python loop over the segments (tests/test_segreduce.py holds them
                to the loop forms).
The named layouts at the end are (n, offsets) pairs; paths() says, from a layout alone, which paths of the kernels it reaches, and
join_schedule() which open tiles every workgroup of the join takes, in order.
"""
import numpy as np

OPS = ("sum", "min", "max", "argmin", "argmax")
OPCODE = {"sum": 0, "min": 1, "max": 2, "argmin": 3, "argmax": 4}
WIDE = {np.dtype(np.float32): np.float64, np.dtype(np.float64): np.longdouble}
UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
TILE, KPT, THREADS, WAVE = 4096, 16, 256, 64
JOIN = 256                                                         # threads of the join: thread r folds lead[r], lead[r + 256], ...
NO_INDEX = 0xFFFFFFFF


def identity(dtype, op):
    dtype = np.dtype(dtype)
    if op == "sum":
        return dtype.type(0)
    low = op in ("min", "argmin")
    if dtype.kind == "f":
        return dtype.type(np.inf if low else -np.inf)
    info = np.iinfo(dtype)
    return dtype.type(info.max if low else info.min)


def _offsets(n, off):
    return np.array([0, n], dtype=np.int64) if off is None else np.asarray(off).astype(np.int64)


def first_extreme(x, low):
    """position of the first minimum (low) or maximum of the non-empty 1-D x; the first NaN if there is one"""
    if x.dtype.kind == "f":
        nan = np.flatnonzero(np.isnan(x))
        if nan.size:
            return int(nan[0])
    best = x.min() if low else x.max()
    return int(np.flatnonzero(x == best)[0])                       # (-0.0 == +0.0: they tie)


def reduce_oracle(values, off=None, op="sum"):
    """(results, indices): indices is None unless op is an arg op; then results holds the values at those positions, bits unchanged"""
    v = np.asarray(values)
    o = _offsets(v.size, off)
    nseg = len(o) - 1
    arg = op in ("argmin", "argmax")
    low = op in ("min", "argmin")
    if op == "sum" and v.dtype.kind == "f":
        res = np.zeros(nseg, dtype=WIDE[v.dtype])
    else:
        res = np.full(nseg, identity(v.dtype, op), dtype=v.dtype)
    idx = np.full(nseg, -1, dtype=np.int64) if arg else None
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(nseg):
            x = v[o[s]:o[s + 1]]
            if x.size == 0:
                continue
            if op == "sum":
                res[s] = x.astype(res.dtype).sum() if v.dtype.kind == "f" else np.add.reduce(x, dtype=v.dtype)
            elif arg:
                idx[s] = first_extreme(x, low)
                res[s] = x[idx[s]]
            elif v.dtype.kind == "f" and np.isnan(x).any():
                res[s] = np.nan
            else:
                res[s] = x.min() if low else x.max()
    return res, idx


def reduce_terms(values, off=None):
    """(m, mag) per segment: the number of elements and the sum of |v| in the wide format"""
    v = np.asarray(values)
    o = _offsets(v.size, off)
    wide = WIDE[v.dtype]
    mag = np.array([np.abs(v[o[s]:o[s + 1]].astype(wide)).sum() for s in range(len(o) - 1)], dtype=wide)
    return (o[1:] - o[:-1]).astype(np.int64), mag


# -- the same without a loop over the segments, for layouts of a million of them ----------------------------------------------------------

def _live(o):
    """the non-empty segments and where each starts inside [off[0], off[S]): they lie back to back there, which is what reduceat folds"""
    live = np.flatnonzero(o[1:] > o[:-1])
    return live, o[live] - o[0]


def reduce_fast(values, off=None, op="sum"):
    """reduce_oracle by ufunc.reduceat over the non-empty segments.  The float sums are folded left to right in the wide format where
    reduce_oracle adds pairwise: equal wherever the wide sums are exact, one rounding of the wide format apart otherwise.  The sign of a
    zero minimum or maximum is numpy's choice in both forms (the arg ops return the element itself: its own bits)."""
    v = np.asarray(values)
    o = _offsets(v.size, off)
    nseg = len(o) - 1
    arg = op in ("argmin", "argmax")
    low = op in ("min", "argmin")
    floats = v.dtype.kind == "f"
    res = np.zeros(nseg, dtype=WIDE[v.dtype]) if op == "sum" and floats else np.full(nseg, identity(v.dtype, op), dtype=v.dtype)
    idx = np.full(nseg, -1, dtype=np.int64) if arg else None
    live, at = _live(o)
    if live.size == 0:
        return res, idx
    x = v[o[0]:o[-1]]
    with np.errstate(over="ignore", invalid="ignore"):
        if op == "sum":
            res[live] = np.add.reduceat(x.astype(res.dtype), at) if floats else np.add.reduceat(x, at, dtype=v.dtype)
            return res, idx
        best = (np.minimum if low else np.maximum).reduceat(x, at)             # (NaN if the segment holds one)
        if not arg:
            res[live] = best
            return res, idx
        lengths = (o[live + 1] - o[live]).astype(np.int64)
        mine = np.repeat(best, lengths)
        hit = np.flatnonzero((x == mine) | ((x != x) & (mine != mine)))     # a NaN beats every number: where the extreme is NaN the NaNs are the hits
        first = hit[np.searchsorted(hit, at, side="left")]                  # the first hit at or behind each start: inside the segment, which has one
        idx[live] = first - at
        res[live] = x[first]
    return res, idx


def terms_fast(values, off=None):
    """reduce_terms by reduceat (the magnitudes folded left to right in the wide format)"""
    v = np.asarray(values)
    o = _offsets(v.size, off)
    wide = WIDE[v.dtype]
    mag = np.zeros(len(o) - 1, dtype=wide)
    live, at = _live(o)
    if live.size:
        mag[live] = np.add.reduceat(np.abs(v[o[0]:o[-1]].astype(wide)), at)
    return (o[1:] - o[:-1]).astype(np.int64), mag


# -- the written association ------------------------------------------------------------------------------------------------------------

def _join(leads):
    """J of rsx_segreduce.hpp over the m >= 1 partials lead[t+1 .. u]"""
    dt = leads.dtype
    m = leads.size
    rows = (m + JOIN - 1) // JOIN
    pad = np.zeros(rows * JOIN, dtype=dt)
    pad[:m] = leads
    have = (np.arange(rows * JOIN) < m).reshape(rows, JOIN)
    pad = pad.reshape(rows, JOIN)
    p, has = pad[0].copy(), have[0].copy()
    for i in range(1, rows):                                       # thread r: left to right over r, r + 256, ...
        p = np.where(have[i], p + pad[i], p)
    p, has = p.reshape(JOIN // WAVE, WAVE), has.reshape(JOIN // WAVE, WAVE)
    d = 1
    while d < WAVE:                                                # the tree of a wave: y[l] = y[l] o y[l + d]
        q, qh = p.copy(), has.copy()
        take = qh[:, d:]
        p[:, :-d] = np.where(take, np.where(qh[:, :-d], q[:, :-d] + q[:, d:], q[:, d:]), q[:, :-d])
        has[:, :-d] = qh[:, :-d] | take
        d *= 2
    total = p[0, 0]
    for w in range(1, JOIN // WAVE):                               # the wave totals, left to right
        if has[w, 0]:
            total = total + p[w, 0]
    return total


def model_sum(values, off=None):
    """the float sums of all segments in the order of rsx_segreduce.hpp, as an array of the values' dtype"""
    v = np.asarray(values)
    dt = v.dtype
    assert dt.kind == "f"
    n = v.size
    o = _offsets(n, off)
    nseg = len(o) - 1
    out = np.zeros(nseg, dtype=dt)
    lo, hi = int(o[0]), int(o[-1])
    if lo >= hi:
        return out
    ntiles = (n + TILE - 1) // TILE
    pad = np.zeros(ntiles * TILE, dtype=dt)
    pad[lo:hi] = v[lo:hi]                                          # elements outside [off[0], off[S]) count as 0
    live = np.flatnonzero(o[1:] > o[:-1])
    r = np.zeros(ntiles * TILE, dtype=bool)
    r[o[live]] = True
    with np.errstate(over="ignore", invalid="ignore"):
        a = pad.reshape(ntiles, THREADS, KPT).copy()
        rr = r.reshape(ntiles, THREADS, KPT)
        for j in range(1, KPT):                                    # the thread level
            a[:, :, j] = np.where(rr[:, :, j], a[:, :, j], a[:, :, j - 1] + a[:, :, j])
        cut = np.cumsum(rr, axis=2) > 0                            # a restart of the thread at or before j
        x = a[:, :, KPT - 1].reshape(ntiles, THREADS // WAVE, WAVE).copy()
        xf = rr.any(axis=2).reshape(ntiles, THREADS // WAVE, WAVE).copy()
        d = 1
        while d < WAVE:                                            # the flagged Hillis-Steele scan of a wave
            y, yf = x[:, :, :-d].copy(), xf[:, :, :-d].copy()
            x[:, :, d:] = np.where(xf[:, :, d:], x[:, :, d:], y + x[:, :, d:])
            xf[:, :, d:] |= yf
            d *= 2
        wv, wf = x[:, :, WAVE - 1].copy(), xf[:, :, WAVE - 1].copy()
        pv, pf = wv[:, 0].copy(), wf[:, 0].copy()
        for w in range(1, THREADS // WAVE):                        # the wave totals, left to right, on the left of the lanes' x
            x[:, w, :] = np.where(xf[:, w, :], x[:, w, :], pv[:, None] + x[:, w, :])
            xf[:, w, :] |= pf[:, None]
            pv = np.where(wf[:, w], wv[:, w], pv + wv[:, w])
            pf = pf | wf[:, w]
        T = x.reshape(ntiles, THREADS)

        last = o[live + 1] - 1
        t, q, j = last // TILE, (last % TILE) // KPT, last % KPT
        own = a[t, q, j]
        before = T[t, np.maximum(q, 1) - 1]
        E = np.where(cut[t, q, j], own, np.where(j == KPT - 1, T[t, q], np.where(q == 0, own, before + own)))
        ta = o[live] // TILE
        out[live] = E
        for i in np.flatnonzero(ta < t):                           # the segments that cross a tile edge
            leads = np.concatenate([T[ta[i] + 1:t[i], THREADS - 1], E[i:i + 1]])
            out[live[i]] = T[ta[i], THREADS - 1] + _join(leads)
    return out


# -- the named layouts: (n, offsets) ----------------------------------------------------------------------------------------------------

LENGTHS = [1500, 0, 1, 2, 15, 16, 17, 255, 256, 4095, 4096, 4097, 0, 3, 17, 0, 256, 1, 4096, 15, 4097, 2, 0]
CUS = 256                                                          # MI355X: two tiles per workgroup above 16 * 256 tiles


def offsets_from(lengths, start=0):
    return np.concatenate([[start], start + np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uint64)


def layout_ragged():
    off = offsets_from(LENGTHS, start=3)
    return int(off[-1]) + 5, off


def layout_inside():
    """every segment inside one tile: three tiles, none crossed"""
    off = offsets_from([100, 0, 3900, 96, 1, 4095, 2000, 2096])
    return 3 * TILE, off


def layout_ends_on_edge():
    """segments that end exactly on a tile edge: one that began in the tile, one that began a tile earlier, and the last one at off[S]"""
    off = offsets_from([7, 4089, 4000, 4192, 4096], start=0)
    return 4 * TILE + 9, off


def layout_first_last():
    """a boundary at the first element of a tile and one at its last"""
    off = offsets_from([5, TILE - 5, 1, TILE - 2, 1, 30], start=0)
    return 2 * TILE + 100, off


def layout_long(tiles, start=11):
    """one segment of `tiles` tiles' worth of elements that begins inside a tile, between two short ones"""
    off = offsets_from([start, tiles * TILE, 9])
    return int(off[-1]) + 3, off


def layout_two_tiles(rows):
    n = (1 << 24) + 4097
    if not rows:
        return n, np.array([0, n], dtype=np.uint64)
    off = np.minimum(np.arange(0, n + TILE, TILE, dtype=np.uint64), np.uint64(n))
    return n, off


def layout_many_empty():
    """5000 empty segments at one position, in the middle of a tile"""
    return 3000, offsets_from([1234] + [0] * 5000 + [1766])


def layout_empty_at_end():
    """empty segments at off[S] == n with n a multiple of 4096: no tile holds that position"""
    return 2 * TILE, offsets_from([TILE, TILE, 0, 0, 0])


def layout_all_empty():
    return 5000, offsets_from([0] * 7, start=4100)


def dense_cycle(lengths, lead=()):
    """(n, off): off[0] = 3, then `lead`, then `lengths` over and over, cut so that the segments cover two tiles and 37 elements; 5 trailing elements"""
    want = 2 * TILE + 37
    out = list(lead)
    while sum(out) < want:
        out += list(lengths)
    total = np.cumsum(out)
    keep = int(np.searchsorted(total, want, side="left")) + 1
    out = out[:keep]
    out[-1] -= int(total[keep - 1]) - want
    off = offsets_from(out, start=3)
    assert int(off[-1]) == 3 + want
    return int(off[-1]) + 5, off


def layout_every_element():
    """every element is a segment of its own: 16 flags in every thread, 4096 entries of ids.last in a whole tile"""
    return dense_cycle([1])


def layout_ones_and_empties():
    """lengths 1, 0, 2, 0, 0, 1, 3: empty segments before and behind one-element segments, four starts in many a thread"""
    return dense_cycle([1, 0, 2, 0, 0, 1, 3])


def layout_thread_edges():
    """lengths 16, 1, 15 from position 16 on (a first segment of 13 elements takes off[0] = 3 there): boundaries on every thread edge
    and, every other thread, one element behind it"""
    return dense_cycle([16, 1, 15], lead=[13])


DENSE = {"every element": layout_every_element, "ones and empties": layout_ones_and_empties, "thread edges": layout_thread_edges}

POSITIONS = [0, 1, 15, 16, 17, 1023, 1024, 4095, 4096, 4097, 8191, 8192, 12287, 12288]
POSITIONS_N = 3 * TILE


def position_layouts():
    """[(n, off)]: one segment [lo, hi) for every pair lo < hi of POSITIONS, n = 3 tiles; then the two segments [3, b) and [b, n - 3) for
    every b of POSITIONS that leaves both non-empty (0, 1, 12287 and 12288 would make the offsets decrease: no valid call); and two
    segments that end on a thread edge inside a LATER tile than they began in, which no pair of POSITIONS does"""
    n = POSITIONS_N
    one = [(n, np.array([a, b], dtype=np.uint64)) for i, a in enumerate(POSITIONS) for b in POSITIONS[i + 1:]]
    two = [(n, np.array([3, b, n - 3], dtype=np.uint64)) for b in POSITIONS if 3 < b < n - 3]
    later = [(n, np.array([5, TILE + 1024], dtype=np.uint64)), (n, np.array([5, 2 * TILE + 16], dtype=np.uint64))]
    return one + two + later


def layout_two_joins():
    """4401 tiles, 9 boundaries: on 256 CUs the join's grid is 4096 workgroups, and workgroups 5, 105 and 125 take a second open tile"""
    T = TILE
    n = 4400 * T + 7
    return n, np.array([11, 5 * T + 100, 35 * T + 50, 105 * T + 7, 300 * T + 9, 4101 * T + 3, 4201 * T + 1, 4221 * T + 2, n - 3], dtype=np.uint64)


def layout_million_segments():
    """2^20 + 4099 segments, lengths 1, 0, 2, 0, 0, 1 over and over from off[0] = 5; 5 trailing elements"""
    S = (1 << 20) + 4099
    off = offsets_from(np.resize(np.array([1, 0, 2, 0, 0, 1], dtype=np.int64), S), start=5)
    return int(off[-1]) + 5, off


def chunk_of(n, cus=CUS):
    """tiles a workgroup of segreduce_tile_kernel walks"""
    tiles = (n + TILE - 1) // TILE
    return max((tiles + 16 * cus - 1) // (16 * cus), 1)


def join_grid(n, nseg, cus=CUS):
    """workgroups of segreduce_join_kernel: one thread per segment and one workgroup per tile, at most 16 per CU"""
    return min(max((nseg + JOIN - 1) // JOIN, (n + TILE - 1) // TILE, 1), 16 * cus)


def join_schedule(n, off, cus=CUS):
    """{workgroup: [(open tile, m)]} in the order the workgroup takes them: tile t is open if a segment that began in it goes on behind
    it, m = the tiles after t that the segment reaches; the workgroups take the tiles from off[0]'s on, grid-stride"""
    o = _offsets(n, off)
    grid = join_grid(n, len(o) - 1, cus)
    live = np.flatnonzero(o[1:] > o[:-1])
    t, u = o[live] // TILE, (o[live + 1] - 1) // TILE
    t_first = int(o[0]) // TILE
    out = {}
    for a, b in zip(t[u > t].tolist(), u[u > t].tolist()):
        out.setdefault((a - t_first) % grid, []).append((a, b - a))
    return out


def dense_paths(o):
    """how densely the segment starts lie (rsx_segreduce.hpp stores a segment between two flags of one thread at once, by ids.last)"""
    got = set()
    lengths = o[1:] - o[:-1]
    starts = o[:-1][lengths > 0]
    if starts.size:
        per_thread = np.bincount(starts // KPT)
        if per_thread.max() >= 3:
            got.add("three or more starts in a thread")
        if per_thread.max() == KPT:
            got.add("16 starts in a thread")
        if np.bincount(starts // TILE).max() == TILE:
            got.add("4096 starts in a tile")
        if np.any(starts % KPT == 0):
            got.add("boundary on a thread edge")
        if np.any(starts % KPT == 1):
            got.add("boundary one element behind a thread edge")
    empty = lengths == 0
    if empty.any() and lengths.size > 2:
        after_one = empty[1:] & (lengths[:-1] == 1)                # an empty segment right behind a one-element segment,
        before_one = empty[:-1] & (lengths[1:] == 1)               # and one right before a one-element segment
        if after_one.any() and before_one.any():
            got.add("empty between one-element segments")
    return got


def stop_paths(o):
    """where off[S] stands in its tile: the stop flag of segreduce_tile_kernel"""
    got = set()
    lo, hi = int(o[0]), int(o[-1])
    if lo < hi:
        if hi % KPT == 0 and hi % TILE != 0:
            got.add("stop on a thread edge inside a tile")
        if hi % TILE == 1:
            got.add("stop at a tile's second element")
        if hi % TILE == TILE - 1:
            got.add("stop at a tile's last element")
    return got


def paths(n, off):
    """the paths of rsx_segreduce.hpp that a layout reaches, from the layout alone"""
    o = _offsets(n, off)
    got = set()
    lo, hi = int(o[0]), int(o[-1])
    if (n + TILE - 1) // TILE > 16 * CUS:
        got.add("two tiles per workgroup")
    if lo > 0:
        got.add("off[0] > 0")
    if hi < n:
        got.add("off[S] < n")
    got |= dense_paths(o) | stop_paths(o)
    for s in range(len(o) - 1):
        b, e = int(o[s]), int(o[s + 1])
        if b == e:
            got.add("empty")
            if b == hi and b % TILE == 0 and b >= n:
                got.add("empty where no tile is")
            continue
        ta, tb = b // TILE, (e - 1) // TILE
        if e % TILE == 0:
            got.add("ends on a tile edge")
        if b % TILE == 0:
            got.add("boundary at a tile's first element")
        if b % TILE == TILE - 1:
            got.add("boundary at a tile's last element")
        if ta == tb:
            q0, q1 = (b % TILE) // KPT, ((e - 1) % TILE) // KPT
            got.add("inside a thread" if q0 == q1 else "inside a wave" if q0 // WAVE == q1 // WAVE else "inside a tile")
        else:
            m = tb - ta
            got.add("join: one wave" if m <= WAVE else "join: four waves" if m <= JOIN else "join: more than one partial per thread")
    return got
