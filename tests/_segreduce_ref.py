"""Referee of the segmented reduction (rsx_segmented_reduce): plain numpy, no GPU and no library.

reduce_oracle   op over every segment, one slice at a time.  Integer sums wrap; float sums are taken in a wider format (float64 for
                float32, numpy's extended precision for float64) and returned in it; float min / max give NaN if the segment holds one;
                the arg ops give the FIRST position of the extreme, a NaN beating every number.  Empty segments: the identity, index -1.
model_sum       the association written at the top of rsx_segreduce.hpp, transcribed for float32 / float64 from the values, the offsets
                and n alone: the bits the kernels must produce.
reduce_terms    per segment: the elements folded and the sum of their magnitudes, for the any-order error bound.
The named layouts at the end are (n, offsets) pairs; paths() says, from a layout alone, which paths of the kernels it reaches.
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
