"""Host referee of the scan tests (rsx_segmented_scan).

restarts        the restart mask of the call: a position of [off[0], off[S]) that starts a non-empty segment or (keys given) whose key
                differs by bits from the key before it.  off None = one segment [0, n).
scan_oracle     one loop over the runs, ufunc.accumulate inside each.  Integer sums are taken on unsigned words of the value's own width
                (they wrap as the call's do); float32 sums are taken in float64 and float64 sums in numpy's extended precision and stay
                in that wider type; min / max are numpy's minimum / maximum.accumulate, which keep a NaN once they have met one.
flat_scan       the same answer without a loop over the runs: restart mask -> run ids -> a doubling scan (distances 1, 2, 4, ...) in which
                an element takes its partner in only if both carry the same run id.  Another association of a float sum: the two forms
                agree bit for bit wherever every order is exact, and that is where they are compared.
Both return an array of n entries; positions outside [off[0], off[S]) hold the input value (the call does not write them).  Exclusive:
a restart holds the identity, every other position the inclusive value of the position before.
scan_terms      (m, abs): per position the number of elements folded and the sum of their magnitudes in the wide type: what the error
                bound of a float sum is made of.

layouts         layout_deep (A), layout_long (B), layout_misaligned (C), layout_dense (D), layout_two_tiles (E): (n, offsets, keys) of the
                paths that tests/test_gpu_scan_paths.py runs, each from a fixed seed; tests/test_scan.py asserts, from the layout alone, that
                each still reaches the path it is named after.  keys_of_runs and tiny_values are their building blocks.

model_scan      the float sum in the value's OWN type and in the association that rsx_scan_by_key.hpp writes down (ORDER OF A FLOAT SUM):
                the device's bits, not a bound.  A function of the positions on the 4096-element tile grid, the restarts and the values
                alone: it takes no grid size and no tiles-per-workgroup.
"""
import numpy as np

OPS = ("sum", "min", "max")
WIDE = {np.dtype(np.float32): np.float64, np.dtype(np.float64): np.longdouble}
UNSIGNED = {np.dtype(np.int32): np.uint32, np.dtype(np.int64): np.uint64}
BITS = {1: np.uint8, 4: np.uint32, 8: np.uint64}
UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
TILE, THREADS, KPT, WAVE, BLOCK = 4096, 256, 16, 64, 1024      # rsx_scan_by_key.hpp: tile = 256 threads x 16, waves of 64, carry blocks of 1024 tiles


def identity(dtype, op):
    dtype = np.dtype(dtype)
    if op == "sum":
        return dtype.type(0)
    if dtype.kind == "f":
        return dtype.type(np.inf if op == "min" else -np.inf)
    return dtype.type(np.iinfo(dtype).max if op == "min" else np.iinfo(dtype).min)


def restarts(n, off=None, keys=None):
    """(mask over [0, n), lo, hi)"""
    off = np.array([0, n], dtype=np.int64) if off is None else np.asarray(off).astype(np.int64)
    lo, hi = int(off[0]), int(off[-1])
    mask = np.zeros(n, dtype=bool)
    starts = off[:-1][np.diff(off) > 0]                    # empty segments start nothing
    mask[starts] = True
    if keys is not None:
        b = np.ascontiguousarray(keys).view(BITS[keys.dtype.itemsize])
        mask[1:] |= b[1:] != b[:-1]
    mask[:lo] = False
    mask[hi:] = False
    return mask, lo, hi


def _work(values, op):
    """the array the referee computes in, and how to bring a result back"""
    dt = values.dtype
    if op == "sum" and dt.kind == "f":
        return values.astype(WIDE[dt])
    if op == "sum":
        return values.view(UNSIGNED[dt]).copy()
    return values.copy()


def _finish(res, values, op, exclusive, mask, lo, hi):
    dt = values.dtype
    wide = op == "sum" and dt.kind == "f"
    if op == "sum" and dt.kind == "i":
        res = res.view(dt)
    out = values.astype(WIDE[dt]) if wide else values.copy()
    if exclusive:
        shifted = np.empty_like(res)
        shifted[1:] = res[:-1]
        shifted[:1] = 0
        res = np.where(mask, out.dtype.type(identity(dt, op)), shifted)
    out[lo:hi] = res[lo:hi]
    return out


def scan_oracle(values, off=None, keys=None, op="sum", exclusive=False):
    assert op in OPS
    mask, lo, hi = restarts(values.size, off, keys)
    w = _work(values, op)
    res = w.copy()
    heads = np.flatnonzero(mask)
    ufunc = {"sum": np.add, "min": np.minimum, "max": np.maximum}[op]
    with np.errstate(all="ignore"):
        for a, b in zip(heads.tolist(), heads[1:].tolist() + [hi]):
            res[a:b] = ufunc.accumulate(w[a:b])
    return _finish(res, values, op, exclusive, mask, lo, hi)


def flat_scan(values, off=None, keys=None, op="sum", exclusive=False):
    assert op in OPS
    mask, lo, hi = restarts(values.size, off, keys)
    x = _work(values, op)
    rid = np.cumsum(mask)                                  # 0 before off[0]: those positions join nothing that is kept
    rid[:lo] = -1 - np.arange(lo)
    rid[hi:] = -1 - np.arange(hi, values.size) - lo
    ufunc = {"sum": np.add, "min": np.minimum, "max": np.maximum}[op]
    longest = int(np.diff(np.concatenate([np.flatnonzero(mask), [hi]])).max()) if hi > lo else 1
    d = 1
    with np.errstate(all="ignore"):
        while d < longest:
            same = rid[d:] == rid[:-d]
            x[d:] = np.where(same, ufunc(x[:-d], x[d:]), x[d:])
            d *= 2
    return _finish(x, values, op, exclusive, mask, lo, hi)


def scan_terms(values, off=None, keys=None, exclusive=False):
    """(m, abs): elements folded into every output and the sum of their magnitudes (wide type); 0 outside [off[0], off[S])"""
    mask, lo, hi = restarts(values.size, off, keys)
    pos = np.arange(values.size, dtype=np.int64)
    head = np.maximum.accumulate(np.where(mask, pos, -1))
    m = np.where(head >= 0, pos - head + 1, 0)
    m[hi:] = 0
    mag = scan_oracle(np.abs(values), off, keys, "sum", exclusive).astype(WIDE[values.dtype])
    mag[:lo] = 0
    mag[hi:] = 0
    if exclusive:
        m = np.where(m > 0, m - 1, 0)
    return m, mag


def same_values(a, b):
    """equal as numbers, or NaN on both sides"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def _flagged_hillis_steele(x, xf):
    """in place along the last axis (64 lanes): x[l] = x[l-d] o x[l] unless l holds a restart already, d = 1, 2, ... 32"""
    d = 1
    while d < WAVE:
        y, yf = x[..., :-d].copy(), xf[..., :-d].copy()
        x[..., d:] = np.where(xf[..., d:], x[..., d:], y + x[..., d:])
        xf[..., d:] |= yf
        d *= 2


def model_scan(values, off=None, keys=None, exclusive=False):
    """The running sum in values.dtype and in the order of rsx_scan_by_key.hpp; an array of n entries, positions outside
    [off[0], off[S]) hold the input value."""
    dt = values.dtype
    assert dt.kind == "f"
    mask, lo, hi = restarts(values.size, off, keys)
    out = values.copy()
    if lo >= hi:
        return out
    t_first, t_end = lo // TILE, (hi + TILE - 1) // TILE
    nt = t_end - t_first
    base = t_first * TILE
    v = np.zeros(nt * TILE, dtype=dt)                      # outside [off[0], off[S]): 0, no restart
    v[lo - base:hi - base] = values[lo:hi]
    r = np.zeros(nt * TILE, dtype=bool)
    r[lo - base:hi - base] = mask[lo:hi]
    with np.errstate(all="ignore"):
        # thread level: a[j], and whether a restart of the thread lies at or before j
        v2, r2 = v.reshape(-1, KPT), r.reshape(-1, KPT)
        a, cut = v2.copy(), r2.copy()
        for j in range(1, KPT):
            a[:, j] = np.where(r2[:, j], v2[:, j], a[:, j - 1] + v2[:, j])
            cut[:, j] = cut[:, j - 1] | r2[:, j]
        nthr = a.shape[0]

        # tile level: T(q) and whether a restart of the tile lies at or before the end of thread q
        x = a[:, KPT - 1].reshape(nt, THREADS // WAVE, WAVE).copy()
        xf = cut[:, KPT - 1].reshape(nt, THREADS // WAVE, WAVE).copy()
        _flagged_hillis_steele(x, xf)
        T, Tf = x.copy(), xf.copy()
        pv, pf = x[:, 0, WAVE - 1].copy(), xf[:, 0, WAVE - 1].copy()
        for w in range(1, THREADS // WAVE):
            T[:, w, :] = np.where(xf[:, w, :], x[:, w, :], pv[:, None] + x[:, w, :])
            Tf[:, w, :] = xf[:, w, :] | pf[:, None]
            tv, tf = x[:, w, WAVE - 1], xf[:, w, WAVE - 1]
            pv = np.where(tf, tv, pv + tv)
            pf = pf | tf
        T, Tf = T.reshape(-1), Tf.reshape(-1)
        tail, tailf = T[THREADS - 1::THREADS], Tf[THREADS - 1::THREADS]

        # grid level: blocks of 1024 tiles aligned on the global grid; after[k] = carry[t_first + k + 1]
        gbase = t_first // BLOCK * BLOCK
        nb = (t_end - gbase + BLOCK - 1) // BLOCK
        X = np.zeros(nb * BLOCK, dtype=dt)
        XF = np.zeros(nb * BLOCK, dtype=bool)
        X[t_first - gbase:t_end - gbase] = tail
        XF[t_first - gbase:t_end - gbase] = tailf
        X, XF = X.reshape(nb, BLOCK // WAVE, WAVE), XF.reshape(nb, BLOCK // WAVE, WAVE)
        _flagged_hillis_steele(X, XF)
        after = np.empty_like(X)
        run = dt.type(0)
        for b in range(nb):
            for w in range(BLOCK // WAVE):
                after[b, w, :] = np.where(XF[b, w, :], X[b, w, :], run + X[b, w, :])
                run = X[b, w, WAVE - 1] if XF[b, w, WAVE - 1] else dt.type(run + X[b, w, WAVE - 1])
        after = after.reshape(-1)[t_first - gbase:t_end - gbase]

        # F: thread level below the thread's end, tile level at it, grid level at the tile's end
        tq = np.arange(nthr) // THREADS
        tid = np.arange(nthr) % THREADS
        c = np.zeros(nt, dtype=dt)
        c[1:] = after[:-1]
        hasc = (np.arange(nt) > 0)[tq]
        c = c[tq]
        ex, exf = np.roll(T, 1), np.roll(Tf, 1)
        G = np.where(exf | ~hasc, ex, c + ex)
        gv = np.ones(nthr, dtype=bool)
        G = np.where(tid == 0, c, G)
        gv = np.where(tid == 0, hasc, gv)
        F = np.empty_like(a)
        for j in range(KPT - 1):
            F[:, j] = np.where(cut[:, j] | ~gv, a[:, j], G + a[:, j])
        F[:, KPT - 1] = np.where(tid == THREADS - 1, after[tq], np.where(Tf | ~hasc, T, c + T))
        F = F.reshape(-1)
        if exclusive:
            E = np.empty_like(F)
            E[1:] = F[:-1]
            E[0] = 0
            F = np.where(r, dt.type(0), E)
    out[lo:hi] = F[lo - base:hi - base]
    return out


# -- layouts of the paths (tests/test_gpu_scan_paths.py; tests/test_scan.py checks what each reaches) -----------------------------------------

RUNS = [1, 2, 17, 300, 4095, 4096, 4097, 6000]
CU_COUNTS = (256, 304)                                         # MI355X, MI300X: layout E must give two tiles per workgroup on both


def keys_of_runs(n, rng, dtype=np.uint32, choices=RUNS):
    """adjacent runs of lengths drawn from `choices`; neighbouring runs always differ"""
    lens = rng.choice(choices, size=n // min(choices) + 1)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), n)) + 1]
    return np.repeat(np.arange(lens.size) % 5 + 3, lens)[:n].astype(dtype)


def layout_deep(kdtype=None):
    """A: off[0] in tile 1000 (lane 40 of wave 15 of carry block 0), mid-tile; the first segment is a run of 70 tiles and a bit that crosses
    the carry-block edge at tile 1024.  With keys: constant but for one change at 1030 * TILE + 5."""
    start = 1000 * TILE + 2000
    n = start + 70 * TILE + 1011
    off = np.array([start, start + 70 * TILE + 1000, n - 5], dtype=np.uint64)
    keys = None
    if kdtype is not None:
        keys = np.full(n, 7, dtype=kdtype)
        keys[1030 * TILE + 5:] = 8
    return n, off, keys


def layout_long(deep=False):
    """B: one run of 1100 tiles, longer than a carry block: R enters block 1 as the fold of all 16 waves of block 0.  deep: off[0] in
    tile 5 (dead lanes 0 .. 4 of block 0, a first tile with elements before off[0]) and off[S] = n - 3."""
    n = 1100 * TILE + 77
    return n, (np.array([5 * TILE + 9, n - 3], dtype=np.uint64) if deep else None), None


def layout_misaligned():
    """C: tiles 1 and 2 are whole (the 16-byte paths where the pointer allows), tiles 0 and 3 are not"""
    n = 3 * TILE + 100
    return n, np.array([5, 2000, n - 7], dtype=np.uint64), None


def _lengths_summing_to(total, rng):
    """segment lengths drawn from {0, 0, 0, 1, 1, 2, 3} that sum to exactly `total`"""
    lens = rng.choice([0, 0, 0, 1, 1, 2, 3], size=4 * total + 64)
    cut = int(np.searchsorted(np.cumsum(lens), total))
    assert cut < lens.size
    lens = lens[:cut + 1].copy()
    lens[-1] -= int(lens.sum()) - total
    return lens


def layout_dense(kind="mixed", kdtype=None):
    """D: off[0] = TILE + 17 and about one offset per element.  "mixed": lengths from {0, 0, 0, 1, 1, 2, 3}, 5000 consecutive empty
    segments mid-tile and 5000 whose common offset is exactly 2 * TILE.  "ones": every segment has one element, every element is a restart.
    "empty" / "empty_edge": nine equal offsets mid-tile / on a tile edge, nothing in range although n > 0.  Keys: runs of 1 .. 3."""
    rng = np.random.default_rng(504)
    lo = TILE + 17
    if kind == "mixed":
        lens = np.concatenate([_lengths_summing_to(1500, rng), np.zeros(5000, dtype=np.int64), _lengths_summing_to(TILE - 17 - 1500, rng),
                               np.zeros(5000, dtype=np.int64), _lengths_summing_to(2 * TILE - 300, rng)])
        off = np.concatenate([[lo], lo + np.cumsum(lens)]).astype(np.uint64)
        n = 4 * TILE - 289
    elif kind == "ones":
        off = np.arange(lo, 3 * TILE + 51, dtype=np.uint64)
        n = 3 * TILE + 61
    else:
        off = np.full(9, lo if kind == "empty" else 2 * TILE, dtype=np.uint64)
        n = 4 * TILE - 289
    assert int(off[-1]) <= n
    return n, off, None if kdtype is None else keys_of_runs(n, rng, kdtype, [1, 2, 3])


def layout_two_tiles(cus, offsets=True):
    """E: the smallest n at which a workgroup walks two tiles (capi_scan.inc: ceil(tiles / (16 * CUs))), u64 keys of RUNS, and segments of
    up to three tiles from off[0] = 3 to off[S] = n - 7 (or no offsets)"""
    rng = np.random.default_rng(505)
    n = two_tiles_n(cus)
    keys = keys_of_runs(n, rng, np.uint64)
    off = None
    if offsets:
        lens = rng.integers(1, 3 * TILE, size=n // TILE)
        lens = lens[:int(np.searchsorted(np.cumsum(lens), n - 10))]
        off = np.concatenate([[3], 3 + np.cumsum(list(lens) + [n - 10 - int(lens.sum())])]).astype(np.uint64)
    return n, off, keys


def two_tiles_n(cus):
    return TILE * 16 * cus + 1


def runs_of(n, off=None, keys=None):
    """(starts, ends) of every run of the call, in order"""
    mask, lo, hi = restarts(n, off, keys)
    heads = np.flatnonzero(mask)
    return heads, np.concatenate([heads[1:], [hi]]).astype(heads.dtype) if heads.size else heads


def nan_sticks(res, lo, pos, end, hi, exclusive=False):
    """min / max of the run [lo, end) that meets its only NaN at `pos`: every later output of the run is NaN, none before is, and the
    first output after the run (if the call has one) is not"""
    first = pos + 1 if exclusive else pos
    return bool(np.isnan(res[first:end]).all() and not np.isnan(res[lo:first]).any() and (end >= hi or not np.isnan(res[end])))


def longest_run(n, off=None, keys=None):
    mask, lo, hi = restarts(n, off, keys)
    return int(np.diff(np.concatenate([np.flatnonzero(mask), [hi]])).max()) if hi > lo else 0


def tiny_values(vt, n, rng, longest=None):
    """Floats around the bottom of the normal range.  longest None: general values, subnormal up to a few binades above finfo.tiny, so that
    partial sums move in and out of the subnormal range and round there.  longest = the longest run of the layout: multiples k * q of the
    smallest subnormal q, |k| small, and +-tiny alternating every 1000th element; any window holds a net of at most one tiny, so every
    partial sum of a run is a multiple of q below 2 * tiny, which is representable: every order of the sum is exact, and the sums
    cross tiny both ways."""
    vt = np.dtype(vt)
    fi = np.finfo(vt)
    if longest is None:
        return (rng.standard_normal(n) * 2.0 ** rng.integers(-8, 4, n)).astype(vt) * vt.type(fi.tiny)
    q = float(fi.smallest_subnormal)
    per_tiny = int(round(float(fi.tiny) / q))                  # 2^23 / 2^52
    kmax = min(per_tiny // max(longest, 1), 1 << 20)
    assert kmax >= 1 and per_tiny + longest * kmax <= 2 * per_tiny
    k = rng.integers(-kmax, kmax + 1, n).astype(np.float64)
    big = np.arange(0, n, 1000)
    k[big] = np.where(np.arange(big.size) % 2 == 0, 1.0, -1.0) * per_tiny
    return (k * q).astype(vt)
