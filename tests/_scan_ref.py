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
