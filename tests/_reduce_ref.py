"""Host referee of the reduce-by-key tests (rsx_segmented_reduce_by_key), built on tests/_unique_ref.py: the grouping (keys, run offsets,
counts, inverse) is unique_oracle's, the reduction runs over its inverse map, in two forms.

reduce_oracle   the numpy form: the elements are brought into run order by a stable argsort of their global run id and reduced with
                ufunc.reduceat.  Integers are summed as unsigned words of the value's own width (they wrap as the call's do); float32
                sums are taken in float64 and float64 sums in numpy's extended precision, and stay in that wider type; min / max are
                numpy's minimum / maximum, which return NaN if the run holds one.
slow_reduce     the same answer from a loop over the elements of every segment: Python integers masked to the width, math.fsum, and a
                NaN-aware comparison.
Both return unique_oracle's dict plus "values" (one per run, packed like keys) and, for float sums, "abs" (the sum of |v| of the run in
the wide type: what the error bound of a float sum is made of).  off None = one segment [0, n).  reduce_oracle takes a precomputed
grouping (`groups`: unique_oracle's or flat_unique's dict) so that large cases group once.

model_sum       the float sum in the value's OWN type and in the association that rsx_reduce.hpp writes down (ORDER OF A FLOAT SUM): the
                device's bits, not a bound.  A function of the grouped order, the head positions and the values alone.
"""
import math

import numpy as np

from _unique_ref import slow_unique, unique_oracle

OPS = ("sum", "min", "max")
WIDE = {np.dtype(np.float32): np.float64, np.dtype(np.float64): np.longdouble}
UNSIGNED = {np.dtype(np.int32): np.uint32, np.dtype(np.int64): np.uint64}


def _run_ids(u, off, n):
    """global run id of every element of [off[0], off[S]) (and those positions)"""
    off = np.array([0, n], dtype=np.int64) if off is None else np.asarray(off, dtype=np.int64)
    lo, hi = int(off[0]), int(off[-1])
    seg = np.repeat(np.arange(len(off) - 1), np.diff(off))
    gid = u["run_offsets"][seg].astype(np.int64) + u["inverse"][lo:hi].astype(np.int64)
    return gid, lo, hi


def reduce_oracle(x, v, off=None, op="sum", descending=False, consecutive=False, groups=None):
    assert op in OPS and v.shape == x.shape
    u = unique_oracle(x, off, descending, consecutive) if groups is None else groups
    total = int(u["run_offsets"][-1])
    out = dict(u)
    if total == 0:
        out["values"] = np.zeros(0, dtype=v.dtype)
        if op == "sum" and v.dtype.kind == "f":
            out["values"] = np.zeros(0, dtype=WIDE[v.dtype])
            out["abs"] = np.zeros(0, dtype=WIDE[v.dtype])
        return out
    if "order" in u:                                  # flat_unique: the run order is the grouped order it sorted into
        lo = int(u["heads"][0])
        hi = lo + u["order"].size
        order = u["order"] - lo
    else:
        gid, lo, hi = _run_ids(u, off, x.size)
        order = np.argsort(gid, kind="stable")
    vs = v[lo:hi][order]
    starts = np.concatenate([[0], np.cumsum(u["counts"].astype(np.int64))[:-1]])
    if op == "sum" and v.dtype.kind == "f":
        wide = vs.astype(WIDE[v.dtype])
        out["values"] = np.add.reduceat(wide, starts)
        out["abs"] = np.add.reduceat(np.abs(wide), starts)
    elif op == "sum":
        out["values"] = np.add.reduceat(vs.view(UNSIGNED[v.dtype]), starts, dtype=UNSIGNED[v.dtype]).view(v.dtype)
    else:
        with np.errstate(invalid="ignore"):
            out["values"] = (np.minimum if op == "min" else np.maximum).reduceat(vs, starts)
    return out


def slow_reduce(x, v, off=None, op="sum", descending=False, consecutive=False):
    assert op in OPS and v.shape == x.shape
    u = slow_unique(x, off, descending, consecutive)
    gid, lo, hi = _run_ids(u, off, x.size)
    total = int(u["run_offsets"][-1])
    runs = [[] for _ in range(total)]
    for g, val in zip(gid.tolist(), v[lo:hi].tolist()):
        runs[g].append(val)
    out = dict(u)
    if op == "sum" and v.dtype.kind == "f":
        out["values"] = np.array([math.fsum(r) for r in runs], dtype=WIDE[v.dtype])
        out["abs"] = np.array([math.fsum(abs(t) for t in r) for r in runs], dtype=WIDE[v.dtype])
    elif op == "sum":
        bits = v.dtype.itemsize * 8
        words = [sum(r) & ((1 << bits) - 1) for r in runs]
        out["values"] = np.array(words, dtype=UNSIGNED[v.dtype]).view(v.dtype)
    else:
        def pick(r):
            best = r[0]
            for t in r[1:]:
                if best != best:
                    break
                if t != t or (t < best if op == "min" else t > best):
                    best = t
            return best
        out["values"] = np.array([pick(r) for r in runs], dtype=v.dtype)
    return out


def same_values(a, b):
    """equal as numbers, or NaN on both sides"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


TILE, THREADS, KPT, WAVE = 4096, 256, 16, 64          # rsx_reduce.hpp: one tile = 256 threads x 16 elements, waves of 64 lanes


def _carry(tail, leads, oks, dt):
    """reduce_carry_kernel for one tile: lane l folds leads[l], leads[l + 64], ... left to right; the lane partials are joined by a tree
    (distances 1 .. 32, the lower lane on the left); the tail goes on the left of that"""
    part = np.zeros(WAVE, dtype=dt)
    has = np.zeros(WAVE, dtype=bool)
    for c in range(0, len(leads), WAVE):
        x, ok = leads[c:c + WAVE], oks[c:c + WAVE]
        m = x.size
        part[:m] = np.where(ok, np.where(has[:m], part[:m] + x, x), part[:m])
        has[:m] |= ok
    d = 1
    while d < WAVE:
        y, yh = part[d:].copy(), has[d:].copy()
        part[:WAVE - d] = np.where(yh, np.where(has[:WAVE - d], part[:WAVE - d] + y, y), part[:WAVE - d])
        has[:WAVE - d] |= yh
        d *= 2
    return dt.type(tail + part[0]) if has[0] else tail


def model_sum(values: np.ndarray, order: np.ndarray, heads: np.ndarray) -> np.ndarray:
    """The sum of every run in the association of rsx_reduce.hpp, in values.dtype.  order[i] = the original position of grouped element
    lo + i (the stable sort's positions; the identity from lo in consecutive mode), lo = heads[0]; heads = the grouped positions on the
    global grid that begin a run.  The grouped range is [lo, lo + len(order)).  One result per head.

    Inside a tile of 4096 = 256 threads x 16: a thread folds its 16 left to right, closing a run at every head; the threads' open ends are
    joined by a head-flagged Hillis-Steele scan over the 64 lanes of a wave (distances 1 .. 32), the four wave totals left to right.
    What a tile holds before its first head is its lead, from its last head on its tail; a run that leaves its tile is
    tail o (the following leads joined as in _carry)."""
    dt = values.dtype
    heads = np.asarray(heads, dtype=np.int64)
    out = np.zeros(heads.size, dtype=dt)
    done = np.zeros(heads.size, dtype=np.int64)
    if heads.size == 0:
        return out
    lo = int(heads[0])
    hi = lo + order.size
    t_lo, t_end = lo // TILE, (hi + TILE - 1) // TILE
    nt = t_end - t_lo
    base = t_lo * TILE
    v = np.zeros(nt * TILE, dtype=dt)
    v[lo - base:hi - base] = values[order]
    head = np.zeros(nt * TILE, dtype=bool)
    head[heads - base] = True
    flag = head.copy()
    if hi - base < nt * TILE:
        flag[hi - base] = True                            # the stop at off[S]: what follows it belongs to no run
    gid = np.cumsum(head) - 1                             # run id of the head last passed

    def store(g, val):
        out[g] = val
        np.add.at(done, g, 1)

    with np.errstate(all="ignore"):
        # 1. the thread's 16, left to right
        v2, f2 = v.reshape(-1, KPT), flag.reshape(-1, KPT)
        nthr = v2.shape[0]
        first_pos = np.arange(nthr, dtype=np.int64) * KPT
        acc, pre = v2[:, 0].copy(), v2[:, 0].copy()
        seen = f2[:, 0].copy()
        for j in range(1, KPT):
            fl = f2[:, j]
            closed = fl & seen                            # an earlier flag in this thread: a whole run
            if closed.any():
                store(gid[first_pos[closed] + j - 1], acc[closed])
            pre = np.where(fl & ~seen, acc, pre)
            acc = np.where(fl, v2[:, j], acc + v2[:, j])
            seen = seen | fl
        f = seen
        pre = np.where(f, pre, acc)
        has_pre = ~f2[:, 0]

        # 2. the flagged inclusive scan over the lanes of every wave, the wave totals folded left to right
        x = acc.reshape(nt, THREADS // WAVE, WAVE).copy()
        xf = f.reshape(nt, THREADS // WAVE, WAVE).copy()
        d = 1
        while d < WAVE:
            y, yf = x[:, :, :-d].copy(), xf[:, :, :-d].copy()
            x[:, :, d:] = np.where(xf[:, :, d:], x[:, :, d:], y + x[:, :, d:])
            xf[:, :, d:] |= yf
            d *= 2
        ex = np.zeros_like(x)
        exf = np.zeros_like(xf)
        ex[:, :, 1:], exf[:, :, 1:] = x[:, :, :-1], xf[:, :, :-1]
        pv, pf = x[:, 0, WAVE - 1].copy(), xf[:, 0, WAVE - 1].copy()
        for w in range(1, THREADS // WAVE):
            ex[:, w, 0], exf[:, w, 0] = pv, pf
            ex[:, w, 1:] = np.where(exf[:, w, 1:], ex[:, w, 1:], pv[:, None] + ex[:, w, 1:])
            exf[:, w, 1:] |= pf[:, None]
            tv, tf = x[:, w, WAVE - 1], xf[:, w, WAVE - 1]
            pv = np.where(tf, tv, pv + tv)
            pf = pf | tf
        ex, exf = ex.reshape(-1), exf.reshape(-1)

        # 3. the run that a thread's first flag ends: a run of this tile, or the tile's lead
        tid = np.arange(nthr) % THREADS
        closed = np.where(tid == 0, pre, np.where(has_pre, ex + pre, ex))
        inside = f & (tid > 0) & exf
        store(gid[first_pos[inside] - 1], closed[inside])
        lead = np.zeros(nt, dtype=dt)
        to_lead = f & ~inside                             # at most one per tile: the thread of the tile's first flag
        lead[np.flatnonzero(to_lead) // THREADS] = closed[to_lead]
        last = np.arange(nt) * THREADS + THREADS - 1
        whole = np.where(f[last], acc[last], ex[last] + acc[last])
        allf = f[last] | exf[last]
        tail = whole.copy()
        lead = np.where(allf, lead, whole)
        lead_ok = ~flag[::TILE]                           # the tile's very first element is not flagged
        tile_end = base + (np.arange(nt) + 1) * TILE
        has_tail = allf & (tile_end <= hi)                # off[S] inside the tile: the tail belongs to no run

        # the carry: tail[t] o lead[t + 1] o ... up to and including the first later tile that has a flag
        stops = np.flatnonzero(allf)
        for t in np.flatnonzero(has_tail):
            k = int(np.searchsorted(stops, t + 1))
            stop = int(stops[k]) if k < stops.size else nt - 1
            store(gid[(t + 1) * TILE - 1], _carry(tail[t], lead[t + 1:stop + 1], lead_ok[t + 1:stop + 1], dt))
    assert (done == 1).all(), "model_sum: a run was stored %s" % ("twice" if (done > 1).any() else "never")
    return out
