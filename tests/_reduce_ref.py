"""Host referee of the reduce-by-key tests (rsx_segmented_reduce_by_key), built on tests/_unique_ref.py: the grouping (keys, run offsets,
counts, inverse) is unique_oracle's, the reduction runs over its inverse map, in two forms.

reduce_oracle   the numpy form: the elements are brought into run order by a stable argsort of their global run id and reduced with
                ufunc.reduceat.  Integers are summed as unsigned words of the value's own width (they wrap as the call's do); float32
                sums are taken in float64 and float64 sums in numpy's extended precision, and stay in that wider type; min / max are
                numpy's minimum / maximum, which return NaN if the run holds one.
slow_reduce     the same answer from a loop over the elements of every segment: Python integers masked to the width, math.fsum, and a
                NaN-aware comparison.
Both return unique_oracle's dict plus "values" (one per run, packed like keys) and, for float sums, "abs" (the sum of |v| of the run in
the wide type: what the error bound of a float sum is made of).  off None = one segment [0, n).
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


def reduce_oracle(x, v, off=None, op="sum", descending=False, consecutive=False):
    assert op in OPS and v.shape == x.shape
    u = unique_oracle(x, off, descending, consecutive)
    gid, lo, hi = _run_ids(u, off, x.size)
    total = int(u["run_offsets"][-1])
    out = dict(u)
    if total == 0:
        out["values"] = np.zeros(0, dtype=v.dtype)
        return out
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
