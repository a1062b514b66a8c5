"""Host referee of rsx_segmented_set_op (no GPU, no library): two independent forms of the same definition.

A key x occurs m times in A_s and n times in B_s; its occurrences on each side are numbered r = 0, 1, ... in input order.
  intersection           the A occurrences r < n                                  min(m, n), all from A
  difference             the A occurrences r >= n                                 max(m - n, 0)
  union                  every A occurrence and the B occurrences r >= m          max(m, n)
  symmetric difference   the A occurrences r >= n and the B occurrences r >= m    |m - n|
The kept elements of segment s come in the order of the stable merge of A_s ++ B_s (A before equal B) and are packed densely across
segments; koff[s] is the number kept before segment s.  index is the position in A_s ++ B_s (below La: from A); match, for the
intersection, the position relative to boff[s] of B's occurrence r of x for the kept A occurrence r.

  setop_oracle        vectorised per segment: np.searchsorted on order-mapped keys gives the rank among equals (i - left) and the count on
                      the other side (right - left); the kept elements are ordered by merge_oracle's rule (a stable argsort of the
                      order-mapped concatenation)
  setop_two_pointer   the textbook std::set_* loops

Offsets None on both sides: one segment [0, na) and [0, nb).  Both need sorted segments.
"""
import numpy as np

from _merge_ref import _offsets
from _search_ref import order_map

INTERSECTION, DIFFERENCE, UNION, SYMMETRIC_DIFFERENCE = 0, 1, 2, 3
OPS = (INTERSECTION, DIFFERENCE, UNION, SYMMETRIC_DIFFERENCE)
OP_NAMES = {INTERSECTION: "intersection", DIFFERENCE: "difference", UNION: "union", SYMMETRIC_DIFFERENCE: "symmetric_difference"}


def capacity(op, na, nb):
    """the elements the caller provides per output: what only A can supply needs na, the others na + nb"""
    return na if op in (INTERSECTION, DIFFERENCE) else na + nb


def _keep_masks(ea, eb, op):
    """(keep of A, keep of B, match of A) of one segment from its order-mapped keys"""
    la_left = np.searchsorted(ea, ea, side="left")
    ra = np.arange(ea.size) - la_left                                            # rank among equals on A's side
    b_left, b_right = np.searchsorted(eb, ea, side="left"), np.searchsorted(eb, ea, side="right")
    hit_a = ra < (b_right - b_left)
    rb = np.arange(eb.size) - np.searchsorted(eb, eb, side="left")
    hit_b = rb < (np.searchsorted(ea, eb, side="right") - np.searchsorted(ea, eb, side="left"))
    if op == INTERSECTION:
        return hit_a, np.zeros(eb.size, dtype=bool), b_left + ra
    if op == DIFFERENCE:
        return ~hit_a, np.zeros(eb.size, dtype=bool), None
    if op == UNION:
        return np.ones(ea.size, dtype=bool), ~hit_b, None
    assert op == SYMMETRIC_DIFFERENCE
    return ~hit_a, ~hit_b, None


def setop_oracle(a, aoff, b, boff, op, descending=False):
    """(keys, index, match, koff): index and match int64; match is None unless op is the intersection"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    aoff, boff = _offsets(a, aoff, b, boff)
    S = aoff.size - 1
    keys, index, match, koff = [], [], [], np.zeros(S + 1, dtype=np.int64)
    for s in range(S):
        sa, sb = a[aoff[s]:aoff[s + 1]], b[boff[s]:boff[s + 1]]
        ea, eb = order_map(sa, descending), order_map(sb, descending)
        keep_a, keep_b, m = _keep_masks(ea, eb, op)
        cat = np.concatenate([sa, sb])
        order = np.argsort(np.concatenate([ea, eb]), kind="stable")            # merge_oracle's index: positions in A_s ++ B_s
        kept = order[np.concatenate([keep_a, keep_b])[order]]
        keys.append(cat[kept])
        index.append(kept)
        if m is not None:
            match.append(m[kept])                                                # (every kept element of the intersection is A's)
        koff[s + 1] = koff[s] + kept.size
    cat_or = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return cat_or(keys, a.dtype), cat_or(index, np.int64), (cat_or(match, np.int64) if op == INTERSECTION else None), koff


def setop_two_pointer(a, aoff, b, boff, op, descending=False):
    """the same by the loops of std::set_intersection / set_difference / set_union / set_symmetric_difference"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    aoff, boff = _offsets(a, aoff, b, boff)
    S = aoff.size - 1
    keys, index, match, koff = [], [], [], np.zeros(S + 1, dtype=np.int64)
    for s in range(S):
        sa, sb = a[aoff[s]:aoff[s + 1]], b[boff[s]:boff[s + 1]]
        ea, eb = order_map(sa, descending).tolist(), order_map(sb, descending).tolist()
        la, lb = len(ea), len(eb)
        i = j = 0
        before = len(keys)
        while i < la or j < lb:
            if j >= lb or (i < la and ea[i] < eb[j]):                            # only A has it
                if op != INTERSECTION:
                    keys.append(sa[i]); index.append(i); match.append(-1)
                i += 1
            elif i >= la or eb[j] < ea[i]:                                       # only B has it
                if op in (UNION, SYMMETRIC_DIFFERENCE):
                    keys.append(sb[j]); index.append(la + j); match.append(-1)
                j += 1
            else:                                                                # a pair: std::set_* copies A's and steps both
                if op in (INTERSECTION, UNION):
                    keys.append(sa[i]); index.append(i); match.append(j)
                i += 1
                j += 1
        koff[s + 1] = koff[s] + len(keys) - before
    k = np.array(keys, dtype=a.dtype) if keys else np.zeros(0, dtype=a.dtype)
    return k, np.array(index, dtype=np.int64), (np.array(match, dtype=np.int64) if op == INTERSECTION else None), koff


def key_counts(e):
    """{order-mapped key: count}"""
    u, c = np.unique(e, return_counts=True)
    return dict(zip(u.tolist(), c.tolist()))


def expected_count(op, m, n):
    return {INTERSECTION: min(m, n), DIFFERENCE: max(m - n, 0), UNION: max(m, n), SYMMETRIC_DIFFERENCE: abs(m - n)}[op]
