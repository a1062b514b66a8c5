"""Host referee of the select tests (rsx_segmented_select): numpy's stable argsort of the order-mapped keys, as topk_oracle, in two forms.

select_oracle   the argsort form: entry ranks[s, q] of seg_oracle's stable sort of every valid segment.
fast_select     the same answer without sorting, for the big shapes: per (segment, rank) np.argpartition of the order-mapped keys
                gives the key at the rank; the wanted element is the (rank - #strictly better)-th of its ties in index order.
Both return (keys [S, R] unsigned words, pos [S, R] uint32, written [S, R] bool); `written` marks the slots the call writes (a rank not
below its segment's length, and every slot of an invalid segment, keeps the caller's contents).
"""
import numpy as np

from test_gpu_float_keys import UINT, enc
from test_gpu_segmented import seg_oracle

NONE = 0xFFFFFFFF        # the conventional "no rank"


def _ranks2d(ranks, nseg):
    r = np.asarray(ranks, dtype=np.uint32)
    return r.reshape(nseg, -1)


def select_oracle(x: np.ndarray, off, ranks, descending: bool = False):
    n = x.size
    off = np.asarray(off, dtype=np.int64)
    nseg = len(off) - 1
    r = _ranks2d(ranks, nseg)
    u = UINT[x.dtype]
    order = seg_oracle(x, off, n, descending)
    keys = np.zeros(r.shape, dtype=u)
    pos = np.zeros(r.shape, dtype=np.uint32)
    written = np.zeros(r.shape, dtype=bool)
    for s in range(nseg):
        a, b = int(off[s]), int(off[s + 1])
        if not (a <= b <= n):
            continue
        for q in range(r.shape[1]):
            if int(r[s, q]) < b - a:
                src = order[a + int(r[s, q])]
                keys[s, q] = x[src:src + 1].view(u)[0]
                pos[s, q] = src - a
                written[s, q] = True
    return keys, pos, written


def fast_select(x: np.ndarray, off, ranks, descending: bool = False):
    n = x.size
    off = np.asarray(off, dtype=np.int64)
    nseg = len(off) - 1
    r = _ranks2d(ranks, nseg)
    u = UINT[x.dtype]
    xu = x.view(u)
    e = enc(x)                      # fast_topk's order map (tests/_topk_ref.py): the smallest word is the best key
    if descending:
        e = ~e
    keys = np.zeros(r.shape, dtype=u)
    pos = np.zeros(r.shape, dtype=np.uint32)
    written = np.zeros(r.shape, dtype=bool)
    for s in range(nseg):
        a, b = int(off[s]), int(off[s + 1])
        if not (a <= b <= n) or a == b:
            continue
        es = e[a:b]
        for q in range(r.shape[1]):
            rk = int(r[s, q])
            if rk >= b - a:
                continue
            kth = es[np.argpartition(es, rk)[rk]]
            better = int(np.count_nonzero(es < kth))
            p = int(np.flatnonzero(es == kth)[rk - better])
            keys[s, q] = xu[a + p]
            pos[s, q] = p
            written[s, q] = True
    return keys, pos, written


def random_ranks(off, R: int, rng, n: int | None = None) -> np.ndarray:
    """[S, R] uint32: random valid ranks in random order, with the edge ranks 0, L - 1, L and 0xFFFFFFFF and duplicates mixed in."""
    off = np.asarray(off, dtype=np.int64)
    nseg = len(off) - 1
    out = np.empty((nseg, R), dtype=np.uint32)
    for s in range(nseg):
        L = int(off[s + 1]) - int(off[s])
        L = L if L > 0 and (n is None or int(off[s + 1]) <= n) else 1
        row = rng.integers(0, L, R).astype(np.int64)
        edge = [0, L - 1, L, NONE, int(row[0]), L // 2]
        for q in range(R):
            if rng.random() < 0.4:
                row[q] = edge[int(rng.integers(0, len(edge)))]
        out[s] = row.astype(np.uint32)
    return out
