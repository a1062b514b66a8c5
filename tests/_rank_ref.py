"""The referee of rsx_segmented_rank (tests/test_rank.py, tests/test_gpu_rank.py): a stable argsort of the encoded keys of every segment,
then the five tie rules from the boundaries of the runs of equal keys.  numpy only; written from the contract in include/radixsort_hip.h
and independent of csrc/rsx_rank_math.hpp (no tiles, no carries).

Order: the unsigned order of encode(x) is the engine's ascending order: unsigned keys as they are, signed keys with the sign bit flipped,
floats in IEEE 754 totalOrder (negative: all bits flipped, else the sign bit flipped); descending is the complement.  Keys tie iff their
bits are equal, which is equality of the encoded keys."""
import numpy as np

ORDINAL, MIN, MAX, DENSE, AVERAGE = 0, 1, 2, 3, 4
METHODS = {"ordinal": ORDINAL, "min": MIN, "max": MAX, "dense": DENSE, "average": AVERAGE}
TILE = 4096
_UINT = {4: np.uint32, 8: np.uint64}


def encode(x, descending=False):
    x = np.ascontiguousarray(x)
    u = _UINT[x.dtype.itemsize]
    bits = x.view(u)
    top = u(1) << u(8 * x.dtype.itemsize - 1)
    if x.dtype.kind == "f":
        e = np.where(bits & top, ~bits, bits ^ top)
    elif x.dtype.kind == "i":
        e = bits ^ top
    else:
        e = bits.copy()
    return ~e if descending else e


def rank_segment(x, descending=False):
    """(ranks [5, L] uint32 by method code, ties [L] uint32) of one segment"""
    L = len(x)
    e = encode(x, descending)
    order = np.argsort(e, kind="stable")
    s = e[order]
    head = np.ones(L, dtype=bool)
    head[1:] = s[1:] != s[:-1]
    run = np.cumsum(head) - 1                              # the run of every sorted position
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], L)
    lo, hi = starts[run], ends[run]
    by_sorted = np.stack([np.arange(L), lo, hi - 1, run, lo + hi - 1]).astype(np.uint32)
    ranks = np.empty((5, L), dtype=np.uint32)
    ranks[:, order] = by_sorted
    ties = np.empty(L, dtype=np.uint32)
    ties[order] = (hi - lo).astype(np.uint32)
    return ranks, ties


def rank_oracle(x, off, descending=False, fill=0):
    """(ranks [5, n] uint32, ties [n] uint32, written [n] bool) of the whole call: `fill` where nothing is written.  off None: one segment."""
    n = len(x)
    ranks = np.full((5, n), fill, dtype=np.uint32)
    ties = np.full(n, fill, dtype=np.uint32)
    written = np.zeros(n, dtype=bool)
    o = np.array([0, n], dtype=np.int64) if off is None else np.asarray(off).astype(np.int64)
    for a, b in zip(o[:-1], o[1:]):
        if b > a:
            ranks[:, a:b], ties[a:b] = rank_segment(x[a:b], descending)
            written[a:b] = True
    return ranks, ties, written


def sorted_keys_layout(x, off, descending=False):
    """Per large segment (> TILE keys) the encoded keys in sorted order with the segment's start: what the tile kernels see."""
    o = np.asarray(off).astype(np.int64)
    return [(int(a), np.sort(encode(x[a:b], descending), kind="stable")) for a, b in zip(o[:-1], o[1:]) if b - a > TILE]


def tile_facts(a, s):
    """For a sorted large segment that starts at global index a: (a run of equal keys crosses a boundary of the global TILE grid,
    some tile of the grid clipped at the segment's ends holds no head)"""
    L = len(s)
    head = np.ones(L, dtype=bool)
    head[1:] = s[1:] != s[:-1]
    edges = np.arange((a // TILE + 1) * TILE, a + L, TILE) - a        # positions inside the segment where a new tile begins
    crossing = bool(np.any(~head[edges]))
    bounds = np.concatenate([[0], edges, [L]])
    headless = any(not head[p:q].any() for p, q in zip(bounds[:-1], bounds[1:]) if q > p)
    return crossing, headless
