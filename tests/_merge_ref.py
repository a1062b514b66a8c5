"""Host referee of rsx_segmented_merge (no GPU, no library): two independent forms of the same definition, the split rule the kernels
copy, and the grid stated at the top of radix-sort_amd/csrc/rsx_merge.hpp.

Output segment s is the stable sort, in the engine's order (unsigned order of order_map(key)), of the concatenation A_s ++ B_s, packed
densely from 0: ooff[s] = (aoff[s] - aoff[0]) + (boff[s] - boff[0]).  index[ooff[s] + r] is the position in that concatenation.

  merge_oracle        a stable argsort of the order-mapped concatenation, segment by segment (any input)
  merge_two_pointer   the two-pointer merge with the tie rule "A before equal B" (needs sorted segments)
  diagonal_split      the split rule: how many of the first d outputs of a segment come from A
  tile_sources        per tile of 4096 OUTPUT positions, the contiguous ranges of A and of B it reads
  thread_paths        per tile, which of its 256 threads (16 consecutive outputs each) are 'serial' (all 16 in one segment) and which
                      'runs' (a segment boundary among the 16: one search per segment touched); None for a thread without outputs

Offsets None on both sides: one segment [0, na) and [0, nb).
"""
import numpy as np

from _search_ref import order_map

TILE = 4096
THREADS = 256
KPT = 16


def _offsets(a, aoff, b, boff):
    if aoff is None:
        assert boff is None, "one offsets array without the other"
        return np.array([0, len(a)], dtype=np.int64), np.array([0, len(b)], dtype=np.int64)
    aoff, boff = np.asarray(aoff).astype(np.int64), np.asarray(boff).astype(np.int64)
    assert aoff.size == boff.size
    return aoff, boff


def out_offsets(aoff, boff):
    return (aoff - aoff[0]) + (boff - boff[0])


def merge_oracle(a, aoff, b, boff, descending=False):
    """(keys, index, ooff): keys[ooff[s] : ooff[s+1]] = the stable sort of A_s ++ B_s, index (int64) the positions in A_s ++ B_s"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    aoff, boff = _offsets(a, aoff, b, boff)
    ooff = out_offsets(aoff, boff)
    keys = np.empty(int(ooff[-1]), dtype=a.dtype)
    index = np.empty(int(ooff[-1]), dtype=np.int64)
    for s in range(aoff.size - 1):
        cat = np.concatenate([a[aoff[s]:aoff[s + 1]], b[boff[s]:boff[s + 1]]])
        order = np.argsort(order_map(cat, descending), kind="stable")
        keys[ooff[s]:ooff[s + 1]] = cat[order]
        index[ooff[s]:ooff[s + 1]] = order
    return keys, index, ooff


def merge_two_pointer(a, aoff, b, boff, descending=False):
    """the same by the textbook merge: take from A while its head is <= B's head"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    aoff, boff = _offsets(a, aoff, b, boff)
    ooff = out_offsets(aoff, boff)
    keys = np.empty(int(ooff[-1]), dtype=a.dtype)
    index = np.empty(int(ooff[-1]), dtype=np.int64)
    for s in range(aoff.size - 1):
        sa, sb = a[aoff[s]:aoff[s + 1]], b[boff[s]:boff[s + 1]]
        ea, eb = order_map(sa, descending).tolist(), order_map(sb, descending).tolist()
        i = j = 0
        o = int(ooff[s])
        while i < len(ea) or j < len(eb):
            if j >= len(eb) or (i < len(ea) and ea[i] <= eb[j]):
                keys[o], index[o] = sa[i], i
                i += 1
            else:
                keys[o], index[o] = sb[j], len(ea) + j
                j += 1
            o += 1
    return keys, index, ooff


def diagonal_split(enc_a, enc_b, d):
    """THE SPLIT RULE of rsx_merge.hpp: the partition point over [max(0, d - Lb), min(d, La)] of m -> enc_a[m] <= enc_b[d - 1 - m], by the
    kernel's bisection.  The first d outputs of the merge are enc_a[:i] and enc_b[:d - i]."""
    la, lb = len(enc_a), len(enc_b)
    assert 0 <= d <= la + lb
    lo, hi = max(0, d - lb), min(d, la)
    while lo < hi:
        mid = (lo + hi) // 2
        if enc_a[mid] <= enc_b[d - 1 - mid]:
            lo = mid + 1
        else:
            hi = mid
    return lo


def segment_of(ooff, p):
    """the largest s with ooff[s] <= p: for p < ooff[S] the segment that holds output position p (empty segments are skipped)"""
    return int(np.searchsorted(ooff[:-1], p, side="right")) - 1


def tile_splits(a, aoff, b, boff, descending=False, T=TILE):
    """split[t] = (s, A position) of every tile boundary t = 0 .. tiles of the grid over na + nb, as merge_split_kernel stores it"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    aoff, boff = _offsets(a, aoff, b, boff)
    ooff = out_offsets(aoff, boff)
    S, total = aoff.size - 1, int(ooff[-1])
    ea, eb = order_map(a, descending), order_map(b, descending)
    tiles = -(-(len(a) + len(b)) // T)
    out = []
    for t in range(tiles + 1):
        p = t * T
        if p >= total:
            out.append((S, int(aoff[S])))
            continue
        s = segment_of(ooff, p)
        i = diagonal_split(ea[aoff[s]:aoff[s + 1]], eb[boff[s]:boff[s + 1]], p - int(ooff[s]))
        out.append((s, int(aoff[s]) + i))
    return out


def tile_sources(a, aoff, b, boff, descending=False, T=TILE):
    """[(a_start, a_end, b_start, b_end)] of every live tile: the contiguous ranges of A and of B whose merge is the tile's outputs"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    splits = tile_splits(a, aoff, b, boff, descending, T)
    aoff, boff = _offsets(a, aoff, b, boff)
    total = int(out_offsets(aoff, boff)[-1])
    a0, b0 = int(aoff[0]), int(boff[0])
    out = []
    for t in range(len(splits) - 1):
        p0 = t * T
        if p0 >= total:
            break
        p1 = min(p0 + T, total)
        ai0 = splits[t][1]
        n_a = min(splits[t + 1][1] - ai0, p1 - p0) if splits[t + 1][1] > ai0 else 0
        bi0 = b0 + p0 - (ai0 - a0)
        out.append((ai0, ai0 + n_a, bi0, bi0 + (p1 - p0) - n_a))
    return out


def thread_paths(aoff, boff, na=None, nb=None, T=TILE):
    """[(single, [path of thread 0 .. 255])] of every live tile.  single: the tile lies inside one segment (no thread looks for its
    segment).  path: 'serial', 'runs' or None.  From the offsets alone."""
    if aoff is None:
        aoff, boff = np.array([0, na], dtype=np.int64), np.array([0, nb], dtype=np.int64)
    aoff, boff = np.asarray(aoff).astype(np.int64), np.asarray(boff).astype(np.int64)
    ooff = out_offsets(aoff, boff)
    total = int(ooff[-1])
    out = []
    for p0 in range(0, total, T):
        p1 = min(p0 + T, total)
        single = int(ooff[segment_of(ooff, p0) + 1]) >= p1
        paths = []
        for q in range(p0, p0 + T, KPT):
            if q >= p1:
                paths.append(None)
            else:
                paths.append("serial" if segment_of(ooff, q) == segment_of(ooff, min(q + KPT, p1) - 1) else "runs")
        out.append((single, paths))
    return out


# -- the layouts of tests/test_gpu_merge.py -----------------------------------------------------------------------------------------------

A_LENGTHS = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 9000, 0, 3, 20011]
B_LENGTHS = A_LENGTHS[5:] + A_LENGTHS[:5]           # rotated by 5: every edge length meets an empty, a tiny and a long partner
A_FIRST, B_FIRST, SPARE = 3, 7, 37


def ragged_layout():
    """(na, aoff, nb, boff): aoff[0] = 3, boff[0] = 7, SPARE keys after the last segment on both sides"""
    aoff = A_FIRST + np.concatenate([[0], np.cumsum(A_LENGTHS)]).astype(np.int64)
    boff = B_FIRST + np.concatenate([[0], np.cumsum(B_LENGTHS)]).astype(np.int64)
    return int(aoff[-1]) + SPARE, aoff, int(boff[-1]) + SPARE, boff


def small_segments_layout(rng, S=5000, hi=8):
    """S segments of (0 .. hi - 1) + (0 .. hi - 1) keys: a tile spans hundreds of segments"""
    la, lb = rng.integers(0, hi, S), rng.integers(0, hi, S)
    aoff = np.concatenate([[0], np.cumsum(la)]).astype(np.int64)
    boff = np.concatenate([[0], np.cumsum(lb)]).astype(np.int64)
    return int(aoff[-1]), aoff, int(boff[-1]), boff


def medium_segments_layout(rng, S=300, mean=100):
    la, lb = rng.integers(mean - 30, mean + 30, S), rng.integers(mean - 30, mean + 30, S)
    aoff = np.concatenate([[0], np.cumsum(la)]).astype(np.int64)
    boff = np.concatenate([[0], np.cumsum(lb)]).astype(np.int64)
    return int(aoff[-1]), aoff, int(boff[-1]), boff


def sorted_segments(x, off, descending=False):
    """x with every segment [off[s], off[s+1]) sorted in the engine's order (stable); the keys outside the segments stay"""
    x = np.ascontiguousarray(x).copy()
    off = np.asarray(off).astype(np.int64)
    for s in range(off.size - 1):
        seg = x[off[s]:off[s + 1]]
        x[off[s]:off[s + 1]] = seg[np.argsort(order_map(seg, descending), kind="stable")]
    return x
