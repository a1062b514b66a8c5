"""Host referee of rsx_segmented_search (no GPU, no library): two independent forms of the same definition, and the grid the kernel
states at the top of radix-sort_amd/csrc/rsx_search.hpp.

For query position j of segment s the result is #{ i in haystack segment s : key_i strictly before q_j } (left) or
#{ i : key_i not after q_j } (right), relative to off[s], in the engine's order: unsigned order of order_map(key).

  search_oracle   np.searchsorted over the order-mapped unsigned keys, segment by segment (needs a sorted haystack)
  search_count    the brute-force counts of the definition (any haystack)

The three forms of offsets: off None = one haystack segment [0, n) with the queries [0, Q) (qoff must be None); off given and qoff None =
the even form, Q / S queries per segment; both given = ragged queries.  Positions outside [qoff[0], qoff[S]) are -1 in the result.

The grid: tiles of TILE_Q = 1024 consecutive query positions, 256 threads; above 16 x CUs tiles a workgroup walks
ceil(tiles / (16 x CUs)) of them.  A tile whose live queries lie in one segment of L keys is RESIDENT when L <= 4096 and 16 Qt >= L,
SAMPLED when L > 4096 and Qt >= 256 (Qt = live queries of the tile), DIRECT otherwise and whenever it spans several segments.  The sampled
path stages the SAMPLES = 1024 keys at sample_positions(L) = floor(i L / 1024), i = 0 .. 1023.  tile_walk gives the (path, staged segment)
of every tile of every workgroup; the layouts at the end are those of tests/test_gpu_search_paths.py.
"""
import numpy as np

TILE_Q = 1024
THREADS = 256
RESIDENT_MAX = 4096
RESIDENT_PAY = 16          # resident when RESIDENT_PAY * Qt >= L
SAMPLED_PAY = 256          # sampled when Qt >= SAMPLED_PAY
SAMPLES = 1024
UINT = {4: np.uint32, 8: np.uint64}


def order_map(x: np.ndarray, descending: bool = False) -> np.ndarray:
    """Unsigned keys whose order is the engine's order of x.  Floats: IEEE 754 totalOrder (negative numbers: all bits flipped; others:
    sign bit set), so -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN.  Signed integers: the sign bit flipped.  Descending: the
    complement of the ascending key."""
    x = np.ascontiguousarray(x)
    u = UINT[x.dtype.itemsize]
    v = x.view(u)
    sign = u(1 << (8 * x.dtype.itemsize - 1))
    if x.dtype.kind == "f":
        y = np.where((v & sign) != 0, ~v, v | sign).astype(u)
    elif x.dtype.kind == "i":
        y = v ^ sign
    else:
        y = v.copy()
    return ~y if descending else y


def sample_positions(L: int) -> np.ndarray:
    """the positions, relative to the segment's start, of the 1024 keys the sampled path stages"""
    return (np.arange(SAMPLES, dtype=np.uint64) * np.uint64(L)) >> np.uint64(10)


def segments(n, off, nq, qoff):
    """[(haystack start, haystack end, query start, query end)] of the three forms of offsets"""
    if off is None:
        assert qoff is None, "query offsets need haystack offsets"
        return [(0, n, 0, nq)]
    off = np.asarray(off).astype(np.int64)
    S = off.size - 1
    if qoff is None:
        assert S > 0 and nq % S == 0, "the even form needs a multiple of the segment count"
        Q = nq // S
        return [(int(off[s]), int(off[s + 1]), s * Q, (s + 1) * Q) for s in range(S)]
    qoff = np.asarray(qoff).astype(np.int64)
    assert qoff.size == off.size
    return [(int(off[s]), int(off[s + 1]), int(qoff[s]), int(qoff[s + 1])) for s in range(S)]


def search_oracle(keys, off, queries, qoff, right=False, descending=False) -> np.ndarray:
    k, q = order_map(keys, descending), order_map(queries, descending)
    out = np.full(q.size, -1, dtype=np.int64)
    for a, b, c, d in segments(k.size, off, q.size, qoff):
        out[c:d] = np.searchsorted(k[a:b], q[c:d], side="right" if right else "left")
    return out


def search_count(keys, off, queries, qoff, right=False, descending=False) -> np.ndarray:
    k, q = order_map(keys, descending), order_map(queries, descending)
    out = np.full(q.size, -1, dtype=np.int64)
    for a, b, c, d in segments(k.size, off, q.size, qoff):
        seg = k[a:b]
        for j0 in range(c, d, 256):                   # blocks of queries: a (256 x L) comparison at a time
            qq = q[j0:min(j0 + 256, d), None]
            out[j0:j0 + qq.shape[0]] = ((seg[None, :] <= qq) if right else (seg[None, :] < qq)).sum(axis=1)
    return out


def tile_paths(n, off, nq, qoff, sampled=True):
    """the path of every tile of the query grid: 'resident', 'sampled', 'direct', or None for a tile without a live query"""
    segs = segments(n, off, nq, qoff)
    qlo, qhi = segs[0][2], segs[-1][3]
    owner = np.full(nq, -1, dtype=np.int64)
    for s, (_, _, c, d) in enumerate(segs):
        owner[c:d] = s
    paths = []
    for t in range((nq + TILE_Q - 1) // TILE_Q):
        a, e = max(t * TILE_Q, qlo), min((t + 1) * TILE_Q, qhi)
        if a >= e:
            paths.append(None)
            continue
        if owner[a] != owner[e - 1]:
            paths.append("direct")
            continue
        L = segs[owner[a]][1] - segs[owner[a]][0]
        qt = e - a
        if L <= RESIDENT_MAX:
            paths.append("resident" if RESIDENT_PAY * qt >= L else "direct")
        else:
            paths.append("sampled" if sampled and qt >= SAMPLED_PAY else "direct")
    return paths


def tile_walk(n, off, nq, qoff, cus, sampled=True):
    """Per workgroup of search_kernel, the (path, segment) of each of its tiles in the order it walks them: ('resident' | 'sampled', the
    segment it stages), ('direct', None), or (None, None) for a tile without a live query.  A workgroup keeps what it staged while path
    and segment stay the same and restages when either changes, so the ordered pairs inside a workgroup say what it does."""
    segs = segments(n, off, nq, qoff)
    starts = np.array([c for _, _, c, _ in segs] + [segs[-1][3]], dtype=np.int64)
    paths = tile_paths(n, off, nq, qoff, sampled)
    chunk = max(-(-len(paths) // (16 * cus)), 1)
    walk = []
    for t, p in enumerate(paths):
        a = max(t * TILE_Q, int(starts[0]))
        # the segment of the tile's first live query: the last one that starts at or before it (empty segments skipped)
        seg = int(np.searchsorted(starts[:-1], a, side="right")) - 1 if p in ("resident", "sampled") else None
        if t % chunk == 0:
            walk.append([])
        walk[-1].append((p, seg))
    return walk


def pairs_of(walk):
    """the ordered pairs (tile, next tile) that occur inside a workgroup"""
    return {(g[i], g[i + 1]) for g in walk for i in range(len(g) - 1)}


# -- layouts with a little more than 1024 x 16 x CUs queries: a workgroup walks two tiles (tests/test_gpu_search_paths.py) --------------------

CYCLE = [0, 7, 3000, 4097, 4096, 20000, 2000]       # haystack lengths of the even layouts: an odd count, so that it drifts against the tiles
RAGGED_CYCLE = [3001, 4095, 1021, 3, 2000, 4090, 1, 2, 6, 0, 4093, 5000, 777]


def even_layout(cus, Q):
    """(n, off, nq): the even form, Q queries a segment, ceil((1024 x 16 x CUs + 1) / Q) segments with the lengths of CYCLE.  Q = 1536:
    tiles are (inside segment 2k, across 2k and 2k + 1, inside 2k + 1) while workgroups pair them by two; Q = 2048: a workgroup's two tiles
    lie inside one segment"""
    S = -(-(TILE_Q * 16 * cus + 1) // Q)
    off = np.concatenate([[0], np.cumsum([CYCLE[s % len(CYCLE)] for s in range(S)])]).astype(np.uint64)
    return int(off[-1]), off, S * Q


def one_segment_layout(cus, L):
    """(n, None, nq): one segment of L keys, 1024 x 16 x CUs + 5 queries"""
    return L, None, TILE_Q * 16 * cus + 5


def ragged_dead_layout(cus):
    """(n, off, nq, qoff): ragged queries.  qoff[0] = 3 x 1024 + 100: workgroup 0 is dead, workgroup 1 = (dead, live).  Then one whole
    tile of queries per segment with the lengths of RAGGED_CYCLE, the haystack starting at 1: every workgroup restages in its second
    tile, at starts of every residue mod 4.  qoff[S] lies in the first tile of a workgroup: (live, dead); the last workgroup is dead"""
    tiles = 16 * cus + 2
    whole = tiles - 4 - 4                                        # tiles 4 .. tiles - 5, one segment each
    lengths = [3001] + [RAGGED_CYCLE[(s + 1) % len(RAGGED_CYCLE)] for s in range(whole)] + [1000]
    off = np.concatenate([[1], 1 + np.cumsum(lengths)]).astype(np.uint64)
    qcounts = [TILE_Q - 100] + [TILE_Q] * whole + [500]
    qoff = np.concatenate([[3 * TILE_Q + 100], 3 * TILE_Q + 100 + np.cumsum(qcounts)]).astype(np.uint64)
    return int(off[-1]) + 3, off, (tiles - 1) * TILE_Q + 5, qoff


def sort_engine_order(x: np.ndarray, descending: bool = False) -> np.ndarray:
    """x sorted in the engine's order (stable)"""
    return x[np.argsort(order_map(x, descending), kind="stable")]


def extremes(dt) -> np.ndarray:
    """the type's extreme keys: integer limits; for floats ±NaN (quiet, and with every payload bit set), ±inf, ±0, ±max, ±smallest subnormal"""
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        return np.array([info.min, info.min + 1, -1 if dt.kind == "i" else 1, 0, 1, info.max - 1, info.max], dtype=dt)
    u = UINT[dt.itemsize]
    bits = 8 * dt.itemsize
    sign = 1 << (bits - 1)
    one = np.array([1.0], dtype=dt).view(u)[0]
    inf = int(np.array([np.inf], dtype=dt).view(u)[0])
    qnan = int(np.array([np.nan], dtype=dt).view(u)[0]) & ~sign
    pats = [0, 1, int(one), inf - 1, inf, qnan, sign - 1]
    return np.array(pats + [p | sign for p in pats], dtype=u).view(dt)


def neighbours(x: np.ndarray) -> np.ndarray:
    """every key, the key before and the key after it in the order (integers: -1 / +1 wrapping; floats: one step in totalOrder)"""
    x = np.ascontiguousarray(x)
    y = order_map(x)
    u = y.dtype.type
    return np.concatenate([x, order_unmap(y - u(1), x.dtype), order_unmap(y + u(1), x.dtype)])


def order_unmap(y: np.ndarray, dt) -> np.ndarray:
    dt = np.dtype(dt)
    u = UINT[dt.itemsize]
    sign = u(1 << (8 * dt.itemsize - 1))
    if dt.kind == "f":
        v = np.where((y & sign) != 0, y ^ sign, ~y).astype(u)
    elif dt.kind == "i":
        v = y ^ sign
    else:
        v = y
    return np.ascontiguousarray(v).view(dt)
