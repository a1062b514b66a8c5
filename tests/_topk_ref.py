"""Helpers of the top-k tests at production shapes: a linear-time exact host reference, the inverse of the engine's key encoding,
a mirror of the select chain's launch geometry, and the layouts the GPU tests run (shared with the CPU test that checks each layout
still reaches the path it is there for).

The reference gives what topk_oracle of tests/test_gpu_topk.py gives (the first min(k, L) entries of every valid segment's stable
sort of enc(x), ~enc(x) when descending) without sorting all n keys: per segment, a partition to the k best, then a sort of those
k.  It is computed once at the largest k; the answer at any smaller k is its prefix (the stable top-k is a prefix of the stable sort).
"""
import numpy as np

from test_gpu_float_keys import UINT, enc

TILE = 4096          # rsx::kSegTileKeys: tiles of the large-segment chain, on the global 4096-key grid
CUS = 256            # MI355X compute units: the engine's cus when it asks the device


def dec(e: np.ndarray, dtype) -> np.ndarray:
    """Inverse of enc: the keys of `dtype` whose encodings are the unsigned words e."""
    dtype = np.dtype(dtype)
    u = UINT[dtype]
    e = np.asarray(e, dtype=u)
    sign = u(1) << u(np.dtype(u).itemsize * 8 - 1)
    if dtype.kind == "f":
        v = np.where(e & sign, e ^ sign, ~e).astype(u)
    elif dtype.kind == "i":
        v = e ^ sign
    else:
        v = e.copy()
    return v.view(dtype)


class TopkRef:
    """keys [S, kmax] unsigned words, pos [S, kmax] uint32, written [S, kmax] bool at the largest k; at(k) is the answer for k <= kmax."""

    def __init__(self, keys, pos, written):
        self.keys, self.pos, self.written = keys, pos, written

    def at(self, k: int):
        assert k <= self.keys.shape[1]
        return self.keys[:, :k], self.pos[:, :k], self.written[:, :k]


def fast_topk(x: np.ndarray, off, kmax: int, descending: bool = False) -> TopkRef:
    n = x.size
    off = np.asarray(off, dtype=np.int64)
    nseg = len(off) - 1
    u = UINT[x.dtype]
    xu = x.view(u)
    e = enc(x)
    if descending:
        e = ~e
    wide = np.dtype(u).itemsize == 8
    keys = np.zeros((nseg, kmax), dtype=u)
    pos = np.zeros((nseg, kmax), dtype=np.uint32)
    written = np.zeros((nseg, kmax), dtype=bool)
    for s in range(nseg):
        a, b = int(off[s]), int(off[s + 1])
        if not (a <= b <= n) or a == b:
            continue
        L = b - a
        m = min(kmax, L)
        es = e[a:b]
        if not wide:
            # (key << 32) | position is unique: the m smallest composites are the stable top m, ties by index
            comp = (es.astype(np.uint64) << np.uint64(32)) | np.arange(L, dtype=np.uint64)
            if m < L:
                comp = np.partition(comp, m - 1)[:m]
            p = (np.sort(comp) & np.uint64(0xFFFFFFFF)).astype(np.int64)
        else:
            if m < L:
                kth = np.partition(es, m - 1)[m - 1]
                better = np.flatnonzero(es < kth)
                ties = np.flatnonzero(es == kth)[:m - better.size]
                sel = np.concatenate([better, ties])
            else:
                sel = np.arange(L)
            p = sel[np.lexsort((sel, es[sel]))]
        keys[s, :m] = xu[a + p]
        pos[s, :m] = p.astype(np.uint32)
        written[s, :m] = True
    return TopkRef(keys, pos, written)


# -- launch geometry of the select chain (mirrors seg_shape in capi_segmented.inc and topk_group_tiles in capi_topk.inc) -------------

def seg_shape(n: int, nseg: int):
    """(max_large, max_tiles) of seg_shape: bounds the host sizes the chain's grids and scratch by."""
    max_large = min(nseg, n // (TILE + 1))
    max_tiles = (n + TILE - 1) // TILE + max_large if max_large else 0
    return max_large, max_tiles


def topk_group_tiles(n: int, nseg: int, cus: int = CUS) -> int:
    """Tiles per workgroup of topk_hist_kernel: enough groups for about 8 workgroups per CU, at most 64 tiles per group."""
    _, max_tiles = seg_shape(n, nseg)
    want = cus * 8
    return min(max((max_tiles + want - 1) // want, 1), 64)


def select_geometry(off, n: int, cus: int = CUS) -> dict:
    """What one rsx_segmented_topk call over these offsets runs: the large segments (> 4096 keys), their tiles on the global grid
    (seg_tiles), the group width, how many large segments begin inside a group rather than at its first tile (each such start makes
    topk_hist_kernel flush the previous segment's counts mid-group), and the grids the pick kernel and the final sort stride over."""
    off = np.asarray(off, dtype=np.int64)
    a, b = off[:-1], off[1:]
    large = (b - a) > TILE
    la, lb = a[large], b[large]
    tiles = (lb + TILE - 1) // TILE - la // TILE
    tstart = np.concatenate([[0], np.cumsum(tiles)])
    nseg = len(off) - 1
    gtiles = topk_group_tiles(n, nseg, cus)
    max_large, _ = seg_shape(n, nseg)
    return {
        "nlarge": int(large.sum()),
        "tiles": int(tstart[-1]),
        "gtiles": gtiles,
        "switches": int(np.count_nonzero(tstart[1:-1] % gtiles)),
        "pick_grid": min(max_large, cus * 2),
        "sort_grid_k_gt_1024": min(max_large, cus * 4),
    }


# -- layouts of the GPU tests ------------------------------------------------------------------------------------------------------

def rows(count: int, length: int, start: int = 0) -> np.ndarray:
    return (start + np.arange(count + 1, dtype=np.int64) * length).astype(np.uint64)


def ragged_offsets() -> np.ndarray:
    """Row lengths drawn from 4097..40000 with small rows (0..4096 keys, every LDS class) between them, from an odd start."""
    rng = np.random.default_rng(2024)
    lens = []
    for _ in range(420):
        lens.append(int(rng.integers(4097, 40001)))
        if rng.random() < 0.5:
            lens.append(int(rng.choice([0, 1, 2, 255, 256, 257, 1024, 1025, 4095, 4096])))
    return (3 + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)


# name -> (key dtype, offsets); n = offsets[-1] (+ a few keys no segment covers for the ragged layout)
SHAPES = {
    "1024x50257_f32": (np.float32, lambda: rows(1024, 50257)),
    "2048x5000_u64": (np.uint64, lambda: rows(2048, 5000)),
    "64x151936_i64": (np.int64, lambda: rows(64, 151936)),
    "ragged_i32": (np.int32, ragged_offsets),
}
SHAPE_KS = (1, 50, 1000, 4096)


def shape_n(off) -> int:
    return int(off[-1]) + 5


# -- keys built in select order ----------------------------------------------------------------------------------------------------
# o is the key's rank word in the call's order: the smallest o is the best key.  enc(x) = o ascending, ~o descending; x = dec(...).

def from_order(o: np.ndarray, dtype, descending: bool) -> np.ndarray:
    u = UINT[np.dtype(dtype)]
    o = o.astype(u)
    return dec(~o if descending else o, dtype)


def _words(u, size, rng):
    return rng.integers(0, np.iinfo(u).max, size=size, dtype=u, endpoint=True)


def digit_local(dtype, off, n: int, rng, variant: str, descending: bool, k: int = 1000) -> np.ndarray:
    """Keys that differ only where one select round decides.  Segment s gets a round r (the large segments cycle through every round)
    and one random base word:
      window:   only the 8-bit digit of round r varies (all other bits equal the base);
      low:      only the lowest r + 1 bytes vary (rounds r' >= rounds - r - 1 all decide between distinct keys);
      straddle: as window, with min(k // 2, L // 4) better digits and a run of up to k ties of the next digit spread over the segment,
                so the run starts before the k-th slot and ends after it."""
    u = UINT[np.dtype(dtype)]
    bits = np.dtype(u).itemsize * 8
    rounds = bits // 8
    o = _words(u, n, rng)
    off = np.asarray(off, dtype=np.int64)
    nlarge = 0
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        L = b - a
        if L <= 0:
            continue
        if L > TILE:
            r = nlarge % rounds
            nlarge += 1
        else:
            r = s % rounds
        base = _words(u, 1, rng)[0]
        if variant == "low":
            width = 8 * (r + 1)
            mask = u(~u(0)) if width == bits else u((1 << width) - 1)
            o[a:b] = (base & ~mask) | (_words(u, L, rng) & mask)
            continue
        shift = u(bits - 8 * (r + 1))
        window = u(0xFF) << shift
        if variant == "window":
            digit = rng.integers(0, 256, L).astype(u)
        else:
            digit = rng.integers(101, 256, L).astype(u)
            nb = min(k // 2, L // 4)
            nt = min(k, L - nb)
            where = rng.permutation(L)
            digit[where[:nb]] = rng.integers(0, 100, nb).astype(u)
            digit[where[nb:nb + nt]] = u(100)
        o[a:b] = (base & ~window) | (digit << shift)
    return from_order(o, dtype, descending)


def pad_heavy(dtype, off, n: int, rng, descending: bool) -> np.ndarray:
    """Segments filled with the key whose select-order word is all ones (the LDS sorts' pad: UINT_MAX / INT_MAX / +NaN with every
    payload bit ascending, 0 / INT_MIN / the all-ones -NaN descending), a few better keys among them (some one below the pad)."""
    u = UINT[np.dtype(dtype)]
    ones = u(~u(0))
    o = np.full(n, ones, dtype=u)
    off = np.asarray(off, dtype=np.int64)
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        L = b - a
        if L <= 0:
            continue
        few = min(L, 1 + L // 97)
        at = a + rng.choice(L, few, replace=False)
        o[at] = _words(u, few, rng)
        o[at[::3]] = ones - u(1)
    return from_order(o, dtype, descending)
