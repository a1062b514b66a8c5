"""The referee of rsx_segmented_rank (tests/test_rank.py, tests/test_gpu_rank.py): a stable argsort of the encoded keys of every segment,
then the five tie rules from the boundaries of the runs of equal keys.  numpy only; written from the contract in include/radixsort_hip.h
and independent of csrc/rsx_rank_math.hpp (no tiles, no carries).  rank_oracle_many is the same referee in one lexsort, for calls with
very many segments.  Below the referee: rank_geometry and join_facts, mirrors of what capi_rank.inc launches and of what the join of
rsx_rank.hpp folds, and the layouts of tests/test_gpu_rank_paths.py with fixed seeds, so that tests/test_rank.py can check on the CPU
that each one reaches the path it is named for.

Order: the unsigned order of encode(x) is the engine's ascending order: unsigned keys as they are, signed keys with the sign bit flipped,
floats in IEEE 754 totalOrder (negative: all bits flipped, else the sign bit flipped); descending is the complement.  Keys tie iff their
bits are equal, which is equality of the encoded keys."""
import numpy as np

import _segmented_ref as S          # seg_geometry: the classify and the chain, which the rank shares with the segmented sort

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


# -- the whole call without a loop over the segments ---------------------------------------------------------------------------------------------

def rank_oracle_many(x, off, descending=False, fill=0):
    """rank_oracle for calls with hundreds of thousands of segments (valid offsets only): ONE stable lexsort over (segment, encoded key),
    runs cut where the key or the segment changes, the five rules and the tie counts scattered back through the order."""
    n = len(x)
    o = np.asarray(off).astype(np.int64)
    lens = np.diff(o)
    assert o[0] >= 0 and o[-1] <= n and (lens >= 0).all(), "valid offsets only"
    lo, hi = int(o[0]), int(o[-1])
    m = hi - lo
    ranks = np.full((5, n), fill, dtype=np.uint32)
    ties = np.full(n, fill, dtype=np.uint32)
    written = np.zeros(n, dtype=bool)
    if m == 0:
        return ranks, ties, written
    seg = np.repeat(np.arange(lens.size, dtype=np.int64), lens)             # the segment of lo + i: non-decreasing
    e = encode(x[lo:hi], descending)
    order = np.lexsort((e, seg))                                            # by segment, then by key, stable: segment s stays in [o[s], o[s+1])
    s = e[order]
    head = np.ones(m, dtype=bool)
    head[1:] = (s[1:] != s[:-1]) | (seg[1:] != seg[:-1])
    run = np.cumsum(head) - 1
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], m)
    first = (o[:-1] - lo)[seg]                                              # where the segment of every sorted position begins
    r_lo, r_hi = starts[run] - first, ends[run] - first
    by_sorted = np.stack([np.arange(m) - first, r_lo, r_hi - 1, run - run[first], r_lo + r_hi - 1]).astype(np.uint32)
    ranks[:, lo + order] = by_sorted
    ties[lo + order] = (r_hi - r_lo).astype(np.uint32)
    written[lo:hi] = True
    return ranks, ties, written


# -- what one call launches (tests/test_gpu_rank_paths.py; tests/test_rank.py pins every layout to its path) -------------------------------------

JOIN_THREADS = 256          # rsx::kRankThreads: threads of rank_join_kernel, each folding `per` consecutive tile records
WAVE = 64                   # rsx::kWave
ONES_THREADS = 256          # rsx::kRankSmallThreads (= kUniqSmallThreads): threads of rank_ones_kernel
OFFSETS_PER_CU = 4          # offsets_grid of capi_family.inc: min(ceil((nseg + 1) / 256), cus * 4)
CLASS_TILE = (256, 1024, 4096)


def _ceil(a, b):
    return (a + b - 1) // b


def rank_geometry(off, n, cus=S.CUS):
    """seg_geometry's figures and what rank_enqueue of capi_rank.inc launches on top of them.  off None: the flat form, whose one segment
    [0, n) is the chain's only large one whatever its length (rank_flat_kernel), with no classify, no one-key and no small kernel.
      ones_grid, ones_trips          rank_ones_kernel's workgroups and the trips of its stride loop
      small_trips[3]                 items the busiest workgroup of rank_small_kernel walks, by class
      tile_grid, tile_trips          rank_edge_kernel / rank_write_kernel: min(max_tiles, cus * 8) workgroups over `tiles` tiles
      join_grid, join_trips          rank_join_kernel: min(max_large, cus * 8) workgroups over `nlarge` segments
      T[], join_per[], join_used[]   per large segment: its tiles, tiles per join thread, join threads with a non-empty piece"""
    if off is None:
        tiles = _ceil(n, TILE)
        g = {"count": [0, 0, 0], "grid": [0, 0, 0], "trips": [0, 0, 0], "nblocks": 0, "per": 0, "large_blocks": 0, "last_large_block": None,
             "nlarge": 1, "max_large": 1, "tiles": tiles, "max_tiles": tiles, "chain_ok": 1, "chain_grid": 0, "bad": np.zeros(0, dtype=np.int64),
             "first_bad": None, "ones": 0, "large": np.zeros(1, dtype=np.int64)}
        T = np.array([tiles], dtype=np.int64)
        nseg = 0
    else:
        g = S.seg_geometry(off, n, cus)
        o = np.asarray(off).astype(np.int64)
        nseg = len(o) - 1
        la, lb = o[:-1][g["large"]], o[1:][g["large"]]
        T = (lb + TILE - 1) // TILE - la // TILE
    g["ones_grid"] = min(_ceil(nseg + 1, ONES_THREADS), cus * OFFSETS_PER_CU) if nseg else 0
    g["ones_trips"] = _ceil(nseg, g["ones_grid"] * ONES_THREADS) if nseg else 0
    g["small_trips"] = list(g["trips"])
    g["tile_grid"] = min(g["max_tiles"], cus * S.CHAIN_PER_CU)
    g["join_grid"] = min(g["max_large"], cus * S.CHAIN_PER_CU)
    g["tile_trips"] = _ceil(g["tiles"], g["tile_grid"]) if g["tile_grid"] else 0
    g["join_trips"] = _ceil(g["nlarge"], g["join_grid"]) if g["join_grid"] else 0
    per = np.maximum(_ceil(T, JOIN_THREADS), 1)
    g["T"], g["join_per"], g["join_used"] = T.tolist(), per.tolist(), _ceil(T, per).tolist()
    return g


def rank_summary(g):
    """the figures of rank_geometry on one line (what the GPU tests print before they assert their path)"""
    shown = slice(0, 6)
    return (S.summary(g) + f" | ones grid={g['ones_grid']} trips={g['ones_trips']} small_trips={g['small_trips']} tile grid={g['tile_grid']} "
            f"trips={g['tile_trips']} join grid={g['join_grid']} trips={g['join_trips']} T={g['T'][shown]} per={g['join_per'][shown]} "
            f"used={g['join_used'][shown]}")


def join_facts(a, s):
    """One sorted large segment (encoded keys s, from global index a) as rank_edge_kernel and rank_join_kernel see it:
      edges                (heads, first, last) per tile of the global grid clipped at the segment's ends; None: the tile holds no head
      T, per               tiles; tiles per join thread
      thread_headless[]    per join thread with a non-empty piece: none of its tiles holds a head (kNone passes through the thread)
      used, idle           join threads with and without tiles
      last_thread_tiles    tiles of the last thread that has any
      wave_headless        some aligned group of 64 join threads, each with tiles, is headless throughout (kNone passes through a lane scan
                           and a wave total)
      first_key_head       some tile but the first begins with a head (a run ends on a tile's last key)
      last_key_head        some tile but the last ends with a head (a run begins on a tile's last key)
      all_heads_tiles      the longest stretch of consecutive tiles in which every key is a head"""
    L = len(s)
    head = np.ones(L, dtype=bool)
    head[1:] = s[1:] != s[:-1]
    inner = np.arange((a // TILE + 1) * TILE, a + L, TILE) - a
    bounds = np.concatenate([[0], inner, [L]]).astype(np.int64)
    edges, full = [], []
    for p, q in zip(bounds[:-1], bounds[1:]):
        h = np.flatnonzero(head[p:q])
        edges.append((int(h.size), int(p + h[0]) if h.size else None, int(p + h[-1]) if h.size else None))
        full.append(h.size == q - p)
    T = len(edges)
    per = max(_ceil(T, JOIN_THREADS), 1)
    used = _ceil(T, per)
    thread_headless = [all(edges[t][0] == 0 for t in range(x * per, min((x + 1) * per, T))) for x in range(used)]
    wave_headless = any(all(thread_headless[w:w + WAVE]) for w in range(0, used - WAVE + 1, WAVE))
    best = run = 0
    for f in full:
        run = run + 1 if f else 0
        best = max(best, run)
    return {"edges": edges, "T": T, "per": per, "used": used, "idle": JOIN_THREADS - used, "last_thread_tiles": T - (used - 1) * per,
            "thread_headless": thread_headless, "wave_headless": wave_headless,
            "first_key_head": any(e[1] == int(p) for e, p in zip(edges[1:], bounds[1:-1])),
            "last_key_head": any(e[2] == int(q) - 1 for e, q in zip(edges[:-1], bounds[1:-1])),
            "all_heads_tiles": best}


# -- the layouts of tests/test_gpu_rank_paths.py ------------------------------------------------------------------------------------------------------

def from_sorted_rank(r, dtype, descending=False):
    """keys of `dtype` whose place in the call's order grows with the small non-negative integers r (exact in every key type)"""
    r = np.asarray(r, dtype=np.int64)
    return (int(r.max()) - r if descending else r).astype(dtype)


# B. real keys equal to the pad key
PAD_PAIRS = [("uint32", False), ("uint32", True), ("float32", False), ("float32", True)]


def pad_value(dtype, descending):
    """the key whose encoded form is all ones, the pad of rank_small_kernel: the unsigned maximum ascending and 0 descending; +NaN with
    every mantissa bit set (0x7FFFFFFF) ascending and -NaN 0xFFFFFFFF descending"""
    dt = np.dtype(dtype)
    u = _UINT[dt.itemsize]
    bits = {("u", False): ~u(0), ("u", True): u(0), ("f", False): ~u(0) >> u(1), ("f", True): ~u(0)}[(dt.kind, descending)]
    v = np.array([bits], dtype=u).view(dt)
    assert encode(v, descending)[0] == ~u(0)
    return v[0]


def pad_equal_layout():
    """(n, off, planted): in every small class segments of TILE_c - 1, TILE_c - 17 and 2 TILE_c / 3 keys (shorter than the class's tile:
    pads follow the real keys), a one-key and an empty segment between the classes, one large segment of 4097 + 300 keys; off[0] = 3.
    planted: the indices of the segments that get the pad-equal tail."""
    lengths = []
    for tile in CLASS_TILE:
        lengths += [tile - 1, tile - 17, 2 * tile // 3, 1, 0]
    lengths.append(TILE + 1 + 300)
    off = S.offsets_from(lengths, start=3)
    return int(off[-1]) + 6, off, [i for i, L in enumerate(lengths) if L >= 2]


def pad_equal_keys(dtype, descending, n, off, planted, rng):
    """(x, count per planted segment): a small alphabet without the pad-equal value everywhere; in each planted segment the last third
    of the positions and a few scattered ones hold the pad-equal value.  The one-key segments hold it too."""
    dt = np.dtype(dtype)
    pad = pad_value(dt, descending)
    if dt.kind == "f":
        alphabet = np.array([-3.5, -0.0, 0.0, 1.25, np.inf, -np.inf, 7.0], dtype=dt)
    else:
        alphabet = np.array([1, 2, 5, 1 << 20, (1 << 32) - 2, 77, 4096], dtype=dt)
    x = alphabet[rng.integers(0, len(alphabet), n)]
    o = np.asarray(off).astype(np.int64)
    counts = {}
    for s in range(len(o) - 1):
        a, b = int(o[s]), int(o[s + 1])
        if b - a == 1:
            x[a] = pad
        if s in planted:
            x[b - (b - a) // 3:b] = pad
            x[a + rng.choice(b - a - (b - a) // 3, 5, replace=False)] = pad
            counts[s] = (b - a) // 3 + 5
    return x, counts


# D. the join beyond one wave and beyond 256 tiles
JOIN_TILES = (65, 256, 385)
# 385, not 257, tiles in the third segment: a run of 2 * 128 tiles' worth does not fit into 257 tiles beside the 6-tile run and the
# increasing stretch; 385 is odd, so that with per == 2 the last join thread still holds ONE tile (193 threads with tiles, 63 idle).


def _runs_to_lengths(L, spans, rng, filler=(1, 3000)):
    """run lengths that sum to L: `spans` is a sorted list of (start, end) runs that must exist exactly; the gaps between them are
    filled with runs of random lengths"""
    out, at = [], 0
    for p, q in list(spans) + [(L, L)]:
        while at < p:
            step = min(int(rng.integers(filler[0], filler[1] + 1)), p - at)
            out.append(step)
            at += step
        if q > p:
            out.append(q - p)
            at = q
    return out


def join_layout(seed=0):
    """(n, off, names, runs): three large segments of 65, 256 and 385 tiles, each starting off the 4096 grid, small, one-key and empty
    segments between them; off[0] = 11.  names: their segment indices.  runs[name]: the run lengths of that segment in sorted order.
      t65    random runs, one of them over the tiles 31 and 32: the second wave of join threads holds one record, tile 64's, with a head
      t256   per == 1, every thread one tile; one run from the middle of tile 60 to the middle of tile 195: join threads 61 .. 194, waves
             1 and 2 whole, hold no head
      t385   per == 2, thread 192 holds the one tile 384, 63 threads idle.  Tiles 0 .. 9 strictly increasing (every key a head); a one-key
             run on the last key of tile 11; a run over the whole tiles 12 .. 17 (it begins on a tile's first key and ends on a tile's
             last key: threads 7 and 8 hold no head); a run from the last key of tile 19 into tile 21; one run from the middle of tile 100
             into the last tile, 283 tiles' worth: the threads 51 .. 191, waves 1 and 2 whole, hold no head, and thread 192 in wave 3 takes
             its start through both"""
    rng = np.random.default_rng(7000 + seed)
    start = 11
    between = [300, 1, 0, 2000]
    lengths, names, runs = [], {}, {}
    at = start
    for name, tiles in zip(("t65", "t256", "t385"), JOIN_TILES):
        a = at
        f = TILE - a % TILE                                     # keys of the first tile
        assert 0 < f < TILE
        tail = int(rng.integers(100, 3000))                     # keys of the last tile
        L = f + (tiles - 2) * TILE + tail
        edge = lambda t: f + (t - 1) * TILE                     # where tile t begins, relative to the segment (t >= 1)
        if name == "t65":
            spans = [(edge(30) + 100, edge(33) + 50), (edge(64) + 10, edge(64) + 11)]
        elif name == "t256":
            spans = [(edge(60) + 2000, edge(195) + 2000)]
        else:
            inc = edge(10)
            spans = [(i, i + 1) for i in range(inc)]
            spans += [(edge(12) - 1, edge(12)), (edge(12), edge(18)), (edge(20) - 1, edge(21) + 700), (edge(100) + 2048, edge(384) + 50)]
        runs[name] = _runs_to_lengths(L, spans, rng)
        names[name] = len(lengths)
        lengths.append(L)
        lengths += between
        at = a + L + sum(between)
    off = S.offsets_from(lengths, start=start)
    return int(off[-1]) + 9, off, names, runs


def join_keys(dtype, descending, n, off, names, runs, rng):
    """the keys of join_layout: every planted segment gets its runs (run i holds the i-th key of the call's order) shuffled inside the
    segment; everything else comes from a 6-value alphabet"""
    x = from_sorted_rank(rng.integers(0, 6, n), dtype, descending)
    o = np.asarray(off).astype(np.int64)
    for name, s in names.items():
        a, b = int(o[s]), int(o[s + 1])
        r = np.repeat(np.arange(len(runs[name])), runs[name])
        assert r.size == b - a
        x[a:b] = from_sorted_rank(r, dtype, descending)[rng.permutation(b - a)]
    return x


def join_paths(facts):
    """{path: reached} of join_layout from the join_facts of its three large segments in order"""
    t65, t256, t385 = facts
    return {
        "65 tiles: the second wave holds one record, with a head": (t65["T"], t65["used"], t65["idle"]) == (65, 65, 191) and not t65["thread_headless"][64],
        "256 tiles: per == 1, every thread one tile": (t256["T"], t256["per"], t256["used"], t256["idle"]) == (256, 1, 256, 0),
        "256 tiles: a whole wave of join threads without a head": t256["wave_headless"],
        "per == 2, the last thread with tiles holds one, idle threads": t385["per"] == 2 and t385["last_thread_tiles"] == 1 and 0 < t385["idle"] == 256 - (t385["T"] + 1) // 2,
        "per == 2: a thread's whole piece without a head": any(t385["thread_headless"]),
        "per == 2: a whole wave of join threads without a head": t385["wave_headless"],
        "a tile begins with a head": t385["first_key_head"],
        "a tile ends with a head": t385["last_key_head"],
        "eight tiles of heads only": t385["all_heads_tiles"] >= 8,
    }


# E. more tiles and more large segments than workgroups
def grid_stride_layout(cus=S.CUS, seed=0):
    """(n, off): cus * 8 + 40 large segments from off[0] = 5, a few empty and one-key segments between them, n = off[S].  All but sixteen
    have 4097 .. 4099 keys, those sixteen up to 4300: as many large segments as n keys can hold, or at most three fewer (max_large =
    n / 4097), on a join grid of cus * 8.  Path: join_trips >= 2, tile_trips >= 2, max_large - nlarge <= 3."""
    rng = np.random.default_rng(900 + seed)
    count = cus * 8 + 40
    lens = TILE + 1 + rng.integers(0, 3, count)
    lens[rng.choice(count, 16, replace=False)] = rng.integers(TILE + 101, TILE + 205, 16)
    out = []
    for i, L in enumerate(lens.tolist()):
        out.append(L)
        if i % 400 == 7:
            out += [0, 1, 0]
    off = S.offsets_from(out, start=5)
    return int(off[-1]), off


# F. the flat form: the regime sort_chain_passes of rsx_capi.hip picks by n, from the engine's defaults (tile_sort, self_scan and
# lookahead on, self_scan_max = 1024 tiles, small_tile_max_keys = 2^19; 8-bit digits above radix8_min_keys, which is at most 2^19)
FLAT_SIZES = [1 << 19, (1 << 19) + 1, 257 * TILE - 100, 1 << 22, (1 << 22) + TILE + 1]
FLAT_SIZES_8BIT = [(1 << 19) + 1, (1 << 20) + 5]
FLAT_CAPACITY = 1 << 23


def flat_regime(n, radix_bits=4):
    if radix_bits == 8 and n > 1 << 19:
        return "8-bit chain"
    if n <= TILE:
        return "one tile"
    if _ceil(n, TILE) <= 1024:
        return "small-tile self-scan" if n <= 1 << 19 else "self-scan"
    return "look-ahead chain"


# H. replays of one captured call over other offsets: the same n and segment count as the mixed layout of tests/test_gpu_rank.py
REPLAY_LENGTHS = {
    "another class mix": [100, 100, 100, 300, 600, 2000, 2500, 4096, 1, 1, 0, 20000, 4097, 9000],
    "no large segment": [4096] * 5 + [4000, 3000, 1024, 1000, 256, 255, 2, 1, 0],
    "large or empty": [0, 10000, 0, 5000, 4097, 0, 0, 12000, 0, 8193, 0, 0, 4100, 0],
}
REPLAY_STARTS = {"another class mix": 5, "no large segment": 37, "large or empty": 0}
