"""Host referee of the sample tests (rsx_segmented_sample): the masses of _wselect_ref.mass_np, the predicate of _compact_ref.keep_flags, the
target rule of _wselect_ref.target_of, an int64 cumsum of the masses in INDEX order and searchsorted(side="left").

masses         int64 masses of every element of [0, n), the elements the bound's predicate rejects weighing 0.
Referee        the running masses once per upload; Referee(...)(targets, fraction) gives (index [S, R] uint32, mass [S, R] uint64,
               written [S, R] bool, total [S] uint64): `written` marks the slots the call writes.
sample_oracle  Referee in one call.
sample_loop    the definition, element by element with Python integers, for the referee's own test.

For the path tests (tests/test_sample.py checks on the CPU that each layout reaches the path it is named for):
walk_facts     what sample_draw_kernel's walk meets on one segment: its tiles, the chunks of WALK_TILES, the prefix at every chunk's end.
tile_sums      which tiles sample_tile_kernel reads: 'both' (inside one long segment), 'lead', 'tail', 'lead+tail', or None (not read).
tile_grid      (chunk, grid) of sample_tile_kernel's launch; group_walk: the tile_sums kinds of every workgroup's tiles, 'outside' for a
               tile the workgroup skips because it lies outside [off[0], off[S]).
group_edges    the 256-element group boundaries of every piece of a segment with the running mass there; group_targets: those and + 1.

The layouts of tests/test_gpu_sample_paths.py (two_tile_layout, group_layout, second_trip_layout, huge_total_layout) take the CU count
where the path depends on it.
"""
import numpy as np

import _compact_ref as C
import _wselect_ref as W

TILE = 4096             # rsx_sample::kTileKeys
WALK_TILES = 256        # rsx_sample::kWalkTiles: tiles of one segment per step of the walk
WALK_LANE = 4           # rsx_sample::kWalkLane
GROUP = 256             # rsx::kSampleGroup: elements of a piece per step
WAVES = 4               # slots a workgroup of sample_draw_kernel takes at a time (kSampleThreads / 64)
DRAW_PER_CU = 32        # its grid: min(ceil(slots / 4), cus * 32)
FRACTION, INVERT, STRICT = 128, C.INVERT, C.STRICT


def masses(weights, keys=None, off=None, bounds=None, descending=False, strict=False, invert=False, weight_exp=0) -> np.ndarray:
    """int64 [n].  weights None: the float keys are their own weights."""
    w = keys if weights is None else weights
    m = W.mass_np(w, weight_exp).astype(np.int64)
    if bounds is not None:
        keep = C.keep_flags(keys, off, bounds=bounds, descending=descending, strict=strict, invert=invert)
        m = np.where(keep, m, 0)
    return m


class Referee:
    def __init__(self, weights, off, keys=None, bounds=None, descending=False, strict=False, invert=False, weight_exp=0):
        n = (keys if weights is None else weights).size
        self.off = C._offsets(n, off)
        self.m = masses(weights, keys, off, bounds, descending, strict, invert, weight_exp)
        self.run = np.concatenate([[0], np.cumsum(self.m, dtype=np.int64)])        # run[i] = the mass of [0, i): below 2^63
        a, b = self.off[:-1], self.off[1:]
        self.total = (self.run[b] - self.run[a]).astype(np.uint64)

    def __call__(self, targets, fraction=False):
        nseg = len(self.off) - 1
        tt = np.asarray(targets).reshape(nseg, -1)
        R = tt.shape[1]
        index = np.zeros((nseg, R), dtype=np.uint32)
        mass = np.zeros((nseg, R), dtype=np.uint64)
        written = np.zeros((nseg, R), dtype=bool)
        for s in np.flatnonzero(self.total > 0):
            a, b = int(self.off[s]), int(self.off[s + 1])
            tot, base = int(self.total[s]), int(self.run[a])
            T = np.array([W.target_of(tot, t, fraction) for t in tt[s]], dtype=np.int64)
            ok = T > 0
            i = np.searchsorted(self.run[a + 1:b + 1], base + T[ok], side="left")   # the smallest i with P_i >= T
            index[s, ok] = i
            mass[s, ok] = self.run[a + 1 + i] - base
            written[s] = ok
        return index, mass, written, self.total.copy()


def sample_oracle(weights, off, targets, fraction=False, **kw):
    return Referee(weights, off, **kw)(targets, fraction)


def sample_loop(weights, off, targets, fraction=False, keys=None, bounds=None, descending=False, strict=False, invert=False, weight_exp=0):
    """sample_oracle, element by element: [(index or None, mass or None)] per slot in row-major order, and the totals"""
    m = [int(v) for v in masses(weights, keys, off, bounds, descending, strict, invert, weight_exp)]
    o = [int(v) for v in C._offsets(len(m), off)]
    nseg = len(o) - 1
    tt = np.asarray(targets).reshape(nseg, -1)
    out, totals = [], []
    for s in range(nseg):
        total = sum(m[o[s]:o[s + 1]])
        totals.append(total)
        for t in tt[s]:
            T = W.target_of(total, t, fraction)
            ans = (None, None)
            run = 0
            if T:
                for i in range(o[s], o[s + 1]):
                    run += m[i]
                    if run >= T:
                        ans = (i - o[s], run)
                        break
            out.append(ans)
    return out, totals


# -- paths ------------------------------------------------------------------------------------------------------------------------------
def walk_facts(m, off, s):
    """segment s: {'tiles': (ta, tb) or None, 'one_tile', 'pieces': the piece masses per tile, 'chunks': number of walk steps,
    'chunk_prefix': the running mass at the end of every chunk but the last}"""
    o = np.asarray(off).astype(np.int64)
    a, b = int(o[s]), int(o[s + 1])
    if a == b:
        return {"tiles": None, "one_tile": True, "pieces": [], "chunks": 0, "chunk_prefix": []}
    ta, tb = a // TILE, (b - 1) // TILE
    run = np.concatenate([[0], np.cumsum(np.asarray(m, dtype=np.int64))])
    pieces = [int(run[min(b, (t + 1) * TILE)] - run[max(a, t * TILE)]) for t in range(ta, tb + 1)]
    chunks = (tb - ta) // WALK_TILES + 1
    prefix = [sum(pieces[:c * WALK_TILES]) for c in range(1, chunks)]
    return {"tiles": (ta, tb), "one_tile": ta == tb, "pieces": pieces, "chunks": chunks, "chunk_prefix": prefix}


def tile_sums(n, off):
    """per tile of the grid what sample_tile_kernel sums: None (the tile is not read), 'lead', 'tail', 'lead+tail' (two segments cross
    its edges), 'both' (the tile lies inside one segment that crosses both edges: read once)"""
    o = C._offsets(n, off)
    lo, hi = int(o[0]), int(o[-1])
    out = []
    for t in range((n + TILE - 1) // TILE):
        ts, te = t * TILE, (t + 1) * TILE
        kind = None
        if ts < hi and te > lo:
            lead = tail = False
            sl = st = -1
            if ts > lo:
                sl = C._seg_upper(o, 0, ts) - 1
                lead = int(o[sl]) < ts
            if te < hi:
                st = C._seg_upper(o, 0, te - 1) - 1
                tail = int(o[st + 1]) > te
            kind = "both" if lead and tail and sl == st else "lead+tail" if lead and tail else "lead" if lead else "tail" if tail else None
        out.append(kind)
    return out


def draw_grid(nseg, R, cus=256):
    """(workgroups of sample_draw_kernel, slots)"""
    slots = nseg * R
    return min((slots + WAVES - 1) // WAVES, cus * DRAW_PER_CU), slots


# -- layouts of the GPU path tests ------------------------------------------------------------------------------------------------------------
def one_tile_layout():
    """one segment inside tile 1"""
    off = C.offsets_from([3000], start=TILE + 100)
    return 2 * TILE + 9, off


def crossing_layout():
    """a segment over one tile boundary (1000 elements before it, 2000 behind), neighbours on both sides"""
    off = C.offsets_from([50, 3000, 70], start=TILE - 1050)
    return 2 * TILE, off


def hollow_layout():
    """a segment of five tiles and a bit whose middle tiles weigh nothing (the test zeroes them): LONG segment index 1"""
    off = C.offsets_from([10, 5 * TILE + 100, 20], start=TILE // 2)
    return int(off[-1]) + 7, off


LONG_LENGTHS = [5000, (WALK_TILES + 1) * TILE + 17, 300]
LONG_SEGMENT = 1


def long_layout():
    """segment 1 is longer than one chunk of the walk by one tile and 17 elements; off[0] = 3"""
    off = C.offsets_from(LONG_LENGTHS, start=3)
    return int(off[-1]) + 5, off


def long_targets(m, off):
    """1, total, and every chunk's prefix and prefix + 1 of the long segment"""
    f = walk_facts(m, off, LONG_SEGMENT)
    total = sum(f["pieces"])
    t = [1, total]
    for p in f["chunk_prefix"]:
        t += [p, p + 1]
    return t


MANY_SEGMENTS = 1 << 16


def many_layout(seed=5):
    """2^16 segments of 0 .. 7 elements: more segments than workgroups of the draw grid at R = 1"""
    rng = np.random.default_rng(seed)
    off = C.offsets_from(rng.integers(0, 8, MANY_SEGMENTS), start=0)
    return int(off[-1]), off


def inner_layout():
    """off[0] > 0 and off[S] < n, both in the middle of tiles, segments across tile edges in between"""
    off = C.offsets_from([5000, 0, 9000, 17], start=TILE + 33)
    return int(off[-1]) + 2 * TILE + 11, off


LAYOUTS = {
    "one_tile": one_tile_layout, "crossing": crossing_layout, "hollow": hollow_layout, "long": long_layout, "many": many_layout,
    "inner": inner_layout,
}


# -- the launch paths that need the CU count (tests/test_gpu_sample_paths.py) -------------------------------------------------------------------------

def tile_grid(n, cus=256):
    """(chunk, grid) of sample_tile_kernel: capi_family.inc's tile_chunks"""
    ntiles = (n + TILE - 1) // TILE
    chunk = (ntiles + cus * 16 - 1) // (cus * 16)
    return chunk, (ntiles + chunk - 1) // chunk


def group_walk(n, off, cus=256):
    """per workgroup of sample_tile_kernel the kinds of its tiles in the order it walks them: tile_sums' kinds, with 'outside' for a
    tile that ends at or before off[0] or begins at or behind off[S] (the `continue` of the tile loop)"""
    o = C._offsets(n, off)
    lo, hi = int(o[0]), int(o[-1])
    kinds = tile_sums(n, off)
    for t in range(len(kinds)):
        if t * TILE >= hi or (t + 1) * TILE <= lo:
            kinds[t] = "outside"
    chunk, grid = tile_grid(n, cus)
    return [tuple(kinds[g * chunk:(g + 1) * chunk]) for g in range(grid)]


SHORT_TILES = 4                                   # tiles 8 .. 11 of two_tile_layout hold whole short segments only
SHORT_PER_TILE = TILE // 7                        # 585 segments of 7 elements and one of 1 fill a tile exactly


def two_tile_layout(cus=256):
    """(n, off, names): n = (16 cus + 3) tiles + 77, so a workgroup of sample_tile_kernel walks two tiles: tiles 2g and 2g + 1.
    names: the segment index of 'few', 'two_edges', 'to_edge' (ends on the edge 5 T behind three empty segments, two more empty ones
    on that edge), 'from_edge' (three tiles, from that edge), 'short' (the first of the short ones), 'bulk', 'last'.

    tile 0 outside, tile 1 tail (off[0] in the middle of a workgroup's SECOND tile); 2 both, 3 lead+tail (again a second tile), 4 lead,
    5 tail, 6 both, 7 lead; 8 .. 11 not read: 4 x (585 segments of 7 and one of 1); 12 tail, 13 lead+tail: the bulk begins in tile 13
    (13 % 4 = 1) and ends in tile 16 cus + 2, the FIRST tile of the last workgroup, whose second tile lies behind off[S]."""
    T = TILE
    n = (16 * cus + 3) * T + 77
    last_tile = 16 * cus + 2
    lengths, names = [], {}

    def add(name, *ls):
        names[name] = len(lengths)
        lengths.extend(ls)

    start = T + 2000
    add("few", 300)
    add("two_edges", 3 * T + 500 - (start + 300))          # over the edges 2 T and 3 T
    add("empty", 0, 0, 0)
    add("to_edge", 5 * T - (3 * T + 500))                  # over the edge 4 T, ends on 5 T
    add("empty_on_edge", 0, 0)
    add("from_edge", 3 * T)                                # tiles 5, 6, 7
    add("short", *(([7] * SHORT_PER_TILE + [T - 7 * SHORT_PER_TILE]) * SHORT_TILES))
    add("before_bulk", T + 1500)                           # from 12 T into tile 13
    bulk_start = 13 * T + 1500
    add("bulk", last_tile * T + 1000 - bulk_start)
    add("last", 50)
    off = C.offsets_from(lengths, start=start)
    assert int(off[names["bulk"]]) == bulk_start and int(off[-1]) == last_tile * T + 1050 < n
    return n, off, names


def weightless_chunk(off, s):
    """[a, b): the elements of segment s in the 256 tiles from its first tile + 256 on, the walk's second chunk; the tests zero them"""
    a, b = int(off[s]), int(off[s + 1])
    ta = a // TILE
    return min((ta + WALK_TILES) * TILE, b), min((ta + 2 * WALK_TILES) * TILE, b)


def chunk_targets(m, off, s, chunks=8):
    """1, total, and the prefix and prefix + 1 of the first `chunks` chunk ends of segment s"""
    f = walk_facts(m, off, s)
    t = [1, sum(f["pieces"])]
    for p in f["chunk_prefix"][:chunks]:
        t += [p, p + 1]
    return t


GROUP_ONE_TILE, GROUP_TWO_TILES = 1, 0            # segments of group_layout


def group_layout():
    """(n, off): segment 0 = [501, T + 1001): pieces of 3595 and 1001 elements, both partial, the first one off the 4-element grid;
    segment 1 = [T + 1001, T + 4001): inside tile 1, off the grid, 11 whole groups of 256 and one of 184"""
    off = np.array([501, TILE + 1001, TILE + 4001], dtype=np.uint64)
    return 2 * TILE + 1000, off


def group_edges(m, off, s):
    """[(edge, prefix)]: for every piece of segment s and every end of a 256-element group of it (the piece's end included), the index
    in the segment and the segment's running mass in front of it"""
    o = np.asarray(off).astype(np.int64)
    a, b = int(o[s]), int(o[s + 1])
    run = np.concatenate([[0], np.cumsum(np.asarray(m, dtype=np.int64))])
    out = []
    for t in range(a // TILE, (b - 1) // TILE + 1 if b > a else 0):
        ps, pe = max(a, t * TILE), min(b, (t + 1) * TILE)
        for e in list(range(ps + GROUP, pe, GROUP)) + [pe]:
            out.append((e - a, int(run[e] - run[a])))
    return out


def group_targets(m, off, s):
    """the running mass at every group boundary of segment s and that plus 1, without 0, repeats and what lies above the total"""
    edges = group_edges(m, off, s)
    total = edges[-1][1] if edges else 0
    out = []
    for _, p in edges:
        for t in (p, p + 1):
            if 1 <= t <= total and t not in out:
                out.append(t)
    return out


SECOND_TRIP_R = 3


def second_trip_layout(cus=256, seed=6):
    """(n, off, names): 48 cus segments of 0 .. 7 elements drawn 3 times each: 144 cus slots on a draw grid of 32 cus workgroups of 4
    waves, so the slots from 128 cus on belong to the second trip.  Among the last 5 cus segments (first slot >= 129 cus): 'two_tiles',
    'long' (300 tiles: two walk chunks), 'empty' and 'one_tile' (3000 elements inside one tile)"""
    rng = np.random.default_rng(seed)
    nseg = 48 * cus
    lengths = rng.integers(0, 8, nseg)
    first = nseg - 5 * cus
    names = {"two_tiles": first + cus, "long": first + 2 * cus, "empty": first + 3 * cus, "one_tile": first + 4 * cus}
    lengths[names["two_tiles"]] = TILE + 700
    lengths[names["long"]] = 299 * TILE + 9
    lengths[names["empty"]] = 0
    lengths[names["one_tile"]] = 3000
    off = C.offsets_from(lengths, start=5)
    # the pieces as named: move the starts where the random lengths before them put them badly
    for name, want_tiles in (("two_tiles", 2), ("long", 300), ("one_tile", 1)):
        s = names[name]
        a, b = int(off[s]), int(off[s + 1])
        pad = 0
        while (b + pad - 1) // TILE - (a + pad) // TILE + 1 != want_tiles:
            pad += 512
        if pad:
            lengths[s - 1] += pad
            off = C.offsets_from(lengths, start=5)
    return int(off[-1]) + 3, off, names


HUGE_LENGTH = (1 << 22) + 3 * TILE + 5


def huge_total_layout():
    """(n, off): one segment of 2^22 + 3 tiles + 5 elements from element 7 on (1028 tiles: five walk chunks), 9 elements behind it"""
    off = np.array([7, 7 + HUGE_LENGTH], dtype=np.uint64)
    return 7 + HUGE_LENGTH + 9, off
