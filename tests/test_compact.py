"""CPU checks of the stream compaction: header, exports, binding and the Python callables agree on rsx_segmented_compact; the two forms
of the host referee (tests/_compact_ref.py) agree with each other and with a hand-made case; the layouts the GPU tests run reach the
paths they are named after; the tiled mirror of the kernels' arithmetic equals the referee, and its named faults show what walk_layout
notices that the older layouts do not; and the call and the torch helpers fail loudly instead of working on the CPU."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import _compact_ref as R
from _compact_ref import compact_loop, compact_oracle, grid, keep_flags, tile_facts
from _search_ref import extremes, neighbours
from test_search import HEADER_DTYPES, header_text, random_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_in_header_exports_and_binding(rsx):
    raw = header_text()
    for name, value in (("PARTITION", 8), ("INVERT", 16), ("STRICT", 32)):
        assert re.search(r"#define\s+RSX_COMPACT_%s\s+%d\b" % (name, value), raw), name
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_compact\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_compact is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_keys", "uint64_t n", "const uint64_t* d_offsets", "uint64_t num_segments",
                      "const uint8_t* d_mask", "const void* d_bounds", "uint32_t flags", "void* d_keys_out", "uint32_t* d_index_out",
                      "uint64_t* d_kept_offsets_out"]
    assert "rsx_segmented_compact" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_compact
    P = C.c_void_p
    assert fn.argtypes == [P, P, C.c_uint64, P, C.c_uint64, P, P, C.c_uint32, P, P, P]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_compact\b", out)
    for name in ("segmented_compact", "masked_select", "nonzero", "compact_rows"):
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_compact)
    # the binding's constants are the header's, the referee's, and disjoint from the family's bits 0 - 2
    assert (rsx.COMPACT_PARTITION, rsx.COMPACT_INVERT, rsx.COMPACT_STRICT) == (8, 16, 32) == (R.PARTITION, R.INVERT, R.STRICT)
    assert (rsx.COMPACT_PARTITION | rsx.COMPACT_INVERT | rsx.COMPACT_STRICT) & (rsx.UNIQUE_CONSECUTIVE | rsx.SCAN_EXCLUSIVE | rsx.SEARCH_RIGHT) == 0


def test_grid_constants_match_the_kernel_headers():
    """tests/_compact_ref.py states the kernels' grid; the numbers are those of the headers"""
    src = lambda f: open(os.path.join(ROOT, "radix-sort_amd", "csrc", f)).read()
    num = lambda text, name: int(re.search(name + r"\s*=\s*(\d+)", text).group(1))
    uniq = src("rsx_unique.hpp")
    assert num(uniq, "kUniqThreads") == R.THREADS and num(uniq, "kUniqKpt") * R.THREADS == R.TILE
    assert num(src("rsx_scan.hpp"), "kScanTiles") == R.SCAN_BLOCK
    comp = src("rsx_compact.hpp")
    assert (num(comp, "kCompactPartition"), num(comp, "kCompactInvert"), num(comp, "kCompactStrict")) == (R.PARTITION, R.INVERT, R.STRICT)
    import test_search
    assert R.LENGTHS == test_search.LENGTHS


def flag_combinations(bound):
    return [dict(partition=p, invert=i, strict=s) for p, i, s in itertools.product((False, True), (False, True), (False, True) if bound else (False,))]


def small_case(dt, rng, descending):
    """a ragged case small enough for the loop: off[0] = 2, empty segments, narrow keys (ties with the bounds) every other segment"""
    lengths = [0, 1, 5, 0, 17, 33, 2, 0, 64, 3]
    off = R.offsets_from(lengths, start=2)
    n = int(off[-1]) + 3
    keys = random_keys(dt, n, rng)
    for s, L in enumerate(lengths):
        if s % 2 == 1:
            keys[int(off[s]):int(off[s]) + L] = random_keys(dt, L, rng, narrow=True)
    mask = R.MASK_BYTES[rng.integers(0, R.MASK_BYTES.size, n)]
    return keys, off, mask, drawn_bounds(keys, off, rng)


def drawn_bounds(keys, off, rng):
    """one bound per segment: one of the segment's own keys, a neighbour of one in the order, or one of the type's extremes"""
    ext = extremes(keys.dtype)
    out = np.empty(len(off) - 1, dtype=keys.dtype)
    for s in range(len(off) - 1):
        seg = keys[int(off[s]):int(off[s + 1])]
        pool = ext if seg.size == 0 or s % 5 == 4 else neighbours(seg[rng.integers(0, seg.size, 1)])
        out[s] = pool[rng.integers(0, pool.size)]
    return out


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt", HEADER_DTYPES, ids=lambda d: np.dtype(d).name)
def test_referee_forms_agree(dt, descending):
    rng = np.random.default_rng(HEADER_DTYPES.index(dt) * 2 + int(descending))
    keys, off, mask, bounds = small_case(dt, rng, descending)
    u = keys.view(R.order_map(keys).dtype)
    n, lo, hi = keys.size, int(off[0]), int(off[-1])
    for form, kw in [("mask", kw) for kw in flag_combinations(False)] + [("bound", kw) for kw in flag_combinations(True)]:
        args = dict(mask=mask) if form == "mask" else dict(bounds=bounds)
        a = compact_oracle(keys, off, descending=descending, **args, **kw)
        b = compact_loop(keys, off, descending=descending, **args, **kw)
        for x, y, what in zip(a, b, ("keys", "index", "koff", "written")):
            assert np.array_equal(x.view(u.dtype) if what == "keys" else x, y.view(u.dtype) if what == "keys" else y), (form, kw, what)
        kout, iout, koff, written = a
        assert koff[0] == 0 and np.all(np.diff(koff) >= 0) and koff[-1] <= hi - lo
        if kw["partition"]:
            assert np.array_equal(np.flatnonzero(written), np.arange(lo, hi))
            for s in range(len(off) - 1):                        # a permutation of the segment whose index output says where from
                a0, a1 = int(off[s]), int(off[s + 1])
                assert sorted(iout[a0:a1].tolist()) == list(range(a1 - a0))
                assert np.array_equal(kout[a0:a1].view(u.dtype), u[a0 + iout[a0:a1]])
        else:
            assert np.array_equal(np.flatnonzero(written), np.arange(int(koff[-1])))
        # invert keeps exactly the others
        inv = compact_oracle(keys, off, descending=descending, **args, **{**kw, "invert": not kw["invert"]})
        assert np.array_equal(koff + inv[2], np.asarray(off).astype(np.int64) - lo)
    # one segment, offsets None
    for kw in flag_combinations(False):
        a, b = compact_oracle(keys, None, mask=mask, **kw), compact_loop(keys, None, mask=mask, **kw)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    # ties with the bound occur, and strict differs from non-strict exactly by them
    le = keep_flags(keys, off, bounds=bounds, descending=descending)
    lt = keep_flags(keys, off, bounds=bounds, descending=descending, strict=True)
    assert np.all(lt <= le) and np.any(lt != le)


def test_hand_made_example():
    """off[0] = 1, an empty segment, a key equal to its bound, keys outside the segments that would be kept"""
    keys = np.array([1, 5, 2, 9, 2, 7, 3, 8, 0], dtype=np.uint32)
    off = np.array([1, 5, 5, 8], dtype=np.uint64)                               # [5 2 9 2] [] [7 3 8]
    mask = np.array([1, 0, 2, 0, 0xFF, 0x80, 0, 1, 1], dtype=np.uint8)
    bounds = np.array([2, 4, 7], dtype=np.uint32)
    for form in (compact_oracle, compact_loop):
        k, i, koff, w = form(keys, off, mask=mask)
        assert koff.tolist() == [0, 2, 2, 4] and w.tolist() == [True] * 4 + [False] * 5
        assert k[:4].tolist() == [2, 2, 7, 8] and i[:4].tolist() == [1, 3, 0, 2]
        k, i, koff, w = form(keys, off, mask=mask, invert=True)
        assert koff.tolist() == [0, 2, 2, 3] and k[:3].tolist() == [5, 9, 3] and i[:3].tolist() == [0, 2, 1] and int(w.sum()) == 3
        k, i, koff, w = form(keys, off, mask=mask, partition=True)
        assert koff.tolist() == [0, 2, 2, 4] and w.tolist() == [False] + [True] * 7 + [False]
        assert k[1:8].tolist() == [2, 2, 5, 9, 7, 8, 3] and i[1:8].tolist() == [1, 3, 0, 2, 0, 2, 1]
        k, i, koff, w = form(keys, off, bounds=bounds)                           # k <= b
        assert koff.tolist() == [0, 2, 2, 4] and k[:4].tolist() == [2, 2, 7, 3] and i[:4].tolist() == [1, 3, 0, 1]
        k, i, koff, w = form(keys, off, bounds=bounds, strict=True)              # k < b
        assert koff.tolist() == [0, 0, 0, 1] and k[:1].tolist() == [3] and i[:1].tolist() == [1]
        k, i, koff, w = form(keys, off, bounds=bounds, descending=True)          # k >= b
        assert koff.tolist() == [0, 4, 4, 6] and k[:6].tolist() == [5, 2, 9, 2, 7, 8] and i[:6].tolist() == [0, 1, 2, 3, 0, 2]
        k, i, koff, w = form(keys, off, bounds=bounds, descending=True, strict=True, invert=True, partition=True)       # not (k > b): k <= b first
        assert koff.tolist() == [0, 2, 2, 4] and k[1:8].tolist() == [2, 2, 5, 9, 7, 3, 8] and i[1:8].tolist() == [1, 3, 0, 2, 0, 1, 2]
        # floats in totalOrder: -0.0 before +0.0, a NaN an ordinary key; signed integers
        f = np.array([0.0, -0.0, np.nan, -1.0, np.inf], dtype=np.float32)
        k, i, koff, w = form(f, None, bounds=np.array([-0.0], dtype=np.float32))
        assert koff.tolist() == [0, 2] and i[:2].tolist() == [1, 3]
        k, i, koff, w = form(f, None, bounds=np.array([np.inf], dtype=np.float32), descending=True)
        assert koff.tolist() == [0, 2] and i[:2].tolist() == [2, 4] and np.isnan(k[0])
        s = np.array([-3, 4, 0, -1], dtype=np.int64)
        assert form(s, None, bounds=np.array([-1], dtype=np.int64))[1][:2].tolist() == [0, 3]


def test_gpu_layouts_reach_their_paths():
    """from the layouts alone: tile counts, tiles without a survivor, tiles that span segments, tiles per workgroup at 256 CUs"""
    # the ragged layout: several tiles, tiles that span segments and tiles inside one, dead positions on both sides
    n, off = R.ragged_layout()
    spans, _ = tile_facts(n, off)
    assert len(spans) == 11 and int(off[0]) == 3 and n - int(off[-1]) == 5
    assert any(s != "dead" and s > 1 for s in spans) and sum(1 for s in spans if s == 1) >= 4 and grid(n)[2] == 1
    # the mask patterns: 4 tiles in one segment
    rng = np.random.default_rng(1)
    kept = {name: tile_facts(R.PATTERN_N, None, R.pattern_mask(name, rng) != 0)[1] for name in R.PATTERNS}
    assert kept["zeros"] == [0, 0, 0, 0] and kept["ones"] == [4096, 4096, 4096, 17] and kept["alternating"] == [2048, 2048, 2048, 9]
    assert all(1800 < k < 2300 for k in kept["half"][:3]) and all(20 < k < 130 for k in kept["sparse"][:3])
    assert kept["last_of_tile"] == [0, 1, 0, 0] and R.pattern_mask("last_of_tile", rng)[2 * 4096 - 1] != 0
    assert kept["first_of_tile"] == [0, 1, 0, 0] and R.pattern_mask("first_of_tile", rng)[4096] != 0
    assert kept["hole"] == [4096, 0, 4096, 17]
    # the large run: workgroups walk two tiles, the table crosses the scan's block edge, segment 1 starts in the second tile of workgroup 0
    n, off = R.big_layout()
    tiles, npad, chunk, scan_groups = grid(n)
    assert (tiles, chunk) == (4098, 2) and npad // 16 > R.SCAN_BLOCK and scan_groups == 2
    assert int(off[1]) // R.TILE == 1 and int(off[1]) % R.TILE != 0 and 1 // chunk == 0 and int(off[-1]) < n
    # 5000 empty segments at one position
    n, off = R.empties_layout()
    d = np.diff(off.astype(np.int64))
    assert int(np.count_nonzero(d == 0)) == 5000 and len(set(off[1:-1].tolist())) == 1 and int(off[1]) % R.TILE != 0
    # off[0] and off[S] in the middle of a tile; dead tiles before, after
    n, off = R.mid_tile_layout()
    spans, _ = tile_facts(n, off)
    assert spans == ["dead", 2, 1, 1, "dead"] and int(off[0]) % R.TILE != 0 and int(off[-1]) % R.TILE != 0
    # nothing in range
    n, off = R.nothing_layout()
    assert set(tile_facts(n, off)[0]) == {"dead"}


def test_walk_layout_reaches_what_a_workgroup_carries():
    """the nine properties of walk_layout at 256 CUs, from the layout alone: grid, tile_facts and the tiles of every workgroup"""
    T = R.TILE
    n, off = R.walk_layout(256)
    o = off.astype(np.int64)
    S = o.size - 1
    assert n == R.BIG_N and grid(n)[:3] == (4098, 4112, 2) and S == 1322 and np.all(np.diff(o) >= 0) and o[-1] < n
    spans, _ = tile_facts(n, off)
    groups = R.workgroups(n, 256)
    assert len(groups) == 2049 and all(len(g) == 2 for g in groups) and groups[5] == [10, 11]
    live = lambda t: spans[t] != "dead"
    per_tile = np.bincount(o // T, minlength=len(spans) + 1)                     # offsets inside every tile
    last_seg = lambda t: int(np.searchsorted(o, min((t + 1) * T, o[-1]) - 1, side="right")) - 1       # the segment of the tile's last live element
    seen = {}                                                                     # property -> the first workgroup that shows it
    for w, (t0, t1) in enumerate(groups):
        # 1. (dead, live inside one segment whose front is dead: off[0] in its middle)
        if not live(t0) and spans[t1] == 1 and o[0] // T == t1 and o[0] % T != 0:
            seen.setdefault(1, w)
        # 2. (live, dead): off[S] in the middle of the first tile
        if live(t0) and not live(t1) and o[-1] // T == t0 and o[-1] % T != 0:
            seen.setdefault(2, w)
        # 4. at least 600 offsets of short segments in the first tile: the second tile's gallop starts beyond 600
        if live(t0) and live(t1) and per_tile[t0] >= 600 and last_seg(t0) + 1 > 600:
            first = int(np.searchsorted(o, t0 * T, side="left"))
            assert np.diff(o[first:first + 601]).tolist() == R.burst(600)
            seen.setdefault(4, w)
        # 5. at least 300 empty segments exactly at the start of the second tile, behind a segment that ends there
        at = np.flatnonzero(o == t1 * T)
        if at.size >= 301 and o[at[0] - 1] < t1 * T and live(t0) and live(t1):
            seen.setdefault(5, w)
        # 6. more than 256 offsets inside the second tile
        if per_tile[t1] > 256:
            seen.setdefault(6, w)
        # 7. (spans segments, inside one) and the reverse
        if live(t0) and live(t1) and spans[t0] > 1 and spans[t1] == 1:
            seen.setdefault("7a", w)
        if live(t0) and live(t1) and spans[t0] == 1 and spans[t1] > 1:
            seen.setdefault("7b", w)
    assert seen == {1: 1, 2: 2047, 4: 2, 5: 2, 6: 2, "7a": 3, "7b": 4}, seen
    # 3. the workgroup before the first live one and the one after the last live one exist and are wholly dead
    alive = [w for w, g in enumerate(groups) if any(live(t) for t in g)]
    assert alive == list(range(1, 2048)) and not any(live(t) for t in groups[0] + groups[2048])
    # 8. one segment covers at least three whole workgroups; 9. the issue's lengths once behind it
    d = np.diff(o)
    long = int(np.argmax(d))
    assert o[long + 1] // (2 * T) - -(-o[long] // (2 * T)) >= 3 and d[long] > 4000 * T
    assert d[long + 1:long + 1 + len(R.LENGTHS)].tolist() == R.LENGTHS and long + 1 + len(R.LENGTHS) == S - 1
    # and on another device: the same walk of two tiles
    n2, off2 = R.walk_layout(304)
    assert grid(n2, 304)[2] == 2 and len(off2) == len(off) and int(off2[-1]) < n2


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


_CASES = {}


def layout_case(name):
    """(keys, off, mask, bounds) of a layout of _compact_ref, narrow uint32 keys (ties with the bounds); drawn once"""
    if name not in _CASES:
        rng = np.random.default_rng(sorted(["ragged", "big", "empties", "mid_tile", "nothing", "walk"]).index(name))
        n, off = getattr(R, name + "_layout")()
        keys = random_keys(np.uint32, n, rng, narrow=True)
        mask = R.MASK_BYTES[rng.integers(0, R.MASK_BYTES.size, n)]
        bounds = random_keys(np.uint32, len(off) - 1, rng, narrow=True)
        _CASES[name] = keys, off, mask, bounds
    return _CASES[name]


_REFS = {}


def mask_partition_ref(name):
    """compact_oracle of the layout's mask form in partition mode (computed once: 2 s at 2^24 elements)"""
    if name not in _REFS:
        keys, off, mask, _ = layout_case(name)
        _REFS[name] = compact_oracle(keys, off, mask=mask, partition=True)
    return _REFS[name]


@pytest.mark.parametrize("name", ["ragged", "empties", "mid_tile", "nothing", "big", "walk"])
def test_tiled_mirror_equals_the_referee(name):
    """compact_tiled without a fault is compact_oracle on every layout: every flag combination on the small ones, one call per kernel
    path (staged compact, staged and per-element partition; mask and bound) on the two of 2^24 elements"""
    keys, off, mask, bounds = layout_case(name)
    if name in ("big", "walk"):
        forms = [(dict(mask=mask), dict(partition=True)), (dict(bounds=bounds), dict(strict=True, invert=True))]
    else:
        forms = [(dict(mask=mask), kw) for kw in flag_combinations(False)] + [(dict(bounds=bounds), kw) for kw in flag_combinations(True)]
    for args, kw in forms:
        ref = mask_partition_ref(name) if "mask" in args and kw == dict(partition=True) else compact_oracle(keys, off, **args, **kw)
        assert _bits_equal(R.compact_tiled(keys, off, **args, **kw), ref), (sorted(args), kw)
    if name == "ragged":                                                           # descending, 8-byte keys, one segment, another device
        k64 = keys.astype(np.float64) - 20.0
        b64 = bounds.astype(np.float64) - 20.0
        assert _bits_equal(R.compact_tiled(k64, off, bounds=b64, descending=True, partition=True, cus=3), compact_oracle(k64, off, bounds=b64, descending=True, partition=True))
        assert _bits_equal(R.compact_tiled(keys, None, mask=mask, cus=1), compact_oracle(keys, None, mask=mask))


# the layouts that test_gpu_compact.py had before walk_layout, and which of them each fault of compact_tiled leaves unchanged: on the
# three small ones no workgroup walks a second tile and no offset lies on a tile's start; on `big` workgroup 0 starts tile 1 inside the
# segment tile 0 ended in, and stages twice, but its offsets are 0, 4096 + 1000 and n - 3: none on a tile's start behind a live tile
UNCHANGED = {"gallop": ["ragged", "empties", "mid_tile"], "boundary": ["ragged", "big", "empties", "mid_tile"], "stale_stage": ["ragged", "empties", "mid_tile"]}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_walk_layout_sees_what_the_older_layouts_cannot(fault):
    """each named fault of compact_tiled changes the result on walk_layout (mask form, partition, keys and index)"""
    changed = {}
    for name in ["ragged", "big", "empties", "mid_tile", "walk"]:
        keys, off, mask, _ = layout_case(name)
        changed[name] = not _bits_equal(R.compact_tiled(keys, off, mask=mask, partition=True, fault=fault), mask_partition_ref(name))
    assert changed["walk"], f"walk_layout does not notice the fault {fault!r}"
    assert [name for name in ["ragged", "big", "empties", "mid_tile"] if not changed[name]] == UNCHANGED[fault]


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    assert lib.rsx_segmented_compact(None, None, 16, None, 1, None, None, 0, None, None, None) == 4       # a null engine is refused
    assert b"rsx_segmented_compact" in lib.rsx_last_error()
    torch = pytest.importorskip("torch")
    keys = torch.arange(10, dtype=torch.int32)
    mask = keys > 4
    offsets = torch.tensor([0, 10], dtype=torch.int64)
    with pytest.raises(ValueError):              # host tensors: no CPU fallback
        rsx.masked_select(keys, mask)
    with pytest.raises(ValueError):
        rsx.nonzero(keys)
    with pytest.raises(ValueError):
        rsx.segmented_compact(keys, offsets, mask=mask)
    with pytest.raises(ValueError):
        rsx.compact_rows(keys.reshape(2, 5), mask=mask.reshape(2, 5))
    for dt in (torch.bfloat16, torch.float16, torch.bool):       # key types outside the six: refused before the device is looked at
        k = keys.to(dt)
        with pytest.raises(TypeError):
            rsx.masked_select(k, mask)
        with pytest.raises(TypeError):
            rsx.segmented_compact(k, offsets, mask=mask)
        with pytest.raises(TypeError):
            rsx.compact_rows(k.reshape(2, 5), mask=mask.reshape(2, 5))
    with pytest.raises(TypeError):               # a mask that is neither bool nor uint8
        rsx.masked_select(keys, keys)
    if not torch.cuda.is_available():
        with pytest.raises(rsx.RadixSortError) as ei:
            rsx.Engine(np.uint32, 16).segmented_compact(16, 4, None, 1, 16, None, 16, None, 16)
        assert ei.value.status == 2              # INITIALIZATION_FAILED: no device, no silent CPU path
