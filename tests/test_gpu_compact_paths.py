"""rsx_segmented_compact where a workgroup walks two tiles: what compact_count_kernel and compact_write_kernel carry from a workgroup's
first tile to its second — the gallop starts `from` and `wfrom`, the LDS staging that is reused after the barrier at the end of a tile,
the early `continue` of a tile without a live element — on every key width, form and flag that tests/test_gpu_compact.py runs on single
tiles only.

The layout is _compact_ref.walk_layout(CUs): 4096 x 16 x CUs + 4096 + 5 elements and 1322 segments.  tests/test_compact.py asserts from
the layout alone, at 256 CUs, that it holds: a workgroup of a dead and a live tile and one of a live and a dead tile, wholly dead
workgroups on both sides, more than 600 offsets in a workgroup's first tile (a carried gallop start beyond 600), 300 empty segments
exactly on the edge between a workgroup's two tiles, more than 256 offsets in a second tile, a tile that spans segments before and
behind one that is staged, a segment over thousands of workgroups, and the ragged lengths of the other suites.  It also shows, with
_compact_ref.compact_tiled, three slips in the carried state that this layout notices and the older ones do not all notice.

run / check, sentinels and guard bands are those of test_gpu_compact.py: every comparison is exact equality of bits with compact_oracle,
keys and mask bytes outside [off[0], off[S]) are random, every engine has capacity 4096.  Each case makes at most two calls: the referee
takes one to two seconds a call at this size.

Not included: a workgroup that walks three tiles (n > 2 x 4096 x 4096 x 16 x CUs / 16).  It runs the same loop body a third time and
would double the memory and the referee's time of every case here.
"""
import numpy as np
import pytest

import _compact_ref as R
from _compact_ref import compact_oracle, keep_flags
from test_compact import drawn_bounds
from test_gpu_compact import CAP, check, random_mask, run
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL
from test_search import random_keys

pytestmark = pytest.mark.gpu


def walk_case(dt, rng):
    """(keys, off) on walk_layout of this device: random keys, every other segment from a narrow range (ties with the bounds)"""
    t = _torch()
    cus = t.cuda.get_device_properties(0).multi_processor_count
    n, off = R.walk_layout(cus)
    tiles, _, chunk, _ = R.grid(n, cus)
    assert chunk == 2 and tiles == 16 * cus + 2
    keys = random_keys(dt, n, rng)
    o = off.astype(np.int64)
    for s in range(1, len(off) - 1, 2):
        keys[o[s]:o[s + 1]] = random_keys(dt, int(o[s + 1] - o[s]), rng, narrow=True)
    return keys, off


def tied_bounds(keys, off, rng, descending=False):
    bounds = drawn_bounds(keys, off, rng)
    assert np.any(keep_flags(keys, off, bounds=bounds, descending=descending) != keep_flags(keys, off, bounds=bounds, descending=descending, strict=True)), "no key ties with its bound"
    return bounds


def calls_u64_mask(keys, off, rng):
    mask = random_mask(keys.size, rng)
    return [dict(mask=mask), dict(mask=mask, partition=True)]


def calls_u64_bound(keys, off, rng):
    bounds = tied_bounds(keys, off, rng)
    return [dict(bounds=bounds, strict=True), dict(bounds=bounds, partition=True, invert=True)]


def calls_f32_desc(keys, off, rng):
    bounds = tied_bounds(keys, off, rng, descending=True)
    return [dict(bounds=bounds, partition=True, descending=True), dict(bounds=bounds, descending=True)]


def calls_index_only(keys, off, rng):
    mask = random_mask(keys.size, rng)
    return [dict(mask=mask, want=("index",)), dict(mask=mask, partition=True, want=("index",))]


def calls_count_only(keys, off, rng):
    return [dict(mask=random_mask(keys.size, rng), want=()), dict(bounds=tied_bounds(keys, off, rng), want=())]


def calls_shifted(keys, off, rng):
    mask = random_mask(keys.size, rng)
    shifts = dict(mask_shift=3, key_shift=1, index_shift=1)                      # the byte loads of the mask in every tile
    return [dict(mask=mask, **shifts), dict(mask=mask, partition=True, **shifts)]


CASES = {"uint64-mask": (np.uint64, calls_u64_mask), "uint64-bound-strict-invert": (np.uint64, calls_u64_bound),
         "float32-descending-bound": (np.float32, calls_f32_desc), "int64-mask-index-only": (np.int64, calls_index_only),
         "uint32-count-only": (np.uint32, calls_count_only), "uint64-mask-shifted": (np.uint64, calls_shifted)}


@pytest.mark.parametrize("name", list(CASES))
def test_two_tiles_per_workgroup(rsx, name):
    dt, calls = CASES[name]
    rng = np.random.default_rng(600 + list(CASES).index(name))
    keys, off = walk_case(dt, rng)
    eng = None
    for kw in calls(keys, off, rng):
        got, eng = run(rsx, keys, off, eng=eng, **kw)
        assert set(got) == set(kw.get("want", ("keys", "index"))) | {"koff"}
        ref_kw = {k: v for k, v in kw.items() if k in ("mask", "bounds", "partition", "invert", "strict", "descending")}
        check(got, compact_oracle(keys, off, **ref_kw), f"{name} {sorted(k for k in kw if k not in ('mask', 'bounds'))}")
    eng.sync()


def test_capture_and_replay_with_offsets_moving_across_the_tile_edge(rsx):
    """one captured call (uint64, mask form, compact mode), replayed twice: before each replay the mask is rewritten and the 300 empty
    segments on the edge between the two tiles of workgroup 2 move down by 1 and by 2, from the start of the workgroup's second tile into
    the end of its first"""
    t = _torch()
    rng = np.random.default_rng(620)
    keys, off = walk_case(np.uint64, rng)
    n, nseg = keys.size, len(off) - 1
    edge = np.flatnonzero(off == 5 * R.TILE)
    assert edge.size == 302 and np.all(np.diff(edge) == 1)                        # the end of a segment, 300 empty segments, the burst's first (empty) one
    side = t.cuda.Stream()
    eng = rsx.Engine(np.uint64, CAP)
    eng.set_stream(side.cuda_stream)
    mask = random_mask(n, rng)
    kd, od, md = dev(t, keys), dev(t, off), dev(t, mask)
    kout, iout, koff = (dev(t, np.full(nb, FILL, dtype=np.uint8)) for nb in (8 * n, 4 * n, 8 * (nseg + 1)))

    def call():
        eng.segmented_compact(kd.data_ptr(), n, od.data_ptr(), nseg, md.data_ptr(), None, kout.data_ptr(), iout.data_ptr(), koff.data_ptr())

    def result():
        return {"keys": kout.cpu().numpy().view(np.uint64), "index": iout.cpu().numpy().view(np.uint32), "koff": koff.cpu().numpy().view(np.uint64)}

    call()                                                                       # eager: the first call of an engine allocates its scratch
    eng.sync()
    check(result(), compact_oracle(keys, off, mask=mask), "eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for rep in range(2):
        mask = random_mask(n, rng)
        moved = off.copy()
        moved[edge[:301]] = 5 * R.TILE - 1 - rep                                 # (with the end of the segment before them: non-decreasing)
        assert np.all(np.diff(moved.astype(np.int64)) >= 0) and int(moved[edge[301]]) == 5 * R.TILE
        md.copy_(t.from_numpy(mask.view(np.int8)))
        od.copy_(t.from_numpy(moved.view(np.int64)))
        for buf in (kout, iout, koff):
            buf.fill_(FILL - 256)
        graph.replay()
        t.cuda.synchronize()
        check(result(), compact_oracle(keys, moved, mask=mask), f"replay {rep}")
    del graph
    eng.sync()
