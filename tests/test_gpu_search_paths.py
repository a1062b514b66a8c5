"""rsx_segmented_search where a workgroup walks two tiles of queries.  search_kernel keeps what it staged (`staged`, `staged_seg`) from a
workgroup's first tile to its second and restages only when the path or the segment changes, so what matters is the ordered pair of
(path, segment) of a workgroup's two tiles.  tests/test_gpu_search.py has one such run (uint64, ragged, ascending) and asserts only that
the three paths occur somewhere.

The layouts are held in tests/_search_ref.py; each has a little more than 1024 x 16 x CUs queries.  _search_ref.tile_walk computes from a
layout the (path, segment) of every tile of every workgroup, and tests/test_search.py asserts at 256 CUs that each layout holds the pairs
it is named for:
  even_mixed    the even form (qoff == NULL, s_first = a / qper), 1536 queries a segment: all seven pairs of different paths or segments
  even_same     the even form, 2048 queries a segment: (resident, resident) and (sampled, sampled) of the same segment: nothing restaged
  one_segment   off == qoff == NULL: resident (4000 keys) and sampled (50000 keys), the same segment in both tiles
  ragged_dead   ragged queries; dead tiles at the head and the tail of the grid beside live ones in the same workgroup; one tile of
                queries per segment, so that every second tile restages, with 4-byte keys at starts of every residue mod 4
Here the pairs are asserted again for the device's own CU count, before the run.  Every case runs left and right (both_sides) against
search_oracle: exact equality, the sentinel outside [qoff[0], qoff[S]), a guard band behind the output.  Queries are drawn, per
segment, from the segment's own keys, their neighbours in the order, the type's extremes and random keys.  Engines have capacity 4096.
"""
import numpy as np
import pytest

import _search_ref as R
from _search_ref import extremes, neighbours, segments, tile_walk
from test_gpu_search import both_sides, engine
from test_gpu_segmented import _torch
from test_gpu_unique import FILL32
from test_search import kinds_of, ragged_case, random_keys

pytestmark = pytest.mark.gpu


def device_cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def haystack(dt, rng, descending, off, n):
    """n keys, every segment sorted in the engine's order (every other one from a narrow range: runs of equal keys), random keys outside"""
    if off is None:
        return ragged_case(dt, rng, descending, [n], start=0, tail=0)[0]
    o = off.astype(np.int64)
    keys, again = ragged_case(dt, rng, descending, np.diff(o).tolist(), start=int(o[0]), tail=n - int(o[-1]))
    assert np.array_equal(again, off) and keys.size == n
    return keys


def drawn_queries(keys, off, nq, qoff, rng):
    """per segment, draws from what test_search.query_pool holds: the segment's keys, their neighbours, the extremes, random keys; random
    keys outside [qoff[0], qoff[S])"""
    dt = keys.dtype
    q = random_keys(dt, nq, rng)
    for a, b, c, d in segments(keys.size, off, nq, qoff):
        pool = np.concatenate([neighbours(keys[a:b]), extremes(dt), random_keys(dt, 64, rng)])
        q[c:d] = pool[rng.integers(0, pool.size, d - c)]
    return q


def two_tiles(walk):
    return all(len(g) == 2 for g in walk[:-1]) and 1 <= len(walk[-1]) <= 2


def search_case(rsx, dt, descending, n, off, nq, qoff, seed, sampled=True, what=""):
    rng = np.random.default_rng(seed)
    keys = haystack(dt, rng, descending, off, n)
    queries = drawn_queries(keys, off, nq, qoff, rng)
    lo, hi = both_sides(rsx, keys, off, queries, qoff, descending, engine(rsx, dt, descending, sampled=sampled), what)
    live = lo != FILL32
    assert np.any(hi[live] > lo[live]) and np.any(hi[live] == lo[live])          # present and absent queries both occur


MIXED = {("resident", "resident", "other"), ("resident", "sampled", "other"), ("sampled", "resident", "other"), ("resident", "direct", None),
         ("direct", "resident", None), ("sampled", "direct", None), ("direct", "sampled", None)}


@pytest.mark.parametrize("dt,descending", [(np.uint32, False), (np.float32, True)], ids=["uint32-asc", "float32-desc"])
def test_even_form_every_change_of_path_or_segment(rsx, dt, descending):
    cus = device_cus()
    n, off, nq = R.even_layout(cus, 1536)
    walk = tile_walk(n, off, nq, None, cus)
    assert two_tiles(walk) and kinds_of(walk) >= MIXED
    search_case(rsx, dt, descending, n, off, nq, None, 700 + int(descending), what="even_mixed")


def test_even_form_without_the_sampled_path(rsx):
    """an engine created under RSX_SEARCH_SAMPLED=0: the tiles that would be sampled bisect global memory, between resident tiles"""
    cus = device_cus()
    n, off, nq = R.even_layout(cus, 1536)
    walk = tile_walk(n, off, nq, None, cus, sampled=False)
    assert two_tiles(walk) and not any(p == "sampled" for g in walk for p, _ in g)
    assert kinds_of(walk) >= {("resident", "resident", "other"), ("resident", "direct", None), ("direct", "resident", None), ("direct", "direct", None)}
    with_samples = tile_walk(n, off, nq, None, cus)
    assert [[("direct", None) if p == "sampled" else (p, s) for p, s in g] for g in with_samples] == walk
    search_case(rsx, np.uint32, False, n, off, nq, None, 702, sampled=False, what="even_mixed, direct")


def test_even_form_two_tiles_inside_one_segment(rsx):
    cus = device_cus()
    n, off, nq = R.even_layout(cus, 2048)
    walk = tile_walk(n, off, nq, None, cus)
    assert two_tiles(walk) and kinds_of(walk) == {("resident", "resident", "same"), ("sampled", "sampled", "same")}
    search_case(rsx, np.uint64, False, n, off, nq, None, 703, what="even_same")


@pytest.mark.parametrize("L,path", [(4000, "resident"), (50000, "sampled")])
def test_one_segment(rsx, L, path):
    cus = device_cus()
    n, off, nq = R.one_segment_layout(cus, L)
    walk = tile_walk(n, off, nq, None, cus)
    assert two_tiles(walk) and walk[:-1] == [[(path, 0), (path, 0)]] * (len(walk) - 1) and walk[-1] == [("direct", None)]
    search_case(rsx, np.uint32, False, n, off, nq, None, 704 + L, what=f"one segment of {L}")


@pytest.mark.parametrize("dt,descending", [(np.uint32, False), (np.float32, True)], ids=["uint32-asc", "float32-desc"])
def test_ragged_form_dead_tiles_and_restaged_segments(rsx, dt, descending):
    cus = device_cus()
    n, off, nq, qoff = R.ragged_dead_layout(cus)
    walk = tile_walk(n, off, nq, qoff, cus)
    S = len(off) - 1
    assert two_tiles(walk) and walk[0] == [(None, None)] * 2 and walk[1] == [(None, None), ("resident", 0)]
    assert walk[-2] == [("resident", S - 1), (None, None)] and walk[-1] == [(None, None)] * 2
    assert kinds_of(walk) >= {("resident", "resident", "other"), ("resident", "sampled", "other"), ("sampled", "resident", "other")}
    search_case(rsx, dt, descending, n, off, nq, qoff, 710 + int(descending), what="ragged_dead")
