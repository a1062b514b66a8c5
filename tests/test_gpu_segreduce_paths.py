"""rsx_segmented_reduce on the paths of rsx_segreduce.hpp (and the ids walk of rsx_scan_by_key.hpp) that tests/test_gpu_segreduce.py never
reaches: up to 16 segment starts in one thread and 4096 in one tile, empty segments among one-element ones; off[0] and off[S] at every
position of a thread and a tile that the kernels tell apart; a workgroup of the join that takes two open tiles, a one-wave join before
and after a four-wave one, 15 partials per thread; more segments than the join has threads; the arg ops without a value output; and one
engine through calls of very different sizes.

The layouts are held in tests/_segreduce_ref.py (tests/test_segreduce.py checks from the offsets alone that each reaches its path, and
holds reduce_fast to reduce_oracle).  run, the checks, sentinels and guard bands are those of test_gpu_segreduce.py: integers, float
min / max and every index are compared exactly, float sums bit for bit with model_sum and inside check_float_sum's bound.
"""
import numpy as np
import pytest

import _segreduce_ref as R
from _segreduce_ref import OPS, reduce_fast
from test_gpu_segreduce import check_any, check_exact, check_float_sum, engine, make_values, run, same

pytestmark = pytest.mark.gpu

ARG = ("argmin", "argmax")
NO_INDEX = 0xFFFFFFFF


def check_fast(vals, idx, v, off, op):
    """check_exact against reduce_fast, for layouts of very many segments (not for float sums: those go to check_float_sum)"""
    assert not (op == "sum" and v.dtype.kind == "f")
    want, widx = reduce_fast(v, off, op)
    if vals is not None:
        have = vals.view(v.dtype)
        bad = np.flatnonzero(~same(have, want))
        assert bad.size == 0, f"{op} {v.dtype.name}: segments {bad[:8].tolist()} (of {bad.size}): {have[bad[:8]].tolist()} != {want[bad[:8]].tolist()}"
    if widx is not None:
        have = idx.view(np.int32).astype(np.int64)
        bad = np.flatnonzero(have != widx)
        assert bad.size == 0, f"{op} {v.dtype.name}: indices of segments {bad[:8].tolist()} (of {bad.size}): {have[bad[:8]].tolist()} != {widx[bad[:8]].tolist()}"
    else:
        assert idx is None


# -- R1. dense offsets ------------------------------------------------------------------------------------------------------------------

DENSE_CASES = [(np.float32, op) for op in OPS] + [(np.int64, op) for op in OPS] + [(vt, op) for vt in (np.int32, np.float64) for op in ("sum", "argmax")]


@pytest.mark.parametrize("name", list(R.DENSE))
def test_dense_offsets(rsx, name):
    """two tiles and 37 elements of segments of 0 to 16 elements: every segment between two flags of one thread is stored by ids.last.
    The arg ops run again without a value output: the indices are the same and their bands stay intact (run checks them)."""
    n, off = R.DENSE[name]()
    rng = np.random.default_rng(300 + list(R.DENSE).index(name))
    eng = engine(rsx)
    for vt, op in DENSE_CASES:
        for ties in ((False, True) if op in ARG else (False,)):
            v = make_values(vt, n, rng, op, off, ties=ties)
            vals, idx, _ = run(rsx, v, off, op, eng=eng)
            if op == "sum" and v.dtype.kind == "f":
                check_float_sum(vals, v, off, name)
            else:
                check_fast(vals, idx, v, off, op)
            if op in ARG:
                vals, idx2, _ = run(rsx, v, off, op, eng=eng, want_values=False)
                assert vals is None and np.array_equal(idx2, idx)
    eng.sync()


# -- R2. where off[0] and off[S] stand ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vt,op", [(np.float32, "sum"), (np.float32, "min"), (np.float32, "argmax"), (np.int32, "sum"), (np.int32, "argmin")],
                         ids=lambda x: x if isinstance(x, str) else np.dtype(x).name)
def test_start_and_stop_positions(rsx, vt, op):
    """one segment [lo, hi) for every pair of positions, and two segments around every boundary, in three tiles; outside [off[0], off[S])
    the values are NaN, or the integer that would win"""
    rng = np.random.default_rng(400 + OPS.index(op))
    eng = engine(rsx)
    for n, off in R.position_layouts():
        check_any(rsx, make_values(vt, n, rng, op, off), off, op, eng=eng, what=str(off.tolist()))
    eng.sync()


# -- R3. two joins per workgroup -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vt,op", [(np.float32, "sum"), (np.int32, "argmax"), (np.float64, "min")], ids=lambda x: x if isinstance(x, str) else np.dtype(x).name)
def test_two_joins_per_workgroup(rsx, vt, op):
    """4401 tiles: workgroup 5 of the join takes a one-wave join and then a four-wave one, workgroup 105 the other way round, workgroup
    125 joins on its second trip only; one join has 15 partials per thread; the tile kernel's workgroups carry s0 over a boundary"""
    n, off = R.layout_two_joins()
    sched = R.join_schedule(n, off)
    assert [len(sched[w]) for w in (5, 105, 125)] == [2, 2, 1] and R.chunk_of(n) == 2
    rng = np.random.default_rng(500 + OPS.index(op))
    if op == "sum":
        v = make_values(vt, n, rng, op, off)
    elif op == "argmax":
        v = rng.integers(-1000, 1001, n).astype(vt)                # (every maximum is attained many times: the first wins)
        v[:int(off[0])] = 2000
        v[int(off[-1]):] = 2000
    else:
        v = rng.uniform(0.5, 2.0, n).astype(vt)                    # (positive: a 0 that leaked in from a dead lane would win)
        v[:int(off[0])] = np.nan
        v[int(off[-1]):] = np.nan
    eng = check_any(rsx, v, off, op, what="two joins per workgroup")
    eng.sync()


# -- R4. more segments than the join has threads ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vt,op,want_values", [(np.int64, "sum", True), (np.float32, "argmin", False), (np.float64, "max", True)],
                         ids=["int64 sum", "float32 argmin without values", "float64 max"])
def test_more_segments_than_join_threads(rsx, vt, op, want_values):
    """2^20 + 4099 segments: part (1) of the join goes round twice; every empty segment holds the identity, or index 0xFFFFFFFF"""
    n, off = R.layout_million_segments()
    assert len(off) - 1 > 256 * 16 * 256
    rng = np.random.default_rng(600 + OPS.index(op))
    v = make_values(vt, n, rng, op, off)
    vals, idx, eng = run(rsx, v, off, op, want_values=want_values)
    assert (vals is None) == (not want_values)
    check_fast(vals, idx, v, off, op)
    empty = np.flatnonzero(np.diff(off.astype(np.int64)) == 0)
    assert empty.size > (1 << 19)
    if idx is not None:
        assert np.all(idx[empty] == NO_INDEX) and not np.any(np.delete(idx, empty) == NO_INDEX)
    if vals is not None:
        assert np.all(vals.view(v.dtype)[empty] == R.identity(vt, op))
    eng.sync()


# -- R5. one engine through all of it --------------------------------------------------------------------------------------------------------

def test_one_engine_through_large_and_small_calls(rsx):
    """the partials and open_seg words of a 258-tile call lie in the scratch when the small calls run: every result equals a fresh
    engine's bit for bit"""
    rng = np.random.default_rng(700)
    calls = [R.layout_long(258), R.layout_every_element(), R.layout_all_empty(), (0, np.zeros(4, dtype=np.uint64)), R.layout_ragged()]
    shared = engine(rsx)
    for first in (0, 1):
        for i, (n, off) in enumerate(calls):
            op = ("sum", "argmax")[(i + first) % 2]
            v = make_values(np.float32, n, rng, op, off, ties=op == "argmax")
            vals, idx, _ = run(rsx, v, off, op, eng=shared)
            fresh_vals, fresh_idx, fresh = run(rsx, v, off, op)
            fresh.sync()
            assert np.array_equal(vals, fresh_vals), (i, op)
            assert (idx is None and fresh_idx is None) or np.array_equal(idx, fresh_idx), (i, op)
            if op == "sum":
                check_float_sum(vals, v, off, f"call {i}")
            else:
                check_exact(vals, idx, v, off, op)
    shared.sync()
