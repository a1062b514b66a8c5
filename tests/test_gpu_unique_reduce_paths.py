"""rsx_segmented_unique and rsx_segmented_reduce_by_key on the paths of their shared grouping chain (unique_groups_enqueue) that the two
entry points' own suites never reach: workgroups that walk two and three tiles over ragged offsets, more than 256 offsets inside one tile,
off[0] deep in the grid and off[S] long before n after a larger call on the same engine, consecutive-mode values that are not 16-byte
aligned, one engine across entry points and shapes, capture and replay, and the written order of a float sum.

The layouts are held in tests/_unique_ref.py (tests/test_unique.py checks that each still reaches its path on 256 CUs).  The referee is
flat_unique (one stable sort for all segments; tests/test_unique.py checks it against the per-segment forms) and, over its grouping,
reduce_oracle; float sums are compared with model_sum, the association that rsx_reduce.hpp writes down, bit for bit.  run / check,
sentinels and guard bands are those of test_gpu_unique.py and test_gpu_reduce.py: every comparison is exact equality of bits, except
float min / max where NaN must match NaN.
"""
import numpy as np
import pytest

import _topk_ref as R
import _unique_ref as U
from _reduce_ref import model_sum, reduce_oracle
from _unique_ref import flat_unique
from test_gpu_float_keys import UINT
from test_gpu_reduce import KIND, OPCODE, VTYPES, boundary_layout, make_values
from test_gpu_reduce import check as red_check
from test_gpu_reduce import run as red_run
from test_gpu_segmented import LENGTHS as SORT_LENGTHS
from test_gpu_segmented import _torch, dev, offsets_from
from test_gpu_segmented import check as seg_check
from test_gpu_segmented import run as seg_run
from test_gpu_topk_shapes import expect, topk_on
from test_gpu_unique import FILL, GUARD, LENGTHS, reconstructs
from test_gpu_unique import check as uniq_check
from test_gpu_unique import run as uniq_run

pytestmark = pytest.mark.gpu

T = U.TILE
REDUCTIONS = ((np.int32, "sum"), (np.int64, "sum"), (np.float32, "min"))         # the float min carries NaN and infinities


def unique_case(rsx, x, off, cons, desc=False, eng=None):
    """every output of one unique call against flat_unique; returns the grouping for the reductions that follow"""
    g = flat_unique(x, off, desc, cons)
    got, eng = uniq_run(rsx, x, off, desc, cons, True, eng=eng)
    uniq_check(x, off, got, desc, cons, ref=g)
    reconstructs(x, off, got)
    eng.sync()
    return g


def reduce_case(rsx, x, off, cons, g, vt, op, rng, desc=False, eng=None):
    v = make_values(vt, x.size, rng, op, off)
    got, eng = red_run(rsx, x, v, off, op, desc, cons, eng=eng)
    red_check(x, v, off, got, op, desc, cons, ref=reduce_oracle(x, v, off, op, desc, cons, groups=g))
    eng.sync()


def order_case(rsx, x, off, cons, g, vt, rng, desc=False, eng=None):
    """a float sum of general values: the device's bits are model_sum's"""
    v = make_values(vt, x.size, rng, "sum", off, general=True)
    assert not np.any((v != 0) & (np.abs(v) < np.finfo(vt).tiny)), "no subnormals"
    got, eng = red_run(rsx, x, v, off, "sum", desc, cons, eng=eng)
    red_check(x, v, off, got, "sum", desc, cons, how="bound", ref=reduce_oracle(x, v, off, "sum", desc, cons, groups=g))
    eng.sync()
    want = model_sum(v, g["order"], g["heads"]).view(UINT[v.dtype])
    have = got["values"][:want.size]
    bad = np.flatnonzero(have != want)
    assert bad.size == 0, (f"{v.dtype.name} sums differ from the written order at runs {bad[:8].tolist()} (of {bad.size}, heads at "
                           f"{g['heads'][bad[:8]].tolist()}): {have[bad[:8]].tolist()} != {want[bad[:8]].tolist()}")


def both_entry_points(rsx, x, off, rng, modes=(False, True), desc=False, reductions=REDUCTIONS, orders=()):
    eng = rsx.Engine(x.dtype, x.size, payload=True, descending=desc)
    for cons in modes:
        g = unique_case(rsx, x, off, cons, desc, eng=eng)
        for vt, op in reductions:
            reduce_case(rsx, x, off, cons, g, vt, op, rng, desc, eng=eng)
        for vt in (orders.get(cons, ()) if isinstance(orders, dict) else orders):
            order_case(rsx, x, off, cons, g, vt, rng, desc, eng=eng)
    eng.close()


# -- 1. workgroups that walk two and three tiles over ragged offsets -----------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [2, 3])
def test_ragged_offsets_where_a_workgroup_walks_several_tiles(rsx, chunk):
    """n just above 2^24 / 2^25: the hand-over of the offsets walk from one tile of a workgroup to the next, runs and segments that cross
    from one workgroup's tiles into another's, a run of 70 tiles that begins in the last tile of a workgroup's range"""
    n, off, keys, _ = U.ragged_layout(chunk)
    rng = np.random.default_rng(chunk)
    # (chunk 2 has its float sums in test_float_sums_in_the_written_order; chunk 3 gets one here, where the three-tile hand-over is)
    both_entry_points(rsx, keys, off, rng, orders={True: (np.float32,)} if chunk == 3 else ())
    if chunk == 2:
        both_entry_points(rsx, keys.astype(np.int64) - 2, off, rng, modes=(False,), reductions=REDUCTIONS[1:2])


# -- 2. more than 256 offsets inside one tile ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ragged", "aligned", "chunk2"])
def test_dense_offsets(rsx, kind):
    """segments of 1 .. 3 keys (about 2000 offsets per tile: eight trips of the 256-wide walks) and blocks of 1000 empty segments mid-tile,
    on a tile edge and at off[S]; "aligned": off[S] == n, a multiple of 4096, so the last block lives in the table's extra entry"""
    n, off, keys = U.dense_layout(kind)
    rng = np.random.default_rng(["ragged", "aligned", "chunk2"].index(kind))
    both_entry_points(rsx, keys, off, rng)
    if kind == "ragged":
        both_entry_points(rsx, keys.astype(np.uint64) << np.uint64(29), off, rng, modes=(False,), reductions=REDUCTIONS[:1])


# -- 3. off[0] deep in the grid, off[S] long before n, after a larger call -----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mid", "edge", "none", "none_edge"])
def test_deep_first_offset_after_a_larger_call(rsx, kind):
    """tiles before off[0] and after off[S] take no part; what an earlier, larger call on the same engine left in the per-tile partials
    and tables must not show"""
    n, off, keys = U.deep_layout(kind)
    rng = np.random.default_rng(["mid", "edge", "none", "none_edge"].index(kind) + 30)
    big = 64 * T + 9
    for x in (keys, keys.astype(np.int64) - 2):
        for desc in (False, True):
            eng = rsx.Engine(x.dtype, big, payload=True, descending=desc)
            for cons in (False, True):
                one = np.full(big, 7, dtype=x.dtype)                           # the larger call: one run over every tile
                ones = make_values(np.float64, big, rng, "sum")
                g1 = unique_case(rsx, one, None, cons, desc, eng=eng)
                got, _ = red_run(rsx, one, ones, None, "sum", desc, cons, eng=eng)
                red_check(one, ones, None, got, "sum", desc, cons, ref=reduce_oracle(one, ones, None, "sum", desc, cons, groups=g1))
                g = unique_case(rsx, x, off, cons, desc, eng=eng)
                assert (int(g["run_offsets"][-1]) == 0) == kind.startswith("none")
                for vt, op in REDUCTIONS:
                    reduce_case(rsx, x, off, cons, g, vt, op, rng, desc, eng=eng)
                for vt in (np.float32, np.float64):
                    order_case(rsx, x, off, cons, g, vt, rng, desc, eng=eng)
            eng.close()


# -- 4. consecutive-mode values that are aligned to their element only -------------------------------------------------------------------

class Outputs:
    """device outputs of one call between sentinel and guard band, refilled before every call (test_gpu_unique.run's, but reusable:
    the misaligned, many-call and capture tests hand the same pointers to several calls)"""

    def __init__(self, t, sizes, types):
        self.t, self.sizes, self.types = t, sizes, types
        self.bufs = {name: t.empty(size + GUARD, dtype=t.uint8, device="cuda") for name, size in sizes.items()}
        self.refill()

    def refill(self):
        for name, size in self.sizes.items():
            self.bufs[name][:size] = FILL
            self.bufs[name][size:] = 0xA5
        self.t.cuda.synchronize()

    def ptr(self, name):
        return self.bufs[name].data_ptr()

    def read(self):
        out = {}
        for name, size in self.sizes.items():
            b = self.bufs[name].cpu().numpy()
            assert np.all(b[size:] == 0xA5), f"{name}: guard band written"
            out[name] = b[:size].copy().view(self.types[name])
        return out


def reduce_outputs(t, n, nseg, kdtype, vt):
    return Outputs(t, {"keys": n * np.dtype(kdtype).itemsize, "run_offsets": (nseg + 1) * 8, "values": n * np.dtype(vt).itemsize, "counts": n * 4},
                   {"keys": UINT[np.dtype(kdtype)], "run_offsets": np.uint64, "values": UINT[np.dtype(vt)], "counts": np.uint32})


def unique_outputs(t, n, nseg, kdtype):
    return Outputs(t, {"keys": n * np.dtype(kdtype).itemsize, "run_offsets": (nseg + 1) * 8, "counts": n * 4, "first": n * 4, "inverse": n * 4},
                   {"keys": UINT[np.dtype(kdtype)], "run_offsets": np.uint64, "counts": np.uint32, "first": np.uint32, "inverse": np.uint32})


@pytest.mark.parametrize("vt", VTYPES, ids=lambda d: np.dtype(d).name)
def test_consecutive_values_off_16_byte_alignment(rsx, vt):
    """d_values at base + one element on whole tiles: the per-element loads instead of the 16-byte ones.  Equal bits as the aligned call,
    and the referee's."""
    t = _torch()
    rng = np.random.default_rng(VTYPES.index(vt) + 50)
    n = 3 * T + 1000
    lens = rng.choice([1, 2, 17, 300], size=n)
    x = np.repeat(rng.integers(0, 4, n), lens)[:n].astype(np.uint32)
    eng = rsx.Engine(np.uint32, n, payload=False)
    kd = dev(t, x)
    for off in (None, np.array([0, T, 3 * T], dtype=np.uint64), np.array([T, 2 * T, 2 * T, 3 * T], dtype=np.uint64)):
        nseg = 1 if off is None else len(off) - 1
        od = None if off is None else dev(t, off)
        g = flat_unique(x, off, False, True)
        for op in ("sum", "min"):
            v = make_values(vt, n, rng, op, off)
            poison = np.array([np.nan if np.dtype(vt).kind == "f" else np.iinfo(vt).min], dtype=vt)
            shifted = dev(t, np.concatenate([poison, v]))
            plain = dev(t, v)
            assert plain.data_ptr() % 16 == 0 and (shifted.data_ptr() + v.itemsize) % 16 != 0
            res = []
            for vptr in (plain.data_ptr(), shifted.data_ptr() + v.itemsize):
                out = reduce_outputs(t, n, nseg, np.uint32, vt)
                eng.segmented_reduce_by_key(kd.data_ptr(), vptr, n, None if od is None else od.data_ptr(), nseg, OPCODE[op], KIND[v.dtype],
                                            out.ptr("keys"), out.ptr("run_offsets"), out.ptr("values"), out.ptr("counts"), consecutive=True)
                eng.sync()
                res.append(out.read())
                red_check(x, v, off, res[-1], op, False, True, ref=reduce_oracle(x, v, off, op, False, True, groups=g))
            for name in res[0]:
                assert np.array_equal(res[0][name], res[1][name]), (name, op)
    eng.close()


# -- 5. one engine across entry points, shapes and calls ---------------------------------------------------------------------------------

def test_one_engine_many_calls(rsx):
    """the tables and scratch that unique and reduce-by-key share with the segmented sort and the top-k, grown, reused and left stale by
    calls of other shapes on one payload engine"""
    t = _torch()
    rng = np.random.default_rng(60)
    cap = 1 << 22
    eng = rsx.Engine(np.uint32, cap, payload=True)
    # unique at a large n
    n = cap - 4101
    off = offsets_from(list(rng.permutation(LENGTHS * 12)) + [3 * T + 5, 700 * T, 1, 0, 150 * T + 1], start=3)
    assert int(off[-1]) <= n
    x = U.run_keys(n, rng)
    unique_case(rsx, x, off, False, eng=eng)
    # reduce at a small n with many segments
    n2 = 50_000
    off2 = offsets_from(rng.integers(0, 4, 30_000), start=2)
    assert int(off2[-1]) <= n2
    x2 = rng.integers(0, 3, n2).astype(np.uint32)
    reduce_case(rsx, x2, off2, False, flat_unique(x2, off2), np.int64, "sum", rng, eng=eng)
    # the segmented sort, the top-k
    off3 = offsets_from(SORT_LENGTHS * 9, start=1)
    n3 = int(off3[-1]) + 7
    x3 = rng.integers(0, 1 << 20, n3).astype(np.uint32)
    sk, sp, _ = seg_run(rsx, x3, off3, False, payload=True, eng=eng)
    seg_check(x3, off3, sk, sp, False, payload=True)
    eng.sync()
    expect(R.fast_topk(x3, off3, 64, False), 64, *topk_on(t, eng, dev(t, x3), n3, dev(t, off3), len(off3) - 1, 64, np.uint32), "top-k")
    # unique, consecutive, at the engine's capacity
    x4 = U.run_keys(cap, rng)
    off4 = offsets_from([cap // 2 - 1, 0, 1, cap // 2 - 77], start=0)
    g4 = unique_case(rsx, x4, off4, True, eng=eng)
    order_case(rsx, x4, off4, True, g4, np.float32, rng, eng=eng)
    # reduce, sorted, at a tiny n
    x5 = rng.integers(0, 5, 37).astype(np.uint32)
    off5 = np.array([1, 1, 20, 36], dtype=np.uint64)
    g5 = flat_unique(x5, off5)
    reduce_case(rsx, x5, off5, False, g5, np.int32, "sum", rng, eng=eng)
    order_case(rsx, x5, off5, False, g5, np.float64, rng, eng=eng)
    # bad offsets: reported once, and the engine stays good
    bad = np.array([0, 100, 5000, 4000, n2], dtype=np.uint64)
    v2 = make_values(np.float32, n2, rng, "sum")
    red_run(rsx, x2, v2, bad, eng=eng)
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "segment 2 " in str(ei.value)
    eng.sync()
    g = unique_case(rsx, x, off, False, eng=eng)
    reduce_case(rsx, x, off, False, g, np.int32, "sum", rng, eng=eng)
    reduce_case(rsx, x2, off2, True, flat_unique(x2, off2, False, True), np.float32, "min", rng, eng=eng)
    eng.close()


# -- 6. capture and replay ---------------------------------------------------------------------------------------------------------------

CAPTURE_LENGTHS = [5000, 300, 70000, 4097, 1025, 20000, 1, 9000, 0, 130001, 3, 2, 4096 * 3]


def test_capture_and_replay(rsx):
    """scratch never grows inside a capture and every launch is sized from n and the segment count: one graph holding a unique call and a
    reduce call is replayed with new keys, values and offsets"""
    t = _torch()
    rng = np.random.default_rng(70)
    off = offsets_from(CAPTURE_LENGTHS, start=1)
    n, nseg = int(off[-1]) + 2, len(off) - 1
    side = t.cuda.Stream()
    eng = rsx.Engine(np.uint32, n, payload=True)
    eng.set_stream(side.cuda_stream)
    vt = np.dtype(np.float32)
    x = rng.integers(0, 40, n).astype(np.uint32)
    v = make_values(vt, n, rng, "sum", off, general=True)
    kd, vd, od = dev(t, x), dev(t, v), dev(t, off)
    uo, ro = unique_outputs(t, n, nseg, np.uint32), reduce_outputs(t, n, nseg, np.uint32, vt)

    def calls(e):
        e.segmented_unique(kd.data_ptr(), n, od.data_ptr(), nseg, uo.ptr("keys"), uo.ptr("run_offsets"), uo.ptr("counts"), uo.ptr("first"), uo.ptr("inverse"))
        e.segmented_reduce_by_key(kd.data_ptr(), vd.data_ptr(), n, od.data_ptr(), nseg, OPCODE["sum"], KIND[vt], ro.ptr("keys"), ro.ptr("run_offsets"),
                                  ro.ptr("values"), ro.ptr("counts"))

    def verify(xv, vv, ov, what):
        g = flat_unique(xv, ov)
        got = uo.read()
        uniq_check(xv, ov, got, ref=g)
        reconstructs(xv, ov, got)
        got = ro.read()
        red_check(xv, vv, ov, got, "sum", how="bound", ref=reduce_oracle(xv, vv, ov, "sum", groups=g))
        want = model_sum(vv, g["order"], g["heads"]).view(np.uint32)
        assert np.array_equal(got["values"][:want.size], want), what

    calls(eng)                                                               # eager: sizes every buffer of this (n, segment count)
    eng.sync()
    verify(x, v, off, "eager")

    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        calls(eng)
    for rep in range(2):                                                     # new keys, values and offsets in the captured buffers
        x = rng.integers(0, 40 + 1000 * rep, n).astype(np.uint32)
        lens = list(rng.permutation(CAPTURE_LENGTHS))
        lens[-1] += 1 - rep
        off = offsets_from(lens, start=rep)                                   # same segment count, ends within n
        assert len(off) - 1 == nseg and int(off[-1]) <= n
        v = make_values(vt, n, rng, "sum", off, general=True)
        kd.copy_(t.from_numpy(x.view(np.int32)))
        vd.copy_(t.from_numpy(v.view(np.int32)))
        od.copy_(t.from_numpy(off.view(np.int64)))
        uo.refill()
        ro.refill()
        graph.replay()
        t.cuda.synchronize()
        verify(x, v, off, f"replay {rep}")
    del graph

    # a fresh engine cannot size its buffers inside a capture, nor grow them after a smaller eager call: refused by name (nothing is
    # captured), and fine eagerly afterwards
    fresh = rsx.Engine(np.uint32, n, payload=True)
    fresh.set_stream(side.cuda_stream)
    small = offsets_from([100, 5000, 300])
    sx, sv = x[:5400].copy(), make_values(vt, 5400, rng, "sum", small)
    for first in (True, False):
        if not first:
            got, _ = uniq_run(rsx, sx, small, eng=fresh)
            uniq_check(sx, small, got)
            got, _ = red_run(rsx, sx, sv, small, eng=fresh)
            red_check(sx, sv, small, got)
            fresh.sync()
        for which in (0, 1):
            g2 = t.cuda.CUDAGraph()
            with t.cuda.graph(g2, stream=side):
                with pytest.raises(rsx.RadixSortError) as ei:
                    if which == 0:
                        fresh.segmented_unique(kd.data_ptr(), n, od.data_ptr(), nseg, uo.ptr("keys"), uo.ptr("run_offsets"), uo.ptr("counts"),
                                               uo.ptr("first"), uo.ptr("inverse"))
                    else:
                        fresh.segmented_reduce_by_key(kd.data_ptr(), vd.data_ptr(), n, od.data_ptr(), nseg, OPCODE["sum"], KIND[vt], ro.ptr("keys"),
                                                      ro.ptr("run_offsets"), ro.ptr("values"), ro.ptr("counts"))
            assert "capture" in str(ei.value), str(ei.value)
            del g2
    uo.refill()
    ro.refill()
    calls(fresh)
    fresh.sync()
    verify(x, v, off, "after capture")
    fresh.close()
    eng.close()


# -- 7. the written order of a float sum -------------------------------------------------------------------------------------------------

def order_layouts():
    x, off = boundary_layout()
    yield "boundaries", x, off
    yield "boundaries, one segment", x, None
    n = 1 << 22
    one = np.full(n, 0xABCD, dtype=np.uint32)
    yield "one run over 1024 tiles", one, None
    yield "1024 tiles, a few offsets", one, np.array([5, 4096 * 3, 4096 * 3 + 1, 4096 * 700 + 17, n - 4096], dtype=np.uint64)
    n, off, keys, _ = U.ragged_layout(2)
    yield "ragged, two tiles per workgroup", keys, off


def test_float_sums_in_the_written_order(rsx):
    """general float32 and float64 values: the device's bits equal the association of the header comment of rsx_reduce.hpp, which depends
    on the grouped order and the heads only.  (The any-order bound would not notice one dropped small addend in a long run.)"""
    rng = np.random.default_rng(80)
    for what, x, off in order_layouts():
        xs = x.copy()
        if off is not None and what.startswith("boundaries"):                 # sorted mode: the same runs from shuffled segments
            for s in range(len(off) - 1):
                a, b = int(off[s]), int(off[s + 1])
                xs[a:b] = rng.permutation(xs[a:b])
        eng = rsx.Engine(np.uint32, x.size, payload=True)
        for cons in (False, True):
            xv = x if cons else xs
            g = flat_unique(xv, off, False, cons)
            for vt in (np.float32, np.float64):
                order_case(rsx, xv, off, cons, g, vt, rng, eng=eng)
        eng.close()
