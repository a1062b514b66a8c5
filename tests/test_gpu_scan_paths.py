"""rsx_segmented_scan on the paths of rsx_scan_by_key.hpp and capi_scan.inc that tests/test_gpu_scan.py never reaches: off[0] beyond
tile 0 (hasc = t > t_first, the dead lanes of scan_carry_kernel, whole tiles before off[0]); R carried from one carry block of 1024 tiles
into the next by a run longer than a block; value and output pointers off 16-byte alignment, each on its own; two tiles per workgroup with
keys and with an exclusive scan; thousands of empty segments at one position, every element a restart, nothing in range at all; min / max
and a NaN through the carry level; sums at the bottom of the float range; one engine without a host wait between calls of different
kinds; a captured call replayed with off[0] in another tile.

The layouts are held in tests/_scan_ref.py (tests/test_scan.py checks that each still reaches its path, and holds the referee to what
is expected of it here).  run / check / check_float_sum, sentinels and guard bands are those of test_gpu_scan.py: integers and float
min / max are compared exactly with scan_oracle, float sums bit for bit with model_scan, the order written in rsx_scan_by_key.hpp.
"""
import numpy as np
import pytest

import _scan_ref as S
from _reduce_ref import reduce_oracle
from _scan_ref import OPS, TILE, identity, keys_of_runs, model_scan, scan_oracle
from test_gpu_float_keys import UINT
from test_gpu_reduce import check as red_check
from test_gpu_reduce import make_values as red_values
from test_gpu_reduce import run as red_run
from test_gpu_scan import CAP, KIND, OPCODE, VTYPES, check, check_float_sum, engine, make_values, ragged, run, sentinel
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, GUARD
from test_gpu_unique_reduce_paths import reduce_outputs

pytestmark = pytest.mark.gpu

DEEP = {"A": lambda: S.layout_deep(), "A-keys-u32": lambda: S.layout_deep(np.uint32), "A-keys-u64": lambda: S.layout_deep(np.uint64),
        "B": lambda: S.layout_long(), "B-deep": lambda: S.layout_long(True)}


def bits_equal_model(got, v, off=None, keys=None, excl=False, what=""):
    """the sentinel outside [off[0], off[S]); inside, model_scan's bits (check_float_sum without the any-order bound)"""
    lo, hi = (0, v.size) if off is None else (int(off[0]), int(off[-1]))
    assert np.all(np.concatenate([got[:lo], got[hi:]]) == sentinel(v.dtype)), "written outside [off[0], off[S])"
    model = model_scan(v, off, keys, excl).view(UINT[v.dtype])
    bad = np.flatnonzero(got[lo:hi] != model[lo:hi])
    assert bad.size == 0, f"{what}: bits differ from the written order at {(bad[:8] + lo).tolist()} (of {bad.size})"


# -- 1, 2. off[0] deep in the grid, a run across the carry-block edge, a run longer than a carry block -------------------------------------

@pytest.mark.parametrize("name", list(DEEP))
def test_sums_from_a_deep_start_and_across_carry_blocks(rsx, name):
    n, off, keys = DEEP[name]()
    rng = np.random.default_rng(list(DEEP).index(name) + 200)
    eng = engine(rsx, keys)
    v = make_values(np.int64, n, rng, off=off)
    for excl in (False, True):
        got, _ = run(rsx, v, off, keys, "sum", excl, eng=eng)
        check(got, v, off, keys, "sum", excl)
    for vt in (np.float32, np.float64):
        v = make_values(vt, n, rng, off=off)
        for excl in (False, True):
            got, _ = run(rsx, v, off, keys, "sum", excl, eng=eng)
            check_float_sum(got, v, off, keys, excl, what=name)
    eng.sync()


def one_sided(vt, n, rng, op, off):
    """strictly positive values for min, strictly negative ones for max: a 0 of the padding that leaked into a fold would win it.  Outside
    [off[0], off[S]): NaN, or the integer that wins."""
    vt = np.dtype(vt)
    sign = 1 if op == "min" else -1
    if vt.kind == "i":
        v = (sign * rng.integers(1, np.iinfo(vt).max, n, endpoint=True)).astype(vt)
        outside = np.iinfo(vt).min if op == "min" else np.iinfo(vt).max
    else:
        v = (sign * rng.uniform(0.5, 2.0, n)).astype(vt)
        outside = np.nan
    if off is not None:
        v[:int(off[0])] = outside
        v[int(off[-1]):] = outside
    return v


@pytest.mark.parametrize("name", ["A", "A-keys-u32", "A-keys-u64", "B-deep"])
def test_min_max_from_a_deep_start_and_across_carry_blocks(rsx, name):
    """The padding outside [off[0], off[S]) and the dead lanes of the carry level are 0, which is not the identity of min or max: what keeps
    it out is the restart at off[0].  Floats, min and max: a NaN in the second tile of the first run shows in every later output of that
    run and not in the first output after it.  On A that is 69 tiles, from wave 15 of carry block 0 into block 1; on B-deep 1094 tiles
    (one run up to off[S]: no output follows it); on the A-keys layouts the run ends at 1030 * TILE + 5, so the NaN goes through 29
    tiles only, but still from block 0 into block 1."""
    n, off, keys = DEEP[name]()
    rng = np.random.default_rng(list(DEEP).index(name) + 220)
    eng = engine(rsx, keys)
    starts, ends = S.runs_of(n, off, keys)
    lo, end, hi = int(starts[0]), int(ends[0]), int(off[-1])
    pos = (lo // TILE + 1) * TILE + 77
    assert (end - pos) // TILE >= 28
    for vt in (np.int32, np.float32, np.float64):
        for op in ("min", "max"):
            v = one_sided(vt, n, rng, op, off)
            assert np.all(v[lo:hi] > 0) if op == "min" else np.all(v[lo:hi] < 0)
            for excl in (False, True):
                got, _ = run(rsx, v, off, keys, op, excl, eng=eng)
                check(got, v, off, keys, op, excl)
            if np.dtype(vt).kind == "f":
                v[pos] = np.nan
                for excl in (False, True):
                    got, _ = run(rsx, v, off, keys, op, excl, eng=eng)
                    check(got, v, off, keys, op, excl)
                    assert S.nan_sticks(got.view(v.dtype), lo, pos, end, hi, excl), f"{op} excl={excl}: the NaN at {pos} in the run [{lo}, {end})"
    eng.sync()


# -- 3. pointers that are aligned to their element only --------------------------------------------------------------------------------------

@pytest.mark.parametrize("vt", VTYPES, ids=lambda d: np.dtype(d).name)
def test_pointers_off_16_byte_alignment(rsx, vt):
    """in_ok and out_ok of scan_tile_kernel are independent: every combination of an aligned and a misaligned input and output, and in
    place misaligned, give the bits of the aligned call on whole tiles as well; nothing is written before or after the output"""
    t = _torch()
    rng = np.random.default_rng(VTYPES.index(vt) + 240)
    n, off, _ = S.layout_misaligned()
    lo, hi = int(off[0]), int(off[-1])
    eng = engine(rsx)
    shifts = (1,) if np.dtype(vt).itemsize == 8 else (1, 3)
    v = make_values(vt, n, rng, off=off)
    for excl in (False, True):
        base, _ = run(rsx, v, off, None, "sum", excl, eng=eng)
        if np.dtype(vt).kind == "f":
            check_float_sum(base, v, off, None, excl, what="aligned")
        else:
            check(base, v, off, None, "sum", excl)
        for sh in shifts:
            for i, o in ((sh, 0), (0, sh), (sh, sh)):
                got, _ = run(rsx, v, off, None, "sum", excl, eng=eng, in_shift=i, out_shift=o)
                assert np.array_equal(got, base), f"input {i} and output {o} elements past a 16-byte boundary, excl={excl}"
            got, _ = run(rsx, v, off, None, "sum", excl, eng=eng, in_place=True, in_shift=sh)
            assert np.array_equal(got[lo:hi], base[lo:hi]), f"in place {sh} elements past a 16-byte boundary, excl={excl}"
            assert np.array_equal(got[:lo], v[:lo].view(UINT[v.dtype])) and np.array_equal(got[hi:], v[hi:].view(UINT[v.dtype]))
        # the torch helper on a misaligned view: the view is the input as it lies, the output is a fresh tensor
        whole = t.from_numpy(np.concatenate([v[:1], v])).cuda()
        view = whole[1:]
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        res = rsx.segmented_scan(view, dev(t, off), exclusive=excl)
        t.cuda.synchronize()
        res = res.cpu().numpy().view(UINT[v.dtype])
        assert np.array_equal(res[lo:hi], base[lo:hi]), f"segmented_scan(view), excl={excl}"
        assert np.array_equal(res[:lo], v[:lo].view(UINT[v.dtype])) and np.array_equal(res[hi:], v[hi:].view(UINT[v.dtype]))
        assert np.array_equal(whole.cpu().numpy().view(UINT[v.dtype]), np.concatenate([v[:1], v]).view(UINT[v.dtype])), "the input is left alone"
    eng.sync()


# -- 4. dense and degenerate offsets -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kdtype", [None, np.uint32], ids=["nokeys", "keys"])
@pytest.mark.parametrize("kind", ["mixed", "ones"])
def test_dense_offsets(rsx, kind, kdtype):
    """about one offset per element: the offsets walk of a tile takes many trips of 256, 5000 empty segments share one position mid-tile
    and 5000 share a tile edge; "ones": every element is a restart, so the exclusive result is the identity everywhere"""
    n, off, keys = S.layout_dense(kind, kdtype)
    rng = np.random.default_rng(["mixed", "ones"].index(kind) * 2 + (kdtype is not None) + 260)
    lo, hi = int(off[0]), int(off[-1])
    eng = engine(rsx, keys)
    v = make_values(np.int32, n, rng, off=off)
    for op in OPS:
        for excl in (False, True):
            got, _ = run(rsx, v, off, keys, op, excl, eng=eng)
            check(got, v, off, keys, op, excl)
            if kind == "ones" and excl:
                assert np.all(got[lo:hi].view(np.int32) == identity(np.int32, op)), op
    v = make_values(np.float64, n, rng, off=off)
    for excl in (False, True):
        got, _ = run(rsx, v, off, keys, "sum", excl, eng=eng)
        check_float_sum(got, v, off, keys, excl, what=f"dense {kind}")
    eng.sync()


@pytest.mark.parametrize("kind", ["empty", "empty_edge"])
def test_every_segment_empty(rsx, kind):
    """off[0] == off[S] inside a call with n > 0: nothing is written and nothing is reported"""
    rng = np.random.default_rng(270)
    for kdtype in (None, np.uint32):
        n, off, keys = S.layout_dense(kind, kdtype)
        eng = engine(rsx, keys)
        for vt in (np.int32, np.float64):
            v = make_values(vt, n, rng, off=off)
            for op, excl in (("sum", False), ("min", True)):
                got, _ = run(rsx, v, off, keys, op, excl, eng=eng)
                assert np.all(got == sentinel(vt)), "a call without anything in range wrote something"
        eng.sync()


# -- 5. two tiles per workgroup with keys ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offsets", [True, False], ids=["offsets", "nooffsets"])
def test_two_tiles_per_workgroup_with_keys(rsx, offsets):
    """n = 4096 * 16 * CUs + 1 (test_several_tiles_per_workgroup): the walk over the offsets handed from a workgroup's first tile to its
    second through uniq_tile_heads, runs of up to 6000 keys that cross tiles and workgroups, an exclusive scan.  (The any-order bound is
    held by model_scan in tests/test_scan.py; here the bits are model_scan's.)"""
    t = _torch()
    cus = t.cuda.get_device_properties(0).multi_processor_count
    n, off, keys = S.layout_two_tiles(cus, offsets)
    assert -(-((n + TILE - 1) // TILE) // (16 * cus)) == 2
    rng = np.random.default_rng(280 + offsets)
    eng = engine(rsx, keys)
    v = make_values(np.float32, n, rng, off=off)
    got, _ = run(rsx, v, off, keys, "sum", True, eng=eng)
    bits_equal_model(got, v, off, keys, True, what=f"{n} elements, two tiles per workgroup, exclusive")
    v = make_values(np.int32, n, rng, off=off)
    got, _ = run(rsx, v, off, keys, "min", eng=eng)
    check(got, v, off, keys, "min")
    eng.sync()


# -- 6. subnormals and signed zeros --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_sums_at_the_bottom_of_the_float_range(rsx, vt):
    """values from deep in the subnormal range to a few binades above finfo.tiny: partial sums move in and out of the subnormal range and
    round there, and the bits stay model_scan's (a flush to zero anywhere would not); a run of -0.0 sums to -0.0 at every position"""
    rng = np.random.default_rng(290 + (vt is np.float64))
    tiny = np.finfo(vt).tiny
    minus = np.array([-0.0], dtype=vt).view(UINT[np.dtype(vt)])[0]
    n, off, keys = ragged(rng, np.uint32)
    for n, off, keys in ((n, off, keys), (n, off, None), (70 * TILE, None, None)):
        eng = engine(rsx, keys)
        v = S.tiny_values(vt, n, rng)
        assert np.any((v != 0) & (np.abs(v) < tiny)) and np.any(np.abs(v) >= tiny)
        if off is not None:
            v[:int(off[0])] = np.nan
            v[int(off[-1]):] = np.nan
        for excl in (False, True):
            got, _ = run(rsx, v, off, keys, "sum", excl, eng=eng)
            bits_equal_model(got, v, off, keys, excl, what=f"tiny values, {n} elements")
        if keys is None:
            a, b = (0, n) if off is None else (int(off[12]), int(off[13]))         # the segment of 9000 elements, or everything
            assert b - a >= 9000
            v[a:b] = -0.0
            got, _ = run(rsx, v, off, None, "sum", eng=eng)
            bits_equal_model(got, v, off, None, what="a run of -0.0")
            assert np.all(got[a:b] == minus), "a run of -0.0 does not sum to -0.0 everywhere"
            assert np.all(scan_oracle(v, off).astype(vt)[a:b].view(UINT[np.dtype(vt)]) == minus)
        eng.sync()


# -- 7. one engine, one host wait ------------------------------------------------------------------------------------------------------------------

class Scan:
    """one scan call with its buffers on the device, so that several can be enqueued back to back and read afterwards"""

    def __init__(self, t, v, off=None, keys=None, op="sum", excl=False):
        self.v, self.off, self.keys, self.op, self.excl = v, off, keys, op, excl
        self.nbytes = v.size * v.dtype.itemsize
        self.v_in = dev(t, v)
        self.k_in = None if keys is None else dev(t, keys)
        self.o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
        self.out = dev(t, np.concatenate([np.full(self.nbytes, FILL, dtype=np.uint8), np.full(GUARD, 0xA5, dtype=np.uint8)]))

    def enqueue(self, eng):
        eng.segmented_scan(None if self.k_in is None else self.k_in.data_ptr(), self.v_in.data_ptr(), self.v.size,
                           None if self.o is None else self.o.data_ptr(), 1 if self.off is None else len(self.off) - 1, OPCODE[self.op],
                           KIND[self.v.dtype], self.out.data_ptr(), exclusive=self.excl)

    def read(self):
        b = self.out.cpu().numpy().view(np.uint8)
        assert np.all(b[self.nbytes:] == 0xA5), "guard band written"
        return b[:self.nbytes].copy().view(UINT[self.v.dtype])

    def fresh(self, rsx):
        return run(rsx, self.v, self.off, self.keys, self.op, self.excl)[0]


def test_one_engine_many_kinds_one_wait(rsx):
    """The scan reinterprets the 8-byte slots of the per-tile partials it shares with rsx_segmented_reduce_by_key per value kind, and
    growing them waits for and frees what pending calls use.  Five calls of different sizes, kinds and entry points on one engine and one
    stream, without a host wait between them: each output has the bits that the same call gives on an engine of its own."""
    t = _torch()
    rng = np.random.default_rng(300)
    na, offa, _ = S.layout_deep()
    nr, offr, keysr = ragged(rng, np.uint32)
    scans = [Scan(t, make_values(np.int32, 100, rng)),
             Scan(t, make_values(np.float64, na, rng, off=offa), offa),                                 # grows the partials
             None,
             Scan(t, make_values(np.float32, nr, rng, off=offr), offr, keysr, excl=True),
             Scan(t, make_values(np.int64, 100, rng), op="max")]
    x = rng.integers(0, 3, 3000).astype(np.uint32)
    xv = red_values(np.float32, 3000, rng, "sum", general=True)
    xd, xvd = dev(t, x), dev(t, xv)
    ro = reduce_outputs(t, 3000, 1, np.uint32, np.float32)
    eng = rsx.Engine(np.uint32, CAP, payload=True)
    t.cuda.synchronize()                                                         # every upload has landed; from here on nothing waits
    for s in scans:
        if s is not None:
            s.enqueue(eng)
        else:
            eng.segmented_reduce_by_key(xd.data_ptr(), xvd.data_ptr(), 3000, None, 1, OPCODE["sum"], KIND[xv.dtype], ro.ptr("keys"),
                                        ro.ptr("run_offsets"), ro.ptr("values"), ro.ptr("counts"))
    eng.sync()
    for i, s in enumerate(scans):
        if s is not None:
            assert np.array_equal(s.read(), s.fresh(rsx)), f"call {i} ({s.v.dtype.name} {s.op}, {s.v.size} elements)"
    got = ro.read()
    alone, _ = red_run(rsx, x, xv, None, "sum")
    red_check(x, xv, None, got, "sum", how="bound", ref=reduce_oracle(x, xv, None, "sum"))
    for name in got:
        assert np.array_equal(got[name], alone[name]), f"the reduce between the scans: {name}"
    eng.close()


# -- 8. replay with off[0] in another tile -----------------------------------------------------------------------------------------------------

def test_replay_with_a_moving_first_offset(rsx):
    """the launches are fixed at capture, so the first tile in range must be found on the device at every replay: one captured call is
    replayed with off[0] = 0, with off[0] in tile 37 and with every segment empty (the same segment count throughout)"""
    t = _torch()
    rng = np.random.default_rng(310)
    T = TILE
    n = 80 * T
    layouts = [np.array([0, 5000, 5000, 30 * T + 7, 60 * T, 70 * T + 1, n - 3], dtype=np.uint64),
               np.array([37 * T + 5, 37 * T + 5, 40 * T, 55 * T + 9, 55 * T + 10, 79 * T, n], dtype=np.uint64),
               np.full(7, 41 * T + 100, dtype=np.uint64)]
    off = np.array([9, 100, 20 * T, 20 * T, 50 * T + 1, 66 * T, n - 1], dtype=np.uint64)
    nseg = len(off) - 1
    side = t.cuda.Stream()
    keys = keys_of_runs(n, rng, np.uint32)
    eng = engine(rsx, keys, stream=side.cuda_stream)
    v = make_values(np.float32, n, rng, off=off)
    kd, vd, od = dev(t, keys), dev(t, v), dev(t, off)
    out = dev(t, np.full(n * 4, FILL, dtype=np.uint8))

    def call():
        eng.segmented_scan(kd.data_ptr(), vd.data_ptr(), n, od.data_ptr(), nseg, OPCODE["sum"], KIND[v.dtype], out.data_ptr())

    call()                                                                   # eager: sizes the scratch of this n
    eng.sync()
    check_float_sum(out.cpu().numpy().view(np.uint32), v, off, keys, what="eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for rep, off in enumerate(layouts):
        assert len(off) - 1 == nseg
        keys = keys_of_runs(n, rng, np.uint32)
        v = make_values(np.float32, n, rng, off=off)
        kd.copy_(t.from_numpy(keys.view(np.int32)))
        vd.copy_(t.from_numpy(v.view(np.int32)))
        od.copy_(t.from_numpy(off.view(np.int64)))
        out.fill_(FILL - 256)
        graph.replay()
        t.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        if rep == 2:
            assert np.all(got == sentinel(np.float32)), "a replay without anything in range wrote something"
        else:
            eager, _ = run(rsx, v, off, keys)
            assert np.array_equal(got, eager), f"replay {rep} (off[0] = {int(off[0])}) differs from the eager call"
            check_float_sum(got, v, off, keys, what=f"replay {rep}")
    del graph
    eng.sync()
