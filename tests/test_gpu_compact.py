"""Stream compaction (rsx_segmented_compact, radix_sort_amd.segmented_compact / masked_select / nonzero / compact_rows) on the GPU.

The referee is tests/_compact_ref.py; every comparison is exact equality of bits with compact_oracle: the call moves bits, there is no
tolerance anywhere.  Every output starts out holding the family's sentinel, which must survive wherever the referee says nothing is
written, and ends in a guard band.  Keys and mask bytes outside [off[0], off[S]) are random, so that reading one changes an answer.
Every engine here has capacity 4096: the call is not bound by it.  The layouts come from _compact_ref, where tests/test_compact.py
checks from the layout alone that each reaches the path it is named after.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import _compact_ref as R
from _compact_ref import compact_oracle, keep_flags
from _search_ref import UINT
from test_compact import drawn_bounds, flag_combinations
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, FILL32, FILL64, GUARD
from test_search import HEADER_DTYPES as DTYPES
from test_search import random_keys

pytestmark = pytest.mark.gpu

CAP = 4096
GUARD_BYTE = 0xA5


def filled(t, nbytes):
    return dev(t, np.concatenate([np.full(nbytes, FILL, dtype=np.uint8), np.full(GUARD, GUARD_BYTE, dtype=np.uint8)]))


def run(rsx, keys, off, mask=None, bounds=None, partition=False, invert=False, strict=False, descending=False, eng=None, want=("keys", "index"),
        key_shift=0, index_shift=0, mask_shift=0):
    """One rsx_segmented_compact through the Engine API.  Every output is pre-filled with the sentinel and followed by a guard band; the key
    and index outputs start key_shift / index_shift elements into their buffers and the mask mask_shift bytes into its own (the bytes
    before must survive).  Returns ({name: host array of the whole output}, engine)."""
    t = _torch()
    n, ks = keys.size, keys.dtype.itemsize
    nseg = 1 if off is None else len(off) - 1
    k = dev(t, keys)
    o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
    m = None if mask is None else dev(t, np.concatenate([np.full(mask_shift, 1, dtype=np.uint8), np.asarray(mask).view(np.uint8)]))
    b = None if bounds is None else dev(t, np.asarray(bounds, dtype=keys.dtype))
    kout = filled(t, (n + key_shift) * ks) if "keys" in want else None
    iout = filled(t, (n + index_shift) * 4) if "index" in want else None
    koff = filled(t, (nseg + 1) * 8)
    if eng is None:
        eng = rsx.Engine(keys.dtype, CAP, descending=descending)
    eng.segmented_compact(k.data_ptr(), n, None if o is None else o.data_ptr(), nseg, None if m is None else m.data_ptr() + mask_shift,
                          None if b is None else b.data_ptr(), None if kout is None else kout.data_ptr() + key_shift * ks,
                          None if iout is None else iout.data_ptr() + index_shift * 4, koff.data_ptr(), partition=partition, invert=invert, strict=strict)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    got = {}
    for name, buf, shift, size in (("keys", kout, key_shift, ks), ("index", iout, index_shift, 4), ("koff", koff, 0, 8)):
        if buf is None:
            continue
        raw = buf.cpu().numpy().view(np.uint8)
        assert np.all(raw[-GUARD:] == GUARD_BYTE), f"{name}: guard band written"
        assert np.all(raw[:shift * size] == FILL), f"{name}: bytes before the output written"
        got[name] = raw[shift * size:-GUARD].copy().view({4: np.uint32, 8: np.uint64}[size])
    return got, eng


def check(got, ref, what=""):
    """exact equality with the referee where it writes, the sentinel everywhere else"""
    rk, ri, rkoff, written = ref
    u = UINT[rk.dtype.itemsize]
    assert np.array_equal(got["koff"].astype(np.int64), rkoff), f"{what}: kept offsets differ: {got['koff'][:8].tolist()} != {rkoff[:8].tolist()}"
    for name, want in (("keys", np.where(written, rk.view(u), u(FILL64 & ((1 << (8 * rk.dtype.itemsize)) - 1)))),
                       ("index", np.where(written, ri, FILL32).astype(np.uint32))):
        if name in got:
            bad = np.flatnonzero(got[name] != want)
            assert bad.size == 0, f"{what}: {name} differ at {bad[:8].tolist()} (of {bad.size}): {got[name][bad[:8]].tolist()} != {want[bad[:8]].tolist()}"


def run_check(rsx, keys, off, what="", **kw):
    got, eng = run(rsx, keys, off, **kw)
    ref_kw = {k: v for k, v in kw.items() if k in ("mask", "bounds", "partition", "invert", "strict", "descending")}
    check(got, compact_oracle(keys, off, **ref_kw), what)
    return got, eng


def random_mask(n, rng):
    return R.MASK_BYTES[rng.integers(0, R.MASK_BYTES.size, n)]


def ragged_keys(dt, rng):
    """the ragged layout: every other segment from a narrow range (ties with the bound), random keys outside the segments"""
    n, off = R.ragged_layout()
    keys = random_keys(dt, n, rng)
    for s, L in enumerate(R.LENGTHS):
        if s % 2 == 1:
            keys[int(off[s]):int(off[s]) + L] = random_keys(dt, L, rng, narrow=True)
    return keys, off


# -- 1. the ragged layout: six dtypes x {mask, bound} x every flag combination ------------------------------------------------------------

@pytest.mark.parametrize("form", ["mask", "bound"])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_ragged_matrix(rsx, dt, form):
    rng = np.random.default_rng(100 + DTYPES.index(dt) * 2 + (form == "bound"))
    keys, off = ragged_keys(dt, rng)
    for descending in ((False,) if form == "mask" else (False, True)):
        eng = rsx.Engine(dt, CAP, descending=descending)
        args = dict(mask=random_mask(keys.size, rng)) if form == "mask" else dict(bounds=drawn_bounds(keys, off, rng))
        if form == "bound":                                                      # ties with the bound occur
            assert np.any(keep_flags(keys, off, descending=descending, **args) != keep_flags(keys, off, descending=descending, strict=True, **args))
        for kw in flag_combinations(form == "bound"):
            run_check(rsx, keys, off, f"{form} {kw} descending={descending}", eng=eng, descending=descending, **args, **kw)
        eng.sync()


# -- 2. mask patterns on one segment of 3 x 4096 + 17 elements ---------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_mask_patterns(rsx, pattern):
    rng = np.random.default_rng(R.PATTERNS.index(pattern))
    mask = R.pattern_mask(pattern, rng)
    for dt in (np.uint32, np.uint64):
        keys = random_keys(dt, R.PATTERN_N, rng)
        eng = rsx.Engine(dt, CAP)
        for kw in flag_combinations(False):
            run_check(rsx, keys, None, f"{pattern} {kw}", eng=eng, mask=mask, **kw)
        eng.sync()


# -- 3. output selection ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("want", [("keys",), ("index",), ()], ids=["keys_only", "index_only", "count_only"])
def test_output_selection(rsx, want):
    rng = np.random.default_rng(300 + len(want))
    keys, off = ragged_keys(np.int64, rng)
    eng = rsx.Engine(np.int64, CAP)
    for partition in (False, True):
        got, _ = run_check(rsx, keys, off, f"mask {want}", eng=eng, mask=random_mask(keys.size, rng), partition=partition, want=want)
        assert set(got) == set(want) | {"koff"}
        run_check(rsx, keys, off, f"bound {want}", eng=eng, bounds=drawn_bounds(keys, off, rng), partition=partition, want=want)
    eng.sync()


# -- 4. paths ---------------------------------------------------------------------------------------------------------------------------------

def test_large_run_two_tiles_per_workgroup_and_scan_block_edge(rsx):
    """2^24 + 4096 + 5 uint32: on 256 CUs a workgroup walks two tiles, the tile table crosses the block edge of scan_blocks_kernel, and
    segment 1 starts inside the second tile of workgroup 0: once mask form compact, once bound form partition"""
    rng = np.random.default_rng(400)
    n, off = R.big_layout()
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    eng = rsx.Engine(np.uint32, CAP)
    mask = np.where(rng.integers(0, 3, n) == 0, np.uint8(0), random_mask(n, rng)).astype(np.uint8)
    run_check(rsx, keys, off, "large, mask, compact", eng=eng, mask=mask)
    bounds = np.array([1 << 31, 3 << 30], dtype=np.uint32)
    run_check(rsx, keys, off, "large, bound, partition", eng=eng, bounds=bounds, partition=True)
    eng.sync()


@pytest.mark.parametrize("layout", ["empties", "mid_tile", "nothing"])
def test_path_layouts(rsx, layout):
    rng = np.random.default_rng(410)
    n, off = getattr(R, layout + "_layout")()
    for dt in (np.uint32, np.float64):
        keys = random_keys(dt, n, rng, narrow=True)
        eng = rsx.Engine(dt, CAP, descending=dt is np.float64)
        mask, bounds = random_mask(n, rng), drawn_bounds(keys, off, rng)
        for kw in flag_combinations(False):
            run_check(rsx, keys, off, f"{layout} mask {kw}", eng=eng, mask=mask, **kw)
        for kw in flag_combinations(True):
            got, _ = run_check(rsx, keys, off, f"{layout} bound {kw}", eng=eng, bounds=bounds, descending=dt is np.float64, **kw)
        if layout == "nothing":
            assert np.all(got["koff"] == 0) and np.all(got["keys"] == got["keys"][0])
        eng.sync()


# -- 5. alignment --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [np.uint32, np.uint64], ids=lambda d: np.dtype(d).name)
def test_alignment(rsx, dt):
    rng = np.random.default_rng(500)
    keys, off = ragged_keys(dt, rng)
    eng = rsx.Engine(dt, CAP)
    mask = random_mask(keys.size, rng)
    for (ksh, ish), msh in zip(itertools.product((1, 2, 3), (3, 1, 2)), itertools.cycle((1, 3, 7, 15))):
        for partition in (False, True):
            run_check(rsx, keys, off, f"shifts {ksh} {ish} {msh}", eng=eng, mask=mask, partition=partition, key_shift=ksh, index_shift=ish, mask_shift=msh)
    # one segment over whole tiles: the misaligned mask takes the byte loads in every tile
    k1 = random_keys(dt, 2 * R.TILE, rng)
    for msh in (1, 3, 7, 15):
        run_check(rsx, k1, None, f"mask shift {msh}", eng=eng, mask=random_mask(k1.size, rng), mask_shift=msh)
    eng.sync()


# -- 6. refusals -------------------------------------------------------------------------------------------------------------------------------

def test_refusals(rsx):
    t = _torch()
    n = 1 << 12
    eng = rsx.Engine(np.uint32, n)
    x = t.zeros(n + 4, dtype=t.int32, device="cuda")
    eng.sort_from(x.data_ptr(), n)                                               # the engine's result buffer is then one of its own
    eng.sync()
    assert eng.result_device()[0] != 0
    kout, iout = (t.full((n,), -7, dtype=t.int32, device="cuda") for _ in range(2))
    mask = t.ones(n + 64, dtype=t.uint8, device="cuda")
    bounds = t.zeros(2, dtype=t.int32, device="cuda")
    off = t.tensor([0, n], dtype=t.int64, device="cuda")
    koff = t.full((2,), -7, dtype=t.int64, device="cuda")
    base = dict(d_keys=x.data_ptr(), n=n, d_offsets=off.data_ptr(), num_segments=1, d_mask=mask.data_ptr(), d_bounds=None, d_keys_out=kout.data_ptr(),
                d_index_out=iout.data_ptr(), d_kept_offsets_out=koff.data_ptr())
    ok = lambda **kw: eng.segmented_compact(**{**base, **kw})
    refused = [
        (4, dict(d_bounds=bounds.data_ptr())),                                   # both mask and bounds
        (4, dict(d_mask=None)),                                                  # neither
        (4, dict(strict=True)),                                                  # STRICT with a mask
        (4, dict(n=(1 << 31) + 1)),                                              # beyond 2^31 (pointers only: nothing is launched)
        (1, dict(d_keys=x.data_ptr() + 4)),                                      # misaligned keys
        (1, dict(d_keys=None)),
        (1, dict(d_kept_offsets_out=None)),                                      # the required output
        (1, dict(d_kept_offsets_out=koff.data_ptr() + 4)),                       # misaligned kept offsets, index, bounds
        (1, dict(d_index_out=iout.data_ptr() + 2)),
        (1, dict(d_mask=None, d_bounds=bounds.data_ptr() + 2)),
        (1, dict(d_keys_out=x.data_ptr())),                                      # each overlap: an output on the keys,
        (1, dict(d_index_out=x.data_ptr() + 16)),
        (1, dict(d_keys_out=mask.data_ptr())),                                   # on the mask,
        (1, dict(d_mask=None, d_bounds=bounds.data_ptr(), d_index_out=bounds.data_ptr())),       # on the bounds,
        (1, dict(d_kept_offsets_out=off.data_ptr())),                            # on the offsets,
        (1, dict(d_index_out=kout.data_ptr())),                                  # two outputs,
        (1, dict(d_index_out=kout.data_ptr() + 4 * (n - 1))),
        (1, dict(d_kept_offsets_out=iout.data_ptr() + 8)),
        (1, dict(d_keys_out=eng.result_device()[0])),                            # the engine's own buffers
        (1, dict(d_keys=eng.result_device()[0])),
    ]
    for status, kw in refused:
        with pytest.raises(rsx.RadixSortError) as ei:
            ok(**kw)
        assert ei.value.status == status and "rsx_segmented_compact" in str(ei.value), kw
    lib = rsx.load_library()
    P = C.c_void_p
    for flags in (1, 2, 4, 7, 64, 1 << 31):                                      # unknown flag bits: the family's bits 0 - 2 included
        assert lib.rsx_segmented_compact(eng._h, P(x.data_ptr()), n, P(off.data_ptr()), 1, P(mask.data_ptr()), None, flags, P(kout.data_ptr()),
                                         P(iout.data_ptr()), P(koff.data_ptr())) == 4
        assert b"rsx_segmented_compact" in lib.rsx_last_error()
    # n == 0 and no segments: nothing is launched, nothing is written — the kept offsets included
    ok(n=0)
    ok(num_segments=0)
    ok(n=0, d_offsets=None)
    eng.sync()
    for buf in (kout, iout, koff):
        assert bool((buf == -7).all()), "a refused call wrote something"
    ok()                                                                         # and the call these were variations of works
    eng.sync()
    assert koff.tolist() == [0, n] and iout.tolist() == list(range(n))


# -- 7. bad offsets ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("partition", [False, True], ids=["compact", "partition"])
@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_reported_once(rsx, bad, partition):
    rng = np.random.default_rng(23)
    n = 40000
    x = rng.integers(0, 99, n).astype(np.uint32)
    off = np.array([0, 100, 5000, 4000 if bad == "decreasing" else n + 1, n], dtype=np.uint64)       # segment 2 is the first bad one
    eng = rsx.Engine(np.uint32, CAP)
    for args in (dict(mask=random_mask(n, rng)), dict(bounds=np.array([50, 10, 98, 0], dtype=np.uint32))):
        got, _ = run(rsx, x, off, eng=eng, partition=partition, **args)          # guard bands checked inside
        with pytest.raises(rsx.RadixSortError) as ei:
            eng.sync()
        assert ei.value.status == 4 and "segment 2 " in str(ei.value)
        eng.sync()                                                               # reported once
        assert np.all(got["koff"] == 0) and np.all(got["keys"] == FILL32) and np.all(got["index"] == FILL32)
        # the engine stays usable: a correct call right after gives correct results
        good = np.array([0, 3, 5000, 5001, n], dtype=np.uint64)
        run_check(rsx, x, good, "after bad offsets", eng=eng, partition=partition, **args)
        eng.sync()


# -- 8. call state -----------------------------------------------------------------------------------------------------------------------------

def test_sort_state_is_untouched_and_n_exceeds_capacity(rsx):
    t = _torch()
    rng = np.random.default_rng(61)
    eng = rsx.Engine(np.uint32, CAP)
    x = rng.integers(0, 1 << 32, CAP, dtype=np.uint32)
    xd = dev(t, x)
    eng.sort_from(xd.data_ptr(), CAP)
    n = 20000
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    off = np.array([7, 5000, 5000, 19990], dtype=np.uint64)
    run_check(rsx, keys, off, "on an engine that holds a sort's result", eng=eng, mask=random_mask(n, rng))
    run_check(rsx, keys, off, "the same, bound form, partition", eng=eng, bounds=keys[[100, 0, 6000]], partition=True)
    assert eng.geometry().num_keys == CAP
    out = t.zeros(CAP, dtype=t.int32, device="cuda")
    t.cuda.synchronize()                                                         # (the engine copies on its own stream)
    eng.copy_result(out.data_ptr())
    eng.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.sort(x))


def test_two_engines_two_streams_identical_bits(rsx):
    t = _torch()
    rng = np.random.default_rng(62)
    keys, off = ragged_keys(np.float32, rng)
    mask = random_mask(keys.size, rng)
    res = []
    streams = [t.cuda.Stream(), t.cuda.Stream()]
    for s in streams:
        eng = rsx.Engine(np.float32, CAP, descending=True)
        eng.set_stream(s.cuda_stream)
        a, _ = run(rsx, keys, off, eng=eng, mask=mask, partition=True)
        b, _ = run(rsx, keys, off, eng=eng, bounds=drawn_bounds(keys, off, np.random.default_rng(5)), descending=True)
        eng.sync()
        res.append((a, b))
    for x, y in zip(res[0], res[1]):
        for name in x:
            assert np.array_equal(x[name], y[name]), name


def test_capture_and_replay(rsx):
    """every launch is sized from n and the segment count: one captured call (a linear chain) is replayed after the mask's contents and
    off[0] have changed"""
    t = _torch()
    rng = np.random.default_rng(70)
    dt = np.int32
    keys, off = ragged_keys(dt, rng)
    n, nseg = keys.size, len(off) - 1
    side = t.cuda.Stream()
    eng = rsx.Engine(dt, CAP)
    eng.set_stream(side.cuda_stream)
    mask = random_mask(n, rng)
    kd, od, md = dev(t, keys), dev(t, off), dev(t, mask)
    kout, iout, koff = (dev(t, np.full(nb, FILL, dtype=np.uint8)) for nb in (4 * n, 4 * n, 8 * (nseg + 1)))

    def call():
        eng.segmented_compact(kd.data_ptr(), n, od.data_ptr(), nseg, md.data_ptr(), None, kout.data_ptr(), iout.data_ptr(), koff.data_ptr())

    def result():
        return {"keys": kout.cpu().numpy().view(np.uint32), "index": iout.cpu().numpy().view(np.uint32), "koff": koff.cpu().numpy().view(np.uint64)}

    call()                                                                       # eager: the first call of an engine allocates its scratch
    eng.sync()
    check(result(), compact_oracle(keys, off, mask=mask), "eager")
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        call()
    for rep in range(2):
        mask = random_mask(n, rng)
        off = off.copy()
        off[0] = rep                                                             # segment 0 is empty in the layout: off[0] may move below off[1]
        md.copy_(t.from_numpy(mask.view(np.int8)))
        od.copy_(t.from_numpy(off.view(np.int64)))
        for buf in (kout, iout, koff):
            buf.fill_(FILL - 256)
        graph.replay()
        t.cuda.synchronize()
        check(result(), compact_oracle(keys, off, mask=mask), f"replay {rep}")
    del graph
    eng.sync()


# -- 9. the family: bounds from segmented_select ---------------------------------------------------------------------------------------------

def test_bounds_from_select_keep_the_top_50(rsx):
    t = _torch()
    rng = np.random.default_rng(90)
    rows, cols, rank = 64, 5000, 49
    x = (rng.integers(-300, 300, (rows, cols)) / 4.0).astype(np.float32)          # ties at the 50th value occur
    xd = t.from_numpy(x).cuda()
    offsets = t.arange(0, rows + 1, device="cuda", dtype=t.int64) * cols
    bounds = rsx.segmented_select(xd.reshape(-1), offsets, t.full((rows,), rank, dtype=t.int64, device="cuda"), descending=True)[0].reshape(-1).contiguous()
    assert bounds.numel() == rows
    srt = rsx.sort_rows(xd, descending=True)[0].cpu().numpy()
    ties = 0
    for strict in (False, True):
        vals, koff, idx = rsx.segmented_compact(xd.reshape(-1), offsets, bound=bounds, descending=True, strict=strict, return_index=True)
        vals, koff, idx = vals.cpu().numpy(), koff.cpu().numpy(), idx.cpu().numpy()
        for r in range(rows):
            got = vals[koff[r]:koff[r + 1]]
            b = srt[r, rank]
            want = srt[r][srt[r] > b] if strict else srt[r][srt[r] >= b]
            assert strict or got.size >= rank + 1
            assert np.array_equal(np.sort(got.view(np.uint32)), np.sort(want.view(np.uint32))), (r, strict)
            assert np.array_equal(x[r, idx[koff[r]:koff[r + 1]]].view(np.uint32), got.view(np.uint32))
            ties += int(not strict and got.size > rank + 1)
    assert ties > 0


# -- 10. the torch helpers ---------------------------------------------------------------------------------------------------------------------

def test_masked_select_and_nonzero_equal_torch(rsx):
    t = _torch()
    g = t.Generator().manual_seed(11)
    bits = lambda a: a.contiguous().view(t.int32 if a.element_size() == 4 else t.int64)
    for dt in (t.int32, t.int64, t.float32):
        for shape in [(0,), (1,), (5000,), (37, 211), (4, 5, 1000), (1 << 20,)]:
            x = t.randint(-3, 4, shape, generator=g).to(dt).cuda()
            if dt.is_floating_point and x.numel() > 8:
                flat = x.reshape(-1)
                flat[1], flat[3], flat[5] = float("nan"), -0.0, float("inf")
            mask = (t.rand(shape, generator=g) < 0.4).cuda()
            got, want = rsx.masked_select(x, mask), t.masked_select(x, mask)
            assert got.dtype == want.dtype and got.shape == want.shape and t.equal(bits(got), bits(want)), (dt, shape)
            assert t.equal(bits(rsx.masked_select(x, mask.to(t.uint8) * 255)), bits(want))
            nz, want_nz = rsx.nonzero(x), t.nonzero(x)
            assert nz.dtype == t.int64 and nz.shape == want_nz.shape and t.equal(nz, want_nz), (dt, shape)
            for a, b in zip(rsx.nonzero(x, as_tuple=True), t.nonzero(x, as_tuple=True)):
                assert t.equal(a, b)
    # a 3-D non-contiguous input and a broadcast mask
    x = t.randn((6, 50, 70), generator=g).cuda().transpose(0, 2)[:, 1:, :]
    mask = (t.rand((49, 1), generator=g) < 0.5).cuda()
    assert not x.is_contiguous()
    assert t.equal(bits(rsx.masked_select(x, mask)), bits(t.masked_select(x, mask)))
    assert t.equal(rsx.nonzero(x > 0.5), t.nonzero(x > 0.5))


def test_compact_rows_and_partition_helper(rsx):
    t = _torch()
    g = t.Generator().manual_seed(12)
    x = t.randint(-50, 50, (33, 4100), generator=g).to(t.int32).cuda()
    mask = (t.rand((33, 4100), generator=g) < 0.3).cuda()
    vals, ro, idx = rsx.compact_rows(x, mask=mask, return_index=True)
    assert ro.dtype == t.int64 and idx.dtype == t.int64 and ro.numel() == 34
    for r in range(33):
        a, b = int(ro[r]), int(ro[r + 1])
        assert t.equal(vals[a:b], x[r][mask[r]]) and t.equal(idx[a:b], t.nonzero(mask[r]).reshape(-1))
    bound = t.randint(-50, 50, (33,), generator=g).to(t.int32).cuda()
    for descending, strict in itertools.product((False, True), (False, True)):
        vals, ro = rsx.compact_rows(x, bound=bound, descending=descending, strict=strict)
        for r in range(33):
            keep = (x[r] > bound[r] if strict else x[r] >= bound[r]) if descending else (x[r] < bound[r] if strict else x[r] <= bound[r])
            assert t.equal(vals[int(ro[r]):int(ro[r + 1])], x[r][keep])
    # partition=True with the index: keys[off[s] + index] == out per segment; outside the segments the input's keys
    keys = x.reshape(-1)[:100000].contiguous()
    off = t.tensor([5, 5, 4101, 9000, 9000, 70001, 99990], dtype=t.int64, device="cuda")
    m = mask.reshape(-1)[:100000].contiguous()
    out, ko, index = rsx.segmented_compact(keys, off, mask=m, partition=True, return_index=True)
    assert out.shape == keys.shape and index.dtype == t.int64
    for s in range(off.numel() - 1):
        a, b = int(off[s]), int(off[s + 1])
        assert t.equal(keys[a + index[a:b]], out[a:b])
        split = int(ko[s + 1] - ko[s])
        assert split == int(m[a:b].sum()) and t.equal(out[a:a + split], keys[a:b][m[a:b]]) and t.equal(out[a + split:b], keys[a:b][~m[a:b]])
    assert t.equal(out[:5], keys[:5]) and t.equal(out[99990:], keys[99990:])
