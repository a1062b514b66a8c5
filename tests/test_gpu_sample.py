"""The categorical draw (rsx_segmented_sample, radix_sort_amd.segmented_sample, multinomial and sample_rows) on the GPU.

The referee is tests/_sample_ref.py; every comparison is exact integer equality with it: there is no tolerance anywhere.  The harness is
tests/test_gpu_whistogram.py's: engines of capacity 4096 (the call is not bound by it), the outputs pre-filled with the family's sentinel
— a slot without an answer must still hold it — and followed by guard bands, a few bytes in front of them so that they start aligned to
their element only, and random keys and weights outside [off[0], off[S]), so that reading one changes a total.  The layouts come from
_sample_ref, where tests/test_sample.py checks from the layout alone that each reaches the path it is named for.
Every engine a test creates is closed by the test: an engine left to the garbage collector (a pytest.raises block keeps its frame in a
reference cycle) would be freed at an arbitrary later moment, possibly inside another test's stream capture.
"""
import numpy as np
import pytest

import _compact_ref as C
import _sample_ref as R
import _whistogram_ref as W
from _wselect_ref import kind_of, random_targets
from test_gpu_segmented import _torch, dev
from test_gpu_unique import FILL, FILL32, FILL64, GUARD
from test_gpu_wselect import run as wselect_run

pytestmark = pytest.mark.gpu

CAP = 4096
GUARD_BYTE = 0xA5
KEY_DTYPES = ["uint32", "int32", "uint64", "int64", "float32", "float64"]


def _band(t, nbytes, front):
    buf = dev(t, np.concatenate([np.full(front + nbytes, FILL, dtype=np.uint8), np.full(GUARD, GUARD_BYTE, dtype=np.uint8)]))
    assert buf.data_ptr() % 16 == 0
    return buf


def _unband(buf, nbytes, front, what):
    raw = buf.cpu().numpy().view(np.uint8)
    assert np.all(raw[-GUARD:] == GUARD_BYTE), f"guard band behind the {what} written"
    assert np.all(raw[:front] == FILL), f"bytes before the {what} written"
    return raw[front:front + nbytes].copy()


class Inputs:
    """the device copies of one upload: keys (or None), weights (or None: the keys are the weights) with a skew, offsets"""

    def __init__(self, weights, off, keys=None, skew=0):
        t = _torch()
        self.weights, self.keys, self.off = weights, keys, off
        self.n = (keys if weights is None else weights).size
        self.nseg = 1 if off is None else len(off) - 1
        self.k = None if keys is None else dev(t, keys)
        self.wptr = None
        if weights is not None:
            self.w = dev(t, np.concatenate([np.zeros(skew, dtype=weights.dtype), weights, np.zeros(1, dtype=weights.dtype)]))
            assert self.w.data_ptr() % 16 == 0
            self.wptr = self.w.data_ptr() + skew * weights.dtype.itemsize
        self.o = None if off is None else dev(t, np.asarray(off, dtype=np.uint64))
        self.kind = kind_of(keys if weights is None else weights)


def run(rsx, eng, inp, targets, bounds=None, fraction=False, strict=False, invert=False, weight_exp=0, want_mass=True, want_total=True, pass_keys=None):
    """One rsx_segmented_sample through the Engine API.  Returns (index [S, R] uint32, mass [S, R] uint64 or None, total [S] uint64 or
    None).  The keys' pointer is passed only where the call reads it (pass_keys overrides)."""
    t = _torch()
    nseg = inp.nseg
    tt = np.ascontiguousarray(np.asarray(targets, dtype=np.float64 if fraction else np.uint64).reshape(nseg, -1))
    Rr = tt.shape[1]
    t_in = dev(t, tt)
    b_in = None if bounds is None else dev(t, np.ascontiguousarray(bounds))
    reads_keys = bounds is not None or inp.weights is None
    if pass_keys is None:
        pass_keys = reads_keys
    i_buf, m_buf, s_buf = _band(t, nseg * Rr * 4, 4), _band(t, nseg * Rr * 8, 8), _band(t, nseg * 8, 8)
    flags = (rsx.WSELECT_FRACTION if fraction else 0) | (rsx.COMPACT_STRICT if strict else 0) | (rsx.COMPACT_INVERT if invert else 0)
    eng.segmented_sample(inp.k.data_ptr() if pass_keys else None, inp.wptr, inp.n, None if inp.o is None else inp.o.data_ptr(), nseg,
                         None if b_in is None else b_in.data_ptr(), t_in.data_ptr(), Rr, flags, inp.kind, weight_exp, i_buf.data_ptr() + 4,
                         m_buf.data_ptr() + 8 if want_mass else None, s_buf.data_ptr() + 8 if want_total else None)
    t.cuda.synchronize()          # the engine runs on its own stream; a device-wide wait leaves its status word to eng.sync()
    index = _unband(i_buf, nseg * Rr * 4, 4, "indices").view(np.uint32).reshape(nseg, Rr)
    mass = _unband(m_buf, nseg * Rr * 8, 8, "masses").view(np.uint64).reshape(nseg, Rr)
    total = _unband(s_buf, nseg * 8, 8, "totals").view(np.uint64)
    assert want_mass or np.all(mass == FILL64), "a NULL d_mass_out: the buffer was not passed"
    assert want_total or np.all(total == FILL64)
    return index, mass if want_mass else None, total if want_total else None


def check(got, ref_out, what=""):
    index, mass, written, total = ref_out
    gi, gm, gt = got
    for name, g, w, mask, fill in (("indices", gi, index, written, FILL32), ("masses", gm, mass, written, FILL64), ("totals", gt, total, None, None)):
        if g is None:
            continue
        want = w if mask is None else np.where(mask, w, w.dtype.type(fill))
        bad = np.argwhere(g != want)
        assert bad.size == 0, f"{what}: {name} differ at {bad[:6].tolist()} (of {len(bad)}): got {g[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    return written


def run_check(rsx, eng, inp, targets, what="", descending=False, **kw):
    ref = R.Referee(inp.weights, inp.off, keys=inp.keys, bounds=kw.get("bounds"), descending=descending, strict=kw.get("strict", False),
                    invert=kw.get("invert", False), weight_exp=kw.get("weight_exp", 0))
    got = run(rsx, eng, inp, targets, **kw)
    return check(got, ref(targets, kw.get("fraction", False)), what), got


def edge_targets(total, Rr, rng, fraction):
    """[S, R]: _wselect_ref.random_targets (0, 1, total, total + 1 among them), as fractions of the total with NaNs where asked"""
    tt = random_targets(total, Rr, rng)
    tt[:, 0] = np.where(rng.random(len(total)) < 0.5, total, tt[:, 0])
    if not fraction:
        return tt
    u = np.where(total[:, None] > 0, tt.astype(np.float64) / np.maximum(total[:, None], 1).astype(np.float64), rng.random(tt.shape))
    u[rng.random(u.shape) < 0.1] = np.nan
    return u


def random_keys(rng, dt, n):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return (rng.standard_normal(n) * 4).astype(dt)
    return rng.integers(-40 if dt.kind == "i" else 0, 60, n).astype(dt)            # few values: ties with every bound


# -- 1. hand cases ---------------------------------------------------------------------------------------------------------------------------------

def test_hand_cases(rsx):
    eng = rsx.Engine(np.uint32, CAP)
    inp = Inputs(np.array([3, 0, 2, 5], dtype=np.uint32), None)
    index, mass, total = run(rsx, eng, inp, np.arange(1, 11, dtype=np.uint64))
    assert index[0].tolist() == [0, 0, 0, 2, 2, 3, 3, 3, 3, 3] and mass[0].tolist() == [3, 3, 3, 5, 5, 10, 10, 10, 10, 10] and total.tolist() == [10]
    index, mass, total = run(rsx, eng, inp, np.array([0, 11], dtype=np.uint64))
    assert np.all(index == FILL32) and np.all(mass == FILL64) and total.tolist() == [10]
    inp = Inputs(np.array([0.5, 0.25, 0.25], dtype=np.float32), None)
    u = np.array([0.0, 0.5, np.nextafter(0.5, 1.0), 0.75, 1.0, np.nan])
    index, mass, total = run(rsx, eng, inp, u, fraction=True)
    assert index[0].tolist() == [0, 0, 1, 1, 2, FILL32] and total.tolist() == [1 << 31]
    assert mass[0].tolist() == [1 << 30, 1 << 30, 3 << 29, 3 << 29, 1 << 31, FILL64]
    eng.sync()
    eng.close()


# -- 2. the ragged matrix --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", KEY_DTYPES)
def test_ragged_matrix(rsx, dt):
    n, off = C.ragged_layout()
    nseg = len(off) - 1
    dtype = np.dtype(dt)
    wcases = [(np.uint32, 0), (np.float32, -3), (np.float64, 5)] + ([(None, 0)] if dtype.kind == "f" else [])
    seen = set()
    for descending in (False, True):
        eng = rsx.Engine(dtype, CAP, descending=descending)
        for wi, (wdt, wexp) in enumerate(wcases):
            rng = np.random.default_rng(4000 + KEY_DTYPES.index(dt) * 100 + wi * 10 + descending)
            if wdt is None:
                keys, w = W.case_weights(rng, dtype, n, off, wexp), None         # the keys are the weights: NaN, +-0, +-inf, negatives among them
            else:
                keys, w = random_keys(rng, dtype, n), W.case_weights(rng, wdt, n, off, wexp)
            inp = Inputs(w, off, keys=keys)
            bounds = keys[np.minimum(off[:-1].astype(np.int64) + rng.integers(0, 9, nseg), n - 1)]       # a key of (or near) the segment: ties occur
            for mode in ("none", "bound", "strict", "invert"):
                kw = dict(weight_exp=wexp)
                if mode != "none":
                    kw.update(bounds=bounds, strict=mode == "strict", invert=mode == "invert")
                total = R.Referee(w, off, keys=keys, bounds=kw.get("bounds"), descending=descending, strict=kw.get("strict", False),
                                  invert=kw.get("invert", False), weight_exp=wexp).total
                for fraction in (False, True):
                    for Rr in (1, 3, 16):
                        tt = edge_targets(total, Rr, rng, fraction)
                        written, got = run_check(rsx, eng, inp, tt, f"{dt} weights={wdt} {mode} descending={descending} fraction={fraction} R={Rr}",
                                                 descending=descending, fraction=fraction, **kw)
                        seen.add((bool(written.any()), bool((~written).any())))
                assert np.any(total > 0) and np.any(total == 0)                   # (the empty segments at least)
        eng.sync()
        eng.close()
    assert seen == {(True, True)}                                                 # every call has slots with and without an answer


# -- 3. the paths --------------------------------------------------------------------------------------------------------------------------------------------

def _targets_of(ref, s_targets, nseg, Rr):
    """[S, R] absolute targets: random ones, with the listed ones planted in the segments given"""
    rng = np.random.default_rng(9)
    tt = random_targets(ref.total, Rr, rng)
    for s, ts in s_targets.items():
        assert len(ts) <= Rr
        tt[s, :len(ts)] = ts
    return tt


@pytest.mark.parametrize("name", sorted(R.LAYOUTS))
def test_paths(rsx, name):
    n, off = R.LAYOUTS[name]()
    nseg = len(off) - 1
    rng = np.random.default_rng(500 + sorted(R.LAYOUTS).index(name))
    w = W.case_weights(rng, np.float32, n, off, 0)
    o = off.astype(np.int64)
    planted = {}
    Rr = 1 if name == "many" else 8
    if name == "hollow":
        w[(o[1] // R.TILE + 1) * R.TILE:(o[2] - 1) // R.TILE * R.TILE] = 0.0      # the middle tiles of segment 1 weigh nothing
    eng = rsx.Engine(np.uint32, CAP)
    inp = Inputs(w, off)
    ref = R.Referee(w, off)
    if name == "crossing":
        f = R.walk_facts(ref.m, off, 1)
        first = f["pieces"][0]
        assert first > 0 and f["pieces"][1] > 0
        planted[1] = [1, first - 1, first, first + 1, int(ref.total[1]), first // 2, first + f["pieces"][1] // 2]      # answers in both pieces
    elif name == "hollow":
        f = R.walk_facts(ref.m, off, 1)
        assert f["pieces"][0] > 0 and f["pieces"][-1] > 0 and not any(f["pieces"][1:-1])
        planted[1] = [1, f["pieces"][0], f["pieces"][0] + 1, int(ref.total[1])]
    elif name == "long":
        planted[R.LONG_SEGMENT] = R.long_targets(ref.m, off)
        assert len(planted[R.LONG_SEGMENT]) == 4
    tt = _targets_of(ref, planted, nseg, Rr)
    got = run(rsx, eng, inp, tt)
    written = check(got, ref(tt), name)
    for s, ts in planted.items():
        assert written[s, :len(ts)].all()
    if name == "crossing":                                                       # T = the first piece's mass is answered in the first tile, + 1 in the second
        split = R.TILE - int(o[1])
        assert got[0][1, 2] < split <= got[0][1, 3] and got[0][1, 5] < split <= got[0][1, 6]
    if name == "long":                                                           # the chunk's prefix is answered in the first chunk, prefix + 1 behind it
        edge = (int(o[1]) // R.TILE + R.WALK_TILES) * R.TILE - int(o[1])
        assert got[0][1, 2] < edge <= got[0][1, 3]
    # fractions too, on the same upload
    u = rng.random((nseg, Rr))
    check(run(rsx, eng, inp, u, fraction=True), ref(u, True), name + " fractions")
    eng.sync()
    eng.close()


# -- 4. pointers ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wdt", [np.uint32, np.float32, np.float64])
def test_pointers(rsx, wdt):
    n, off = R.inner_layout()
    rng = np.random.default_rng(77)
    wexp = 0 if wdt == np.uint32 else 2
    w = W.case_weights(rng, wdt, n, off, wexp)
    keys = random_keys(rng, np.int32, n)
    eng = rsx.Engine(np.int32, CAP)
    ref = R.Referee(w, off, weight_exp=wexp)
    tt = random_targets(ref.total, 3, rng)
    results = []
    for skew in (0, 1, 2, 3):                                                    # the weights start that many elements past a 16-byte boundary
        inp = Inputs(w, off, keys=keys, skew=skew)
        got = run(rsx, eng, inp, tt, weight_exp=wexp, pass_keys=False)            # d_keys = NULL where it is not read
        check(got, ref(tt), f"skew {skew}")
        results.append(got)
    assert all(np.array_equal(r[0], results[0][0]) for r in results)
    inp = Inputs(w, off, keys=keys)
    check(run(rsx, eng, inp, tt, weight_exp=wexp, want_mass=False), ref(tt), "no mass output")
    check(run(rsx, eng, inp, tt, weight_exp=wexp, want_total=False), ref(tt), "no total output")
    one = Inputs(w, None)                                                        # d_offsets = NULL: one segment [0, n)
    ref1 = R.Referee(w, None, weight_exp=wexp)
    t1 = random_targets(ref1.total, 16, rng)
    t1[0, :3] = [1, int(ref1.total[0]), int(ref1.total[0]) // 2]
    check(run(rsx, eng, one, t1, weight_exp=wexp), ref1(t1), "one segment")
    eng.sync()
    eng.close()


# -- 5. the sort state ------------------------------------------------------------------------------------------------------------------------------------------

def test_sort_state_is_untouched_and_n_exceeds_capacity(rsx):
    t = _torch()
    rng = np.random.default_rng(61)
    x = rng.integers(0, 1 << 32, CAP, dtype=np.uint32)
    xd = dev(t, x)
    n = 3 * CAP + 17
    w = W.case_weights(rng, np.float64, n, None, 0)
    keys = rng.integers(0, 80, n).astype(np.uint32)
    off = np.array([7, 5000, 5000, n - 10], dtype=np.uint64)
    res = []
    for payload in (False, True):
        eng = rsx.Engine(np.uint32, CAP, payload=payload)
        pd = dev(t, np.arange(CAP, dtype=np.uint32)) if payload else None
        eng.sort_from(xd.data_ptr(), CAP, pd.data_ptr() if payload else None)
        inp = Inputs(w, off, keys=keys)
        ref = R.Referee(w, off, keys=keys, bounds=np.array([40, 40, 40], dtype=np.uint32))
        tt = random_targets(ref.total, 4, rng)
        got = run(rsx, eng, inp, tt, bounds=np.array([40, 40, 40], dtype=np.uint32))
        check(got, ref(tt), f"payload={payload}")
        res.append(got[2])
        assert eng.geometry().num_keys == CAP
        out = t.zeros(CAP, dtype=t.int32, device="cuda")
        t.cuda.synchronize()                                                     # (the engine copies on its own stream)
        eng.copy_result(out.data_ptr())
        eng.sync()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), np.sort(x))
        eng.close()
    assert np.array_equal(res[0], res[1])


# -- 6. bad offsets ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", ["decreasing", "past_n"])
def test_bad_offsets_reported_once(rsx, bad):
    rng = np.random.default_rng(23)
    n = 40000
    w = W.case_weights(rng, np.float32, n, None, 0)
    off = np.array([0, 100, 5000, 4000 if bad == "decreasing" else n + 1, n], dtype=np.uint64)       # segment 2 is the first bad one
    eng = rsx.Engine(np.uint32, CAP)
    tt = np.ones((4, 2), dtype=np.uint64)
    index, mass, total = run(rsx, eng, Inputs(w, off), tt)                        # guard bands checked inside
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "rsx_segmented_sample" in str(ei.value) and "segment 2 " in str(ei.value)
    eng.sync()                                                                   # reported once
    assert np.all(index == FILL32) and np.all(mass == FILL64) and np.all(total == FILL64)
    good = np.array([0, 3, 5000, 5001, n], dtype=np.uint64)                        # the engine stays usable: the next call is right
    run_check(rsx, eng, Inputs(w, good), tt, "after bad offsets")
    eng.sync()
    eng.close()


# -- 7. two independent kernels agree ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("descending", [False, True])
def test_agrees_with_weighted_select_on_sorted_segments(rsx, descending):
    n, off = C.ragged_layout()
    nseg = len(off) - 1
    rng = np.random.default_rng(88 + descending)
    keys = rng.integers(0, 1000, n).astype(np.uint32)
    o = off.astype(np.int64)
    for s in range(nseg):                                                        # stably sorted in the engine's direction: sorted order = index order
        seg = np.sort(keys[o[s]:o[s + 1]])
        keys[o[s]:o[s + 1]] = seg[::-1] if descending else seg
    w = W.case_weights(rng, np.float32, n, off, 0)
    ref = R.Referee(w, off)
    tt = random_targets(ref.total, 4, rng)
    _, wpos, _, wmass, wtotal, weng = wselect_run(rsx, keys, off, w, tt, descending=descending)
    weng.sync()
    weng.close()
    eng = rsx.Engine(np.uint32, CAP)
    index, mass, total = run(rsx, eng, Inputs(w, off), tt)
    eng.sync()
    eng.close()
    assert np.array_equal(index, wpos) and np.array_equal(mass, wmass) and np.array_equal(total, wtotal)
    assert np.any(index != FILL32) and np.any(index == FILL32)


# -- 8. reproducibility ------------------------------------------------------------------------------------------------------------------------------------------

def test_reproducible_across_engines_streams_and_replays(rsx):
    t = _torch()
    rng = np.random.default_rng(70)
    n, off = C.ragged_layout()
    nseg, Rr = len(off) - 1, 3
    keys = W.case_weights(rng, np.float32, n, off, 0)                            # self-weights with a bound, fractions
    bounds = np.full(nseg, 0.25, dtype=np.float32)
    u = rng.random((nseg, Rr))
    kd, od, bd, ud = dev(t, keys), dev(t, off), dev(t, bounds), dev(t, u)
    flags = rsx.WSELECT_FRACTION
    want = R.Referee(None, off, keys=keys, bounds=bounds, descending=True)(u, True)
    results = []
    for i, cap in enumerate((CAP, 1 << 20)):
        side = t.cuda.Stream()
        eng = rsx.Engine(np.float32, cap, descending=True)
        eng.set_stream(side.cuda_stream)
        iout, mout, tout = (dev(t, np.full(nseg * Rr * 4, FILL, dtype=np.uint8)), dev(t, np.full(nseg * Rr * 8, FILL, dtype=np.uint8)),
                            dev(t, np.full(nseg * 8, FILL, dtype=np.uint8)))
        call = lambda: eng.segmented_sample(kd.data_ptr(), None, n, od.data_ptr(), nseg, bd.data_ptr(), ud.data_ptr(), Rr, flags, rsx.WEIGHT_FLOAT32, 0,
                                            iout.data_ptr(), mout.data_ptr(), tout.data_ptr())
        result = lambda: (iout.cpu().numpy().view(np.uint32).reshape(nseg, Rr).copy(), mout.cpu().numpy().view(np.uint64).reshape(nseg, Rr).copy(),
                          tout.cpu().numpy().view(np.uint64).copy())
        call()                                                                   # eager: the first call of an engine allocates its scratch
        eng.sync()
        results.append(result())
        check(results[-1], want, f"capacity {cap}")
        if i == 1:                                                               # a linear capture on the side stream: no parallel branches
            graph = t.cuda.CUDAGraph()
            with t.cuda.graph(graph, stream=side):
                call()
            for rep in range(2):
                keys2 = W.case_weights(rng, np.float32, n, off, 0)
                u2 = rng.random((nseg, Rr))
                kd.copy_(dev(t, keys2))                                          # rewritten in place
                ud.copy_(dev(t, u2))
                for buf in (iout, mout, tout):
                    buf.fill_(FILL - 256)
                t.cuda.synchronize()
                graph.replay()
                t.cuda.synchronize()
                check(result(), R.Referee(None, off, keys=keys2, bounds=bounds, descending=True)(u2, True), f"replay {rep}")
            del graph
        eng.sync()
        eng.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(results[0], results[1]))


# -- 9. refusals --------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals(rsx):
    t = _torch()
    n = 100
    w = dev(t, np.ones(n + 4, dtype=np.float32))
    k = dev(t, np.ones(n + 4, dtype=np.float32))
    o = dev(t, np.array([0, 50, n], dtype=np.uint64))
    b = dev(t, np.ones(2, dtype=np.float32))
    tt = dev(t, np.ones(4, dtype=np.uint64))
    iout, mout, tout = dev(t, np.zeros(8, dtype=np.uint32)), dev(t, np.zeros(4, dtype=np.uint64)), dev(t, np.zeros(2, dtype=np.uint64))
    feng, ieng = rsx.Engine(np.float32, CAP), rsx.Engine(np.uint32, CAP)
    F32 = rsx.WEIGHT_FLOAT32

    def refused(status, text, eng, *args):
        with pytest.raises(rsx.RadixSortError) as ei:
            eng.segmented_sample(*args)
        assert ei.value.status == status and "rsx_segmented_sample" in str(ei.value) and text in str(ei.value), str(ei.value)

    base = lambda **kw: tuple({**dict(d_keys=k.data_ptr(), d_weights=w.data_ptr(), n=n, d_offsets=o.data_ptr(), num_segments=2, d_bounds=None,
                                      d_targets=tt.data_ptr(), R=2, flags=0, kind=F32, wexp=0, iout=iout.data_ptr(), mout=mout.data_ptr(),
                                      tout=tout.data_ptr()), **kw}.values())
    refused(4, "flags", feng, *base(flags=1))                                                       # unknown flag bits
    refused(4, "flags", feng, *base(flags=rsx.COMPACT_PARTITION))
    refused(4, "bound form", feng, *base(flags=rsx.COMPACT_STRICT))                                 # strict or invert without bounds
    refused(4, "bound form", feng, *base(flags=rsx.COMPACT_INVERT | rsx.WSELECT_FRACTION))
    refused(4, "weight_exp", feng, *base(wexp=2049))
    refused(4, "weight_exp", feng, *base(wexp=-2049))
    refused(4, "weight_exp", feng, *base(kind=rsx.WEIGHT_UINT32, wexp=1))
    refused(4, "weight_kind", feng, *base(kind=3))
    refused(1, "the keys are the weights", ieng, *base(d_weights=None))                             # self-weights on an integer engine
    refused(1, "the keys are the weights", feng, *base(d_weights=None, kind=rsx.WEIGHT_FLOAT64))
    refused(1, "weights must be aligned", feng, *base(d_weights=w.data_ptr() + 2))                  # misaligned pointers
    refused(1, "16-byte aligned", feng, *base(d_keys=k.data_ptr() + 4, d_bounds=b.data_ptr()))
    refused(1, "16-byte aligned", feng, *base(d_keys=None, d_weights=None))
    refused(1, "targets", feng, *base(d_targets=tt.data_ptr() + 4))
    refused(1, "index output", feng, *base(iout=iout.data_ptr() + 2))
    refused(1, "8-byte aligned", feng, *base(mout=mout.data_ptr() + 4))
    refused(1, "overlaps an input", feng, *base(iout=tt.data_ptr()))                                # overlapping buffers
    refused(1, "two outputs overlap", feng, *base(mout=tout.data_ptr()))
    refused(4, "2^31 draws", feng, *base(num_segments=1 << 20, R=(1 << 11) + 1))                     # S * R above 2^31
    # accepted and empty: R == 0, n == 0, no segments
    feng.segmented_sample(*base(R=0))
    feng.segmented_sample(*base(n=0))
    feng.segmented_sample(*base(num_segments=0))
    feng.sync()
    assert bool((iout == 0).all())
    feng.close()
    ieng.close()


# -- 10. the helpers ------------------------------------------------------------------------------------------------------------------------------------------------

UNITS = 1 << 24


def dyadic_rows(t, rows, cols, gen):
    """[rows, cols] float32 on the device: non-negative multiples of 2^-24 that sum to 1 in every row (the gaps of sorted random cuts)"""
    cuts = t.randint(0, UNITS + 1, (rows, cols - 1), dtype=t.int32, device="cuda", generator=gen).sort(dim=1).values
    edges = t.cat([t.zeros((rows, 1), dtype=t.int32, device="cuda"), cuts, t.full((rows, 1), UNITS, dtype=t.int32, device="cuda")], dim=1)
    return ((edges[:, 1:] - edges[:, :-1]).to(t.float32) / float(UNITS)).contiguous()


def chain(rsx, t, probs, u, bound):
    """what sample_rows replaces: compact the nucleus, scan its masses, search the target, gather the column"""
    rows = probs.shape[0]
    nucleus, row_off, cols = rsx.compact_rows(probs, bound=bound, descending=True, return_index=True)
    m = (nucleus.to(t.float64) * float(1 << 31)).to(t.int64)                      # exact for multiples of 2^-24
    run = t.cumsum(m, 0)
    base = t.cat([run.new_zeros(1), run])[row_off[:-1]]
    total = t.cat([run.new_zeros(1), run])[row_off[1:]] - base
    td = total.to(t.float64)
    x = td * u
    T = t.where(x > 1.0, t.where(x >= td, total, t.ceil(x).to(t.int64)), t.ones_like(total))     # the referee's target rule
    pos = rsx.segmented_searchsorted(run, row_off, T + base, t.arange(0, rows + 1, device=probs.device, dtype=t.int64))
    flat = t.clamp(row_off[:-1] + pos, max=max(cols.numel() - 1, 0))
    return t.where(total > 0, cols[flat], t.full_like(total, -1))


def test_multinomial_and_sample_rows(rsx):
    t = _torch()
    gen = t.Generator(device="cuda")
    gen.manual_seed(5)
    rows, cols = 64, 5000
    probs = dyadic_rows(t, rows, cols, gen)
    probs[3] = 0.0                                                               # a row of zeros
    u = t.rand((rows, 4), dtype=t.float64, device="cuda", generator=gen)
    # multinomial with a given u equals the referee
    got = rsx.multinomial(probs, 4, u=u)
    off = np.arange(rows + 1, dtype=np.uint64) * cols
    index, _, written, _ = R.sample_oracle(probs.cpu().numpy().reshape(-1), off, u.cpu().numpy(), fraction=True)
    want = np.where(written, index.astype(np.int64), -1)
    assert got.dtype == t.int64 and np.array_equal(got.cpu().numpy(), want) and np.all(want[3] == -1) and np.all(np.delete(want, 3, 0) >= 0)
    assert np.array_equal(rsx.multinomial(probs.t().contiguous(), 4, dim=0, u=u).cpu().numpy(), want)
    # two generators with one seed give equal bits
    draws = []
    for _ in range(2):
        g = t.Generator(device="cuda")
        g.manual_seed(1234)
        draws.append(rsx.multinomial(probs, 8, generator=g))
    assert t.equal(draws[0], draws[1]) and draws[0].shape == (rows, 8)
    # sample_rows against the chain it replaces
    u1 = u[:, 0].contiguous()
    p = t.randint(1, 1025, (rows,), device="cuda", generator=gen).to(t.float64) / 1024.0
    thr = rsx.top_p(probs, p)[0]
    a = rsx.sample_rows(probs, u1, top_p=p)
    assert t.equal(a, chain(rsx, t, probs, u1, thr)) and int(a[3]) == -1 and bool((a >= -1).all()) and int((a >= 0).sum()) == rows - 1
    kth = rsx.kthvalue(probs, cols - 50 + 1)[0]
    assert t.equal(rsx.sample_rows(probs, u1, top_k=50), chain(rsx, t, probs, u1, kth))
    floor = rsx.amax(probs) * 0.125
    assert t.equal(rsx.sample_rows(probs, u1, min_p=0.125), chain(rsx, t, probs, u1, floor))
    both = t.maximum(t.maximum(thr, kth), floor)
    assert t.equal(rsx.sample_rows(probs, u1, top_k=50, top_p=p, min_p=0.125), chain(rsx, t, probs, u1, both))
    # without a filter it is multinomial's first draw
    assert t.equal(rsx.sample_rows(probs, u1), got[:, 0])
    zeros = t.zeros((2, 7), dtype=t.float32, device="cuda")
    assert rsx.sample_rows(zeros, top_p=0.9).tolist() == [-1, -1] and rsx.multinomial(zeros, 2).tolist() == [[-1, -1], [-1, -1]]


def test_segmented_sample_helper(rsx):
    t = _torch()
    n, off = C.ragged_layout()
    nseg = len(off) - 1
    rng = np.random.default_rng(3)
    w = W.case_weights(rng, np.float32, n, off, -3)
    keys = random_keys(rng, np.int64, n)
    bounds = np.full(nseg, 10, dtype=np.int64)
    ref = R.Referee(w, off, keys=keys, bounds=bounds, descending=True, strict=True, weight_exp=-3)
    tt = random_targets(ref.total, 3, rng)
    index, mass, total = rsx.segmented_sample(dev(t, w).view(t.float32), dev(t, off), targets=dev(t, tt), keys=dev(t, keys), bound=dev(t, bounds),
                                              strict=True, descending=True, weight_exp=-3)
    wi, wm, written, wt = ref(tt)
    assert np.array_equal(index.cpu().numpy(), np.where(written, wi.astype(np.int64), -1))
    assert np.array_equal(mass.cpu().numpy(), np.where(written, wm, 0).astype(np.int64)) and np.array_equal(total.cpu().numpy().view(np.uint64), wt)
    # 1-D u, float32 widened, self-weights with a bound, one segment without offsets
    u = t.rand(1, device="cuda")
    i1, m1, t1 = rsx.segmented_sample(dev(t, w).view(t.float32), None, u=u, bound=t.zeros(1, device="cuda"), descending=True)
    r1 = R.sample_oracle(None, None, u.double().cpu().numpy(), fraction=True, keys=w, bounds=np.zeros(1, dtype=np.float32), descending=True)
    assert i1.shape == (1,) and int(i1[0]) == int(r1[0][0, 0]) and int(m1[0]) == int(r1[1][0, 0]) and int(t1[0]) == int(r1[3][0])
