"""rsx_segmented_weighted_select on the launch paths of rsx_wselect.hpp and capi_wselect.inc that tests/test_gpu_wselect.py never
reaches (every layout there runs one tile per group and gives no workgroup of any kernel a second item):

  A  groups of two tiles that end one large segment and begin the next (the flush / step / reload inside wselect_hist_kernel, START and
     CONT rows from one workgroup, the pick's group range), and the grid strides of the pick, find, locate and tie kernels;
  B  more small segments than workgroups in each LDS class: wselect_sort_kernel's second item, a shorter segment over the stale image
     and over the 64-bit scan scratch that aliases the counters; the same layouts through select_sort_kernel of the plain select;
  C  a segment of more than 1024 tiles: the carries between the chunks of wselect_find_kernel;
  D  weights aligned to their element but not to 16 bytes (the element-wise loads of whole tiles), and absent optional outputs;
  E  the mass function on the device at the ends of both exponent ranges;
  F  one engine across these layouts: scratch rows laid out for one tile per group, then two, then one again.

The layouts and the mirror of the launch geometry are held in tests/_wselect_ref.py and tests/_segmented_ref.py (tests/test_wselect.py
checks on the CPU, at 256 CUs, that each reaches its path); every test here rebuilds its layout for the device's own CU count, prints
the figures and asserts the path condition again before it compares.  Every comparison is exact equality of bits against the referee
of tests/_wselect_ref.py (tests/_select_ref.py for the plain select): keys, positions, ranks, masses and totals, with run()'s sentinel
in every slot the call may not write and guard bands around every output.  One sort per upload serves all its calls (W.Referee).
"""
import numpy as np
import pytest

import _segmented_ref as S
import _wselect_ref as W
from _select_ref import fast_select
from test_gpu_float_keys import UINT, random_bits
from test_gpu_segmented import _torch, dev, offsets_from
from test_gpu_select import check as select_check
from test_gpu_select import run as select_run
from test_gpu_wselect import LENGTHS, _band, _fill, _unband, edge_fractions, edge_targets, make_weights, run

pytestmark = pytest.mark.gpu


def device_cus():
    return int(_torch().cuda.get_device_properties(0).multi_processor_count)


def expect(got, want, absent=False, what=""):
    """check() of test_gpu_wselect.py against an answer of W.Referee; absent: the call had no rank, mass and total outputs, their
    buffers still hold the sentinel everywhere"""
    wk, wi, wr, wm, written, total, valid = want
    opt = np.zeros_like(written) if absent else written
    for name, g, w, mask in (("keys", got[0], wk, written), ("positions", got[1], wi, written), ("ranks", got[2], wr, opt), ("masses", got[3], wm, opt),
                             ("totals", got[4], total, np.zeros_like(valid) if absent else valid)):
        bad = np.argwhere(g != np.where(mask, w, _fill(g.dtype)))
        assert bad.size == 0, f"{what} {name} differ at {bad[:8].tolist()} (of {len(bad)}): got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"
    return written


def same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:5], b[:5]))


def with_ties(dtype, n, rng):
    x = random_bits(dtype, n, rng)
    x[rng.integers(0, n, n // 3)] = x[rng.integers(0, n, n // 3)]
    return x


def own_weights(dtype, n, rng):
    """float keys that are their own weights, as test_kinds_directions_targets makes them: ties, zeros, negatives, NaNs"""
    p = np.ldexp(rng.random(n), -rng.integers(0, 20, n)).astype(dtype)
    p[rng.integers(0, n, n // 4)] = p[rng.integers(0, n, n // 4)]
    p[rng.integers(0, n, n // 10)] = 0.0
    p[rng.integers(0, n, n // 100)] = -p[rng.integers(0, n, n // 100)]
    p[rng.integers(0, n, 50)] = np.nan
    return p


class Case:
    """one upload: layout, keys, weights, the referee's sort, and absolute targets with their answer"""

    def __init__(self, n, off, x, w, descending, R, rng, targets=edge_targets, weight_exp=0):
        self.n, self.off, self.x, self.w, self.descending, self.R, self.weight_exp = n, off, x, w, descending, R, weight_exp
        self.ref = W.Referee(x, off, w, descending, weight_exp)
        self.tt = targets(self.ref.total, R, rng)
        self.want = self.ref(self.tt)

    def run(self, rsx, eng=None, what=""):
        got = run(rsx, self.x, self.off, self.w, self.tt, False, self.descending, self.weight_exp, eng=eng)
        expect(got, self.want, what=what)
        return got


_SHARED = {}       # the int32 ascending cases that F runs again on one engine: built once, never changed


def shared(name, cus):
    if (name, cus) not in _SHARED:
        _SHARED[(name, cus)] = {"many_large": lambda: many_large_case(cus, 0), "stride0": lambda: stride_case(cus, 0),
                                "long": lambda: long_case("0_to_6", False), "lengths": lengths_case}[name]()
    return _SHARED[(name, cus)]


# -- A. shared groups, and every chain kernel striding ------------------------------------------------------------------------------------------

# key type, weight kind (None: the keys are the weights), descending, R of each call: RC = 4, 4 (R = 3), 2 and 1 meet the mid-group flush
MANY = [(np.int32, 1, False, (4,)), (np.uint64, 2, True, (3,)), (np.float32, None, True, (2, 1))]


def many_large_case(cus, i):
    dtype, kind, desc, Rs = MANY[i]
    n, off = W.many_large(cus)
    rng = np.random.default_rng(71 + i)
    x = own_weights(dtype, n, rng) if kind is None else with_ties(dtype, n, rng)
    return Case(n, off, x, None if kind is None else make_weights(kind, n, rng), desc, Rs[0], rng)


def assert_many_large_path(c, cus):
    for R in (4, c.R):
        g = W.wselect_geometry(c.off, c.n, R, cus)
        print(W.summary(g))
        assert g["gtiles"] >= 2 and g["switches"] >= cus and g["tiles"] > g["tie_grid"]
        assert g["items"] > 2 * g["pick_grid"] if R == 4 else g["items"] >= 2 * g["pick_grid"]


@pytest.mark.parametrize("i", range(len(MANY)), ids=["int32-f32-asc-R4", "uint64-f64-desc-R3", "float32-self-desc-R2-R1"])
def test_many_large_segments_share_groups_and_stride(rsx, i):
    """W.many_large: about half of the 4 * cus large segments begin on the second tile of a group, so the workgroup of that group flushes a
    CONT (or START) row, steps to the next segment, reloads R prefixes (inactive slots among active ones: edge targets) and writes a
    START row in the same trip; every workgroup of the pick, find and locate kernels takes eight items at R = 4, and the tie kernel's
    workgroups a second tile.  Absolute form, then fractions on the same engine."""
    cus = device_cus()
    c = shared("many_large", cus) if i == 0 else many_large_case(cus, i)
    assert_many_large_path(c, cus)
    got = c.run(rsx)
    assert c.want[4].any() and not c.want[4].all()
    rng = np.random.default_rng(81 + i)
    fr = edge_fractions(len(c.off) - 1, c.R, rng)
    got = run(rsx, c.x, c.off, c.w, fr, True, c.descending, eng=got[5])
    expect(got, c.ref(fr, True), what="fractions")
    for R in MANY[i][3][1:]:                                                 # a smaller compiled capacity on the same engine and upload
        assert W.wselect_geometry(c.off, c.n, R, cus)["items"] >= 2 * W.wselect_geometry(c.off, c.n, R, cus)["pick_grid"]
        tt = edge_targets(c.ref.total, R, rng)
        got = run(rsx, c.x, c.off, c.w, tt, False, c.descending, eng=got[5])
        expect(got, c.ref(tt), what=f"R={R}")
        fr = edge_fractions(len(c.off) - 1, R, rng)
        got = run(rsx, c.x, c.off, c.w, fr, True, c.descending, eng=got[5])
        expect(got, c.ref(fr, True), what=f"R={R} fractions")


# -- B. more small segments than workgroups -------------------------------------------------------------------------------------------------------

# per class: key type, weight kind, descending, R
STRIDE = [(np.int32, 0, False, 4), (np.uint64, 1, True, 2), (np.float32, 2, False, 2)]
STRIDE_SELECT = [(np.uint32, True), (np.int64, False), (np.float64, True)]


def stride_case(cus, cls):
    dtype, kind, desc, R = STRIDE[cls]
    n, off = S.stride_layout(cls, cus)
    rng = np.random.default_rng(91 + cls)
    return Case(n, off, S.few_distinct(dtype, off, n, rng), make_weights(kind, n, rng), desc, R, rng, targets=W.random_targets)


def assert_stride_path(off, n, R, cls, cus):
    g = W.wselect_geometry(off, n, R, cus)
    print(W.summary(g))
    assert g["trips"][cls] >= 2 and g["count"][cls] > g["sort_grid"][cls] == cus * S.PER_CU[cls]
    assert W.second_items_are_shorter(g, off, cls)


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_more_small_segments_than_workgroups(rsx, cls):
    """S.stride_layout: 400 (200 in class 2) workgroups of wselect_sort_kernel sort and scan a second segment, a shorter one: its pads
    lie over the first one's image, and the wave totals of the first one's 64-bit scan lie in the counters that the second sort clears"""
    cus = device_cus()
    c = shared("stride0", cus) if cls == 0 else stride_case(cus, cls)
    assert_stride_path(c.off, c.n, c.R, cls, cus)
    c.run(rsx)
    assert c.want[4].any() and not c.want[4].all()


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_more_small_segments_than_workgroups_plain_select(rsx, cls):
    """the same layouts through select_sort_kernel (rsx_segmented_select), whose item loop has the same gap: ranks 0, len - 1 and a
    random one of every segment, keys and positions against tests/_select_ref.py"""
    cus = device_cus()
    dtype, desc = STRIDE_SELECT[cls]
    n, off = S.stride_layout(cls, cus)
    assert_stride_path(off, n, 3, cls, cus)
    rng = np.random.default_rng(97 + cls)
    x = S.few_distinct(dtype, off, n, rng)
    lens = np.diff(off.astype(np.int64))
    ranks = np.stack([np.zeros_like(lens), lens - 1, rng.integers(0, lens)], axis=1).astype(np.uint32)
    k, i, _ = select_run(rsx, x, off, ranks, desc)
    select_check(x, off, ranks, k, i, desc, referee=fast_select)


# -- C. a segment of more than 1024 tiles ---------------------------------------------------------------------------------------------------------

def long_case(keys, desc):
    n, off = W.long_segment()
    rng = np.random.default_rng(101 + (keys == "0_to_6"))
    x = np.full(n, 77, dtype=np.int32) if keys == "all_equal" else rng.integers(0, 7, n).astype(np.int32)
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)

    def targets(total, R, rng):
        tt = W.random_targets(total, R, rng)
        tt[W.LONG_SEGMENT] = W.long_targets(int(total[W.LONG_SEGMENT]))
        return tt

    return Case(n, off, x, w, desc, 4, rng, targets=targets)


@pytest.mark.parametrize("keys", ["all_equal", "0_to_6"])
def test_segment_of_more_than_1024_tiles(rsx, keys):
    """W.long_segment: wselect_find_kernel walks the 1031 tiles of segment 1 in two chunks and carries the tie mass and the tie count of
    the first 1024 into the second: an answer in tile 1024 or beyond has its rank and its mass from the carries.  All keys equal: the
    whole segment is one run of ties; keys 0..6: the run of the last key in the call's order ends the segment.  The targets total - 5,
    total / 2, total * 1025 / 1030 and 1 land in tiles 1030, 515, 1025 and 0 (all equal) and 1030, 515, about 995 and 0 (keys 0..6: the
    third target lies 96.6 % into the last key's run, whichever the seed), so over the two directions of either key set at least two
    answers come from the second chunk and at least one from the first; every call has one of each.  A second call per direction puts
    all four targets into the last five tiles."""
    cus = device_cus()
    high = low = 0
    for desc in (False, True):
        c = shared("long", cus) if (keys, desc) == ("0_to_6", False) else long_case(keys, desc)
        g = W.wselect_geometry(c.off, c.n, 4, cus)
        tiles = W.answer_tiles(c.off, W.LONG_SEGMENT, c.want[1][W.LONG_SEGMENT])
        print(W.summary(g), "answers in tiles", tiles)
        assert g["max_segment_tiles"] > W.FIND_CHUNK and c.want[4][W.LONG_SEGMENT].all()
        assert max(tiles) >= W.FIND_CHUNK > min(tiles)
        high += sum(t >= W.FIND_CHUNK for t in tiles)
        low += sum(t < W.FIND_CHUNK for t in tiles)
        got = c.run(rsx, what="desc" if desc else "asc")
        total = int(c.ref.total[W.LONG_SEGMENT])
        tt = c.tt.copy()
        tt[W.LONG_SEGMENT] = [total, total - total // 4000, total - total // 2000, total - total // 1500]
        want = c.ref(tt)
        tail = W.answer_tiles(c.off, W.LONG_SEGMENT, want[1][W.LONG_SEGMENT])
        print("tail answers in tiles", tail)
        assert min(tail) >= W.FIND_CHUNK
        expect(run(rsx, c.x, c.off, c.w, tt, False, desc, eng=got[5]), want, what="tail")
    assert high >= 2 and low >= 1


# -- D. weights not aligned to 16 bytes -----------------------------------------------------------------------------------------------------------

def run_at(rsx, eng, x, off, w, shift, targets, absent=False):
    """run() of test_gpu_wselect.py with the weights `shift` elements into a buffer that is `shift` elements longer (the element before
    them weighs as much as a weight can), and, when `absent`, without the rank, mass and total outputs: their buffers are still made,
    banded and read back, and must hold the sentinel"""
    t = _torch()
    n, nseg = x.size, len(off) - 1
    tt = np.ascontiguousarray(np.asarray(targets, dtype=np.uint64).reshape(nseg, -1))
    R = tt.shape[1]
    ks = x.dtype.itemsize
    heavy = np.full(shift, 0xFFFFFFFF if w.dtype == np.uint32 else np.inf, dtype=w.dtype)
    w_buf = dev(t, np.concatenate([heavy, w]))
    w_ptr = w_buf.data_ptr() + shift * w.dtype.itemsize
    assert w_buf.data_ptr() % 16 == 0 and w_ptr % w.dtype.itemsize == 0 and (w_ptr % 16 == 0) == (shift == 0)
    k_in, o, t_in = dev(t, x), dev(t, np.asarray(off, dtype=np.uint64)), dev(t, tt)
    bufs = [_band(t, nseg * R * ks, ks, 0), _band(t, nseg * R * 4, 4, 0), _band(t, nseg * R * 4, 4, 0), _band(t, nseg * R * 8, 8, 0), _band(t, nseg * 8, 8, 0)]
    ptrs = [b.data_ptr() + g for b, g in bufs]
    eng.segmented_weighted_select(k_in.data_ptr(), w_ptr, n, o.data_ptr(), nseg, t_in.data_ptr(), R, 0, W.kind_of(w), 0,
                                  *(ptrs[:2] + [None, None, None] if absent else ptrs))
    t.cuda.synchronize()
    eng.sync()
    sizes = [nseg * R * ks, nseg * R * 4, nseg * R * 4, nseg * R * 8, nseg * 8]
    views = [UINT[x.dtype], np.uint32, np.uint32, np.uint64, np.uint64]
    out = [_unband(b, g, size, name).view(v) for (b, g), size, name, v in zip(bufs, sizes, ("key", "index", "rank", "mass", "total"), views)]
    return [a.reshape(nseg, R) for a in out[:4]] + [out[4]]


def lengths_case():
    off = offsets_from(LENGTHS, start=3)
    n = int(off[-1]) + 5
    rng = np.random.default_rng(131)
    return Case(n, off, with_ties(np.int32, n, rng), make_weights(2, n, rng), False, 4, rng)


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["u32", "f32", "f64"])
@pytest.mark.parametrize("dtype", [np.uint32, np.int64], ids=lambda d: np.dtype(d).name)
def test_weights_aligned_to_their_element_only(rsx, dtype, kind):
    """The LENGTHS layout of test_gpu_wselect.py with the weights one element (4 bytes; 8 for float64) past a 16-byte boundary, which the
    header allows: wselect_hist_kernel must load the weights of whole tiles element by element.  Equal to the referee, and byte for byte
    to the call on a 16-byte aligned upload of the same values on the same engine (where it takes the vector loads); then once without
    rank, mass and total outputs, which reaches the NULL checks of wselect_init_kernel, of all three LDS classes and of the chain."""
    off = offsets_from(LENGTHS, start=3)
    n = int(off[-1]) + 5
    g = W.wselect_geometry(off, n, 4, device_cus())
    print(W.summary(g))
    assert g["nlarge"] >= 5 and g["tiles"] - 2 * g["nlarge"] >= 100 and min(g["count"]) >= 1           # whole tiles, and every LDS class
    rng = np.random.default_rng(111 + 3 * (np.dtype(dtype).itemsize == 8) + kind)
    x = with_ties(dtype, n, rng)
    w = make_weights(kind, n, rng)
    ref = W.Referee(x, off, w)
    tt = edge_targets(ref.total, 4, rng)
    want = ref(tt)
    eng = rsx.Engine(dtype, n)
    aligned = run_at(rsx, eng, x, off, w, 0, tt)
    expect(aligned, want, what="aligned")
    shifted = run_at(rsx, eng, x, off, w, 1, tt)
    expect(shifted, want, what="shifted")
    assert same_bits(aligned, shifted)
    expect(run_at(rsx, eng, x, off, w, 1, tt, absent=True), want, absent=True, what="no optional outputs")
    expect(run_at(rsx, eng, x, off, w, 0, tt, absent=True), want, absent=True, what="aligned, no optional outputs")


# -- E. weight exponents --------------------------------------------------------------------------------------------------------------------------

def test_weight_exponents_on_the_device(rsx):
    """W.exponent_cases: float32 and float64 weights around 2^weight_exp for weight_exp at the ends of both exponent ranges and of the
    accepted range, half of them with masses just below saturation, half random bit patterns with infinities, NaNs and denormals
    planted: the shifts of rsx_mass_math.hpp as the device compiles them, exact against mass_np in keys, positions, ranks, masses and
    totals.  All sixteen cases have an answer (a planted +inf weighs 2^31 at any exponent; ten are asked for), segment 0 of the last
    cases weighs nothing, and at weight_exp = -2048 every positive weight is saturated."""
    off = offsets_from(W.EXP_LENGTHS)
    n = int(off[-1])
    g = W.wselect_geometry(off, n, 4, device_cus())
    print(W.summary(g))
    assert g["nlarge"] == 2 and g["count"] == [0, 1, 0]                      # the chain's kernels and wselect_sort_kernel both take masses
    rng = np.random.default_rng(141)
    keys = {np.float32: with_ties(np.int32, n, rng), np.float64: with_ties(np.uint64, n, rng)}
    engines = {}
    answered = zero_total = all_saturated = 0
    for dtype, wexp, _, w in W.exponent_cases():
        x, desc = keys[dtype], dtype is np.float64
        ref = W.Referee(x, off, w, desc, wexp)
        tt = W.random_targets(ref.total, 4, rng)
        tt[:, 0] = np.maximum(ref.total // np.uint64(2), np.uint64(1))
        got = run(rsx, x, off, w, tt, False, desc, wexp, eng=engines.get(dtype))
        engines[dtype] = got[5]
        written = expect(got, ref(tt), what=f"{np.dtype(dtype).name} weight_exp={wexp}")
        m = W.mass_np(w, wexp)
        print(np.dtype(dtype).name, wexp, "totals", got[4].tolist(), "saturated", int((m == W.MASS_ONE).sum()), "of", int((w > 0).sum()), "positive")
        assert (written[:, 0] == (ref.total > 0)).all()
        answered += bool(written.any())
        zero_total += bool((got[4] == 0).any())
        all_saturated += bool((w > 0).any() and (m[w > 0] == W.MASS_ONE).all())
    assert answered >= 10 and zero_total >= 1 and all_saturated >= 1


# -- F. one engine across the layouts -------------------------------------------------------------------------------------------------------------

def test_one_engine_across_the_layouts(rsx):
    """One int32 engine with capacity for the largest layout runs the long segment, the class 0 stride layout, many_large and the small
    LENGTHS layout: its state, found, START / CONT and tie rows are laid out for one tile per group, then for two, then for one
    again, each time over what the call before left there."""
    cus = device_cus()
    cases = [shared(name, cus) for name in ("long", "stride0", "many_large", "lengths")]
    geo = [W.wselect_geometry(c.off, c.n, c.R, cus) for c in cases]
    for g in geo:
        print(W.summary(g))
    assert [g["gtiles"] for g in geo] == [1, 1, 2, 1] and geo[0]["max_segment_tiles"] > W.FIND_CHUNK and geo[1]["trips"][0] >= 2
    assert geo[2]["switches"] >= cus and geo[3]["nlarge"] >= 5 and geo[3]["nlarge"] * 4 < geo[2]["items"]
    eng = rsx.Engine(np.int32, max(c.n for c in cases))
    for name, c in zip(("long", "stride0", "many_large", "lengths"), cases):
        assert not c.descending and c.x.dtype == np.int32
        c.run(rsx, eng=eng, what=name)
    eng.sync()
