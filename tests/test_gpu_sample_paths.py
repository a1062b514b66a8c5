"""rsx_segmented_sample on the launch paths of rsx_sample.hpp and capi_sample.inc that tests/test_gpu_sample.py never reaches (every layout
there gives a workgroup of sample_tile_kernel one tile and a walk at most two chunks; tests/test_sample.py pins that):

  A  workgroups of sample_tile_kernel that walk two tiles: the tile loop, the `from` hint from one tile's search into the next, a tile
     outside [off[0], off[S]) in a workgroup's range, two block sums behind a tile already summed; and a walk of sample_draw_kernel over
     sixteen chunks, one of them without mass, from a tile that is no multiple of 4;
  B  the 256-element groups inside one piece: targets on every group's end and one above, a group without mass, a piece off the
     4-element grid, a partial last group, lanes whose four masses pass 2^32;
  C  totals at and above 2^53 on the device: rsx_mass::target_of where the double nearest the total lies above it, and below it;
  D  the draw grid's second trip with R = 3: long, two-tile, one-tile and empty segments whose slots all lie in it;
  E  the mass function of sample_mass_of at the ends of both exponent ranges, with weights of their own and as self-weights;
  F  one engine, one wait: samples between the other users of the per-tile partials buffer, growing it and running below its size, and
     a sample with bad offsets reported among good calls of other kinds.

The layouts are held in tests/_sample_ref.py (tests/test_sample.py checks on the CPU, at three CU counts, that each reaches its path);
every test here rebuilds its layout for the device's own CU count, prints the figures and asserts the path again before it compares.
Every comparison is exact integer equality with _sample_ref.Referee through run / check / Inputs of tests/test_gpu_sample.py: the
sentinel in every slot without an answer, guard bands around every output.  Every engine a test creates is closed by the test.
"""
import numpy as np
import pytest

import _sample_ref as R
import _segreduce_ref as SR
import _whistogram_ref as W
import _wselect_ref as WS
from _wselect_ref import kind_of, random_targets
from test_gpu_family_engine import Call, reduce_call, scan_call, u32
from test_gpu_sample import CAP, Inputs, check, random_keys, run
from test_gpu_scan import ragged as scan_ragged
from test_gpu_segmented import _torch
from test_gpu_segreduce import KIND as SEGREDUCE_KIND
from test_gpu_segreduce import check_exact as segreduce_check
from test_gpu_unique import FILL32, FILL64
from test_gpu_wselect_paths import device_cus

pytestmark = pytest.mark.gpu

T = R.TILE


def plant(tt, rows):
    for s, ts in rows.items():
        assert len(ts) <= tt.shape[1]
        tt[s, :len(ts)] = ts
    return tt


# -- A. two tiles per workgroup, sixteen walk chunks -------------------------------------------------------------------------------------------------------

TWO_TILE_R = 32
UPLOADS = ["float32", "float64-self-bound-descending", "uint32-int64-strict-skew1"]


def two_tile_inputs(which, n, off, names, rng):
    """(Inputs, engine dtype, descending, the call's keywords) of one of the three uploads, the bulk's second walk chunk weighing nothing"""
    nseg = len(off) - 1
    a, z = R.weightless_chunk(off, names["bulk"])
    if which == 0:
        w = W.large_case_weights(rng, np.float32, n, off, 0)
        w[a:z] = 0.0
        return Inputs(w, off), np.uint32, False, {}
    if which == 1:
        keys = W.large_case_weights(rng, np.float64, n, off, 0)                       # the keys are the weights
        keys[a:z] = 0.0
        return Inputs(None, off, keys=keys), np.float64, True, dict(bounds=np.full(nseg, 0.1, dtype=np.float64))
    w = W.case_weights(rng, np.uint32, n, off, 0)
    w[a:z] = 0
    keys = random_keys(rng, np.int64, n)
    return Inputs(w, off, keys=keys, skew=1), np.int64, False, dict(bounds=np.full(nseg, 20, dtype=np.int64), strict=True)


@pytest.mark.parametrize("which", range(3), ids=UPLOADS)
def test_two_tiles_per_workgroup_and_sixteen_walk_chunks(rsx, which):
    """R.two_tile_layout: every workgroup of sample_tile_kernel walks two tiles.  The first workgroup skips its first tile (outside) and
    sums a tail in its second; the second one sums a whole tile and then a lead and a tail of two other segments; two workgroups walk
    four tiles of 586 whole segments each, which nobody reads, `from` moving on through them; the last one's second tile lies behind
    off[S].  The bulk segment has 16 walk chunks at 256 CUs, begins in tile 13 and its second chunk weighs nothing: the prefix at that
    chunk's end is the one at its start, and prefix + 1 is answered behind it.  All 2356 segments against the referee."""
    cus = device_cus()
    n, off, names = R.two_tile_layout(cus)
    nseg = len(off) - 1
    o = off.astype(np.int64)
    rng = np.random.default_rng(600 + which)
    inp, edt, descending, kw = two_tile_inputs(which, n, off, names, rng)
    ref = R.Referee(inp.weights, off, keys=inp.keys, bounds=kw.get("bounds"), descending=descending, strict=kw.get("strict", False))
    walk = R.group_walk(n, off, cus)
    bulk = names["bulk"]
    f = R.walk_facts(ref.m, off, bulk)
    ta, tb = f["tiles"]
    print(f"cus {cus} n {n} tiles {(n + T - 1) // T} (chunk, grid) {R.tile_grid(n, cus)} segments {nseg} bulk tiles {ta}..{tb} walk chunks {f['chunks']} "
          f"draw (grid, slots) {R.draw_grid(nseg, TWO_TILE_R, cus)}")
    assert R.tile_grid(n, cus)[0] == 2 and walk[0] == ("outside", "tail") and walk[1] == ("both", "lead+tail") and walk[-1] == ("lead", "outside")
    assert walk[4] == walk[5] == (None, None) and f["chunks"] >= 3 and ta % 4 != 0 and tb % 2 == 0
    prefix = f["chunk_prefix"]
    assert prefix[1] == prefix[0] > 0 and prefix[2] > prefix[1] and not any(f["pieces"][R.WALK_TILES:2 * R.WALK_TILES])       # the weightless chunk
    planted = {bulk: R.chunk_targets(ref.m, off, bulk)}
    for name in ("to_edge", "from_edge"):
        assert ref.total[names[name]] > 0
        planted[names[name]] = [1, int(ref.total[names[name]])]
    tt = plant(random_targets(ref.total, TWO_TILE_R, rng), planted)
    eng = rsx.Engine(edt, CAP, descending=descending)
    got = run(rsx, eng, inp, tt, **kw)
    written = check(got, ref(tt), UPLOADS[which])
    for s, ts in planted.items():
        assert written[s, :len(ts)].all()
    index = got[0][bulk].astype(np.int64)
    for c in range(min(8, len(prefix))):                                          # columns 2 + 2c, 3 + 2c: the prefix at chunk c's end, and + 1
        end = (ta + (c + 1) * R.WALK_TILES) * T - o[bulk]
        behind = end + R.WALK_TILES * T if c == 0 else end                        # (prefix + 1 at the first chunk's end is answered behind the weightless one)
        assert index[2 + 2 * c] < end and index[3 + 2 * c] >= behind, (c, index[2 + 2 * c], index[3 + 2 * c], end)
    assert index[2] < (ta + R.WALK_TILES) * T - o[bulk] and index[4] == index[2] and index[5] == index[3] >= (ta + 2 * R.WALK_TILES) * T - o[bulk]
    short = slice(names["short"], names["before_bulk"])
    assert written[short].any() and np.array_equal(got[2][short], ref.total[short])                   # nothing leaked from the tiles nobody reads
    u = rng.random((nseg, TWO_TILE_R))
    check(run(rsx, eng, inp, u, fraction=True, **kw), ref(u, True), UPLOADS[which] + " fractions")
    eng.sync()
    eng.close()


# -- B. the groups inside one piece ----------------------------------------------------------------------------------------------------------------------

GROUP_R = 40


@pytest.mark.parametrize("wdt", [np.uint32, np.float32], ids=["uint32", "float32"])
def test_group_edges_inside_a_piece(rsx, wdt):
    """R.group_layout: step 3 of sample_draw_kernel with a target on every 256-element group's end of every piece and one above it.  The
    one-tile segment starts at T + 1001 (off the lanes' 4-element grid), has 11 whole groups and one of 184, its fourth group weighs
    nothing and the first element of its eighth; the two-tile segment's pieces have 3595 and 1001 elements.  uint32: six weights in ten
    are 2^32 - 1, so a lane's four masses pass 2^32."""
    n, off = R.group_layout()
    o = off.astype(np.int64)
    rng = np.random.default_rng(620 + (wdt == np.float32))
    w = W.case_weights(rng, wdt, n, off, 0)
    if wdt == np.uint32:
        w[rng.random(n) < 0.6] = 0xFFFFFFFF
    a = int(o[R.GROUP_ONE_TILE])
    w[a + 3 * R.GROUP:a + 4 * R.GROUP] = 0
    w[a + 7 * R.GROUP] = 0
    ref = R.Referee(w, off)
    edges = {s: R.group_edges(ref.m, off, s) for s in (R.GROUP_TWO_TILES, R.GROUP_ONE_TILE)}
    planted = {s: R.group_targets(ref.m, off, s) for s in edges}
    print(f"n {n} pieces {[R.walk_facts(ref.m, off, s)['pieces'] for s in (0, 1)]} boundaries {[len(e) for e in edges.values()]} "
          f"targets {[len(p) for p in planted.values()]}")
    assert a % 4 and int(o[0]) % 4 and [e for e, _ in edges[R.GROUP_ONE_TILE]][-2:] == [11 * R.GROUP, 3000]
    assert edges[R.GROUP_ONE_TILE][2][1] == edges[R.GROUP_ONE_TILE][3][1] > 0 and ref.m[a + 7 * R.GROUP] == 0                    # the group without mass
    assert wdt != np.uint32 or int(ref.m[a:a + 3000].reshape(-1, 4).sum(1).max()) > 1 << 32          # (a lane's four elements, from the piece's start)
    tt = plant(random_targets(ref.total, GROUP_R, rng), planted)
    eng = rsx.Engine(np.uint32, CAP)
    got = run(rsx, eng, Inputs(w, off), tt)
    written = check(got, ref(tt), "group edges")
    for s, ts in planted.items():
        assert written[s, :len(ts)].all()
        total = int(ref.total[s])
        index = {int(t): int(i) for t, i in zip(tt[s, :len(ts)], got[0][s, :len(ts)])}
        for edge, p in edges[s]:                                                 # `prefix` is answered before the boundary, prefix + 1 at or behind it
            assert p < 1 or index[p] < edge, (s, edge, p, index[p])
            assert p + 1 > total or index[p + 1] >= edge, (s, edge, p)
    eng.sync()
    eng.close()


# -- C. totals at and above 2^53 -------------------------------------------------------------------------------------------------------------------------

def test_totals_above_2_to_53(rsx):
    """R.huge_total_layout with uint32 weights of 2^32 - 1, then 2^32 - 3: both totals pass 2^53; the double nearest the first lies one
    above it, the one nearest the second one below it, the two cases rsx_mass::target_of argues about.  1028 tiles: five walk chunks."""
    n, off = R.huge_total_layout()
    rng = np.random.default_rng(630)
    eng = rsx.Engine(np.uint32, CAP)
    a, z = int(off[0]), int(off[1])
    for word, slip in ((0xFFFFFFFF, 1), (0xFFFFFFFD, -1)):
        w = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)          # (outside the segment: anything)
        w[a:z] = word
        ref = R.Referee(w, off)
        total = int(ref.total[0])
        f = R.walk_facts(ref.m, off, 0)
        print(f"n {n} tiles {len(f['pieces'])} walk chunks {f['chunks']} total {total} = 2^53 + {total - (1 << 53)}, double(total) - total = {int(float(total)) - total}")
        assert total == (z - a) * word >= 1 << 53 and int(float(total)) - total == slip and f["chunks"] == 5 and R.tile_grid(n, device_cus())[0] == 1
        inp = Inputs(w, off)
        u = np.array([0.0, 5e-324, 1 / float(total), np.nextafter(1 / float(total), 1), 0.5, 1 / 3, 0.75, np.nextafter(1, 0), 1.0, np.nextafter(1, 2),
                      np.inf, -1.0, np.nan] + rng.random(16).tolist())
        want = ref(u, True)
        assert want[2][0, :12].all() and not want[2][0, 12]                        # every fraction but the NaN has an answer
        check(run(rsx, eng, inp, u, fraction=True), want, f"fractions of {total}")
        tt = np.array([1, 1 << 53, (1 << 53) + 1, total - 1, total, total + 1], dtype=np.uint64)
        want = ref(tt)
        assert want[2][0].tolist() == [True] * 5 + [False] and int(want[1][0, 2]) >= (1 << 53) + 1
        check(run(rsx, eng, inp, tt), want, f"targets of {total}")
    eng.sync()
    eng.close()


# -- D. the draw grid's second trip ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weightless", ["second_chunk", "first_chunk"])
def test_second_trip_of_the_draw_grid(rsx, weightless):
    """R.second_trip_layout: 48 cus segments drawn 3 times on a grid of 32 cus workgroups of 4 waves; the slots of the last 5 cus segments
    belong to the second trip, s = slot / 3 and q = slot - 3 s behind the trip's edge, and among them lie a segment of 300 tiles (the
    long path: two walk chunks), one of two tiles, one inside a tile and an empty one.  second_chunk: the 300-tile segment's second walk
    chunk weighs nothing (its total is its first chunk's prefix: prefix + 1 has no answer and keeps the sentinel); first_chunk: its
    first one does, so every answer is found in the second chunk."""
    cus = device_cus()
    n, off, names = R.second_trip_layout(cus)
    nseg, Rr = len(off) - 1, R.SECOND_TRIP_R
    o = off.astype(np.int64)
    rng = np.random.default_rng(640)
    w = W.case_weights(rng, np.float32, n, off, 0)
    long_s = names["long"]
    a, z = R.weightless_chunk(off, long_s)
    if weightless == "first_chunk":
        a, z = int(o[long_s]), a
    w[a:z] = 0.0
    ref = R.Referee(w, off)
    grid, slots = R.draw_grid(nseg, Rr, cus)
    f = R.walk_facts(ref.m, off, long_s)
    print(f"cus {cus} n {n} segments {nseg} slots {slots} draw grid {grid} first slot of the second trip {R.WAVES * grid} planted {names} "
          f"long: tiles {f['tiles']} chunks {f['chunks']} chunk masses {f['chunk_prefix'][0]}, {sum(f['pieces']) - f['chunk_prefix'][0]}")
    assert slots > R.WAVES * grid and all(s * Rr >= R.WAVES * grid for s in names.values()) and f["chunks"] == 2 and Rr > 1
    assert (f["chunk_prefix"][0] == 0) == (weightless == "first_chunk") and (sum(f["pieces"]) == f["chunk_prefix"][0]) == (weightless == "second_chunk")
    two = R.walk_facts(ref.m, off, names["two_tiles"])
    assert len(two["pieces"]) == 2 and min(two["pieces"]) > 0 and ref.total[names["empty"]] == 0
    total = {name: int(ref.total[s]) for name, s in names.items()}
    tt = plant(random_targets(ref.total, Rr, rng), {long_s: [1, total["long"], f["chunk_prefix"][0] + 1],
                                                    names["two_tiles"]: [1, total["two_tiles"], two["pieces"][0] + 1],
                                                    names["one_tile"]: [1, total["one_tile"], total["one_tile"] // 2]})
    eng = rsx.Engine(np.uint32, CAP)
    inp = Inputs(w, off)
    got = run(rsx, eng, inp, tt)
    written = check(got, ref(tt), "second trip")                                 # every total, and the sentinel in every slot without an answer
    assert written[long_s].tolist() == [True, True, weightless == "first_chunk"] and written[names["two_tiles"]].all() and written[names["one_tile"]].all()
    assert not written[names["empty"]].any() and np.all(got[0][names["empty"]] == FILL32) and got[2][names["empty"]] == 0
    second = slice(-(-R.WAVES * grid // Rr), nseg)
    assert written[second].any() and (~written[second]).any()
    split = (int(o[long_s]) // T + R.WALK_TILES) * T - int(o[long_s])
    if weightless == "first_chunk":
        assert got[0][long_s].min() >= split                                     # found in the second chunk
    else:
        assert got[0][long_s, 1] < split
    assert got[0][names["two_tiles"], 1] >= T - int(o[names["two_tiles"]]) % T > got[0][names["two_tiles"], 0]
    u = rng.random((nseg, Rr))
    check(run(rsx, eng, inp, u, fraction=True), ref(u, True), "second trip, fractions")
    eng.sync()
    eng.close()


# -- E. weight exponents ---------------------------------------------------------------------------------------------------------------------------------

def test_weight_exponents_on_the_device(rsx):
    """_wselect_ref.exponent_cases (segments of 300, 5000 and 20000 weights, weight_exp from -2048 to 2048, denormals, infinities and NaNs
    planted) through sample_mass_of: with weights of their own on an integer engine, and as self-weights on an engine of the weights'
    type, absolute targets and fractions.  At every exponent the masses hold 0 and 2^31 (a planted +inf), and a value strictly between
    wherever the type has a finite weight in [2^(weight_exp - 31), 2^weight_exp)."""
    engines = {None: rsx.Engine(np.uint32, CAP), np.float32: rsx.Engine(np.float32, CAP), np.float64: rsx.Engine(np.float64, CAP)}
    rng = np.random.default_rng(650)
    between = {np.float32: (-148, 127 + 31), np.float64: (-1073, 1023 + 31)}       # above the smallest denormal; 2^(weight_exp - 31) still finite
    cases = 0
    for dtype, wexp, off, w in WS.exponent_cases():
        m = WS.mass_np(w, wexp)
        mid = bool(((m > 0) & (m < WS.MASS_ONE)).any())
        print(np.dtype(dtype).name, "weight_exp", wexp, "masses: zero", int((m == 0).sum()), "between", int(((m > 0) & (m < WS.MASS_ONE)).sum()),
              "saturated", int((m == WS.MASS_ONE).sum()))
        assert (m == 0).any() and (m == WS.MASS_ONE).any() and int(m.max()) == WS.MASS_ONE
        assert mid or not between[dtype][0] <= wexp <= between[dtype][1]
        for own in (True, False):
            inp = Inputs(w, off) if own else Inputs(None, off, keys=w)
            ref = R.Referee(w if own else None, off, keys=None if own else w, weight_exp=wexp)
            assert np.array_equal(ref.m, m.astype(np.int64))
            eng = engines[None if own else dtype]
            tt = random_targets(ref.total, 4, rng)
            tt[:, 0] = np.maximum(ref.total // np.uint64(2), np.uint64(1))
            what = f"{np.dtype(dtype).name} weight_exp={wexp} {'weights' if own else 'self-weights'}"
            written = check(run(rsx, eng, inp, tt, weight_exp=wexp), ref(tt), what)
            assert (written[:, 0] == (ref.total > 0)).all()
            u = rng.random((len(off) - 1, 4))
            u[:, 0] = 1.0
            check(run(rsx, eng, inp, u, fraction=True, weight_exp=wexp), ref(u, True), what + " fractions")
        cases += 1
    assert cases == 2 * len(WS.WEIGHT_EXPS)
    for eng in engines.values():
        eng.sync()
        eng.close()


# -- F. one engine, one wait -----------------------------------------------------------------------------------------------------------------------------

FAMILY_CAP = 1 << 18


def sample_call(t, w, off, tt, what, fraction=False):
    n, nseg = w.size, len(off) - 1
    tt = np.ascontiguousarray(np.asarray(tt, dtype=np.float64 if fraction else np.uint64).reshape(nseg, -1))
    Rr = tt.shape[1]

    def launch(eng, i, o):
        eng.segmented_sample(None, i["weights"], n, i["off"], nseg, None, i["targets"], Rr, 128 if fraction else 0, kind_of(w), 0, o("index"), o("mass"), o("total"))

    def verify(got):
        check((got["index"].reshape(nseg, Rr), got["mass"].reshape(nseg, Rr), got["total"]), R.Referee(w, off)(tt, fraction), what)

    return Call(t, what, dict(weights=w, off=off, targets=tt), dict(index=4 * nseg * Rr, mass=8 * nseg * Rr, total=8 * nseg),
                dict(index=np.uint32, mass=np.uint64, total=np.uint64), launch, verify)


def whist_call(t, keys, w, off, B, what, signed=True):
    n, nseg = keys.size, len(off) - 1

    def launch(eng, i, o):
        eng.segmented_weighted_histogram(i["keys"], i["weights"], n, i["off"], nseg, B, o("sums"), kind_of(w), 0, W.WHIST_SIGNED if signed else 0)

    def verify(got):
        want = W.whistogram_oracle(keys, w, off, B, signed=signed)
        assert np.array_equal(got["sums"].reshape(nseg, B), want), f"{what}: sums differ"

    return Call(t, what, dict(keys=keys, weights=w, off=off), dict(sums=8 * nseg * B), dict(sums=np.int64), launch, verify)


def segreduce_call(t, v, off, what):
    n, nseg = v.size, len(off) - 1

    def launch(eng, i, o):
        eng.segmented_reduce(i["values"], n, i["off"], nseg, SR.OPCODE["sum"], SEGREDUCE_KIND[v.dtype], o("values"), None)

    return Call(t, what, dict(values=v, off=off), dict(values=8 * nseg), dict(values=np.uint64), launch,
                lambda got: segreduce_check(got["values"], None, v, off, "sum"))


def partials(n, per_tile, tile=T):
    """64-bit words of the per-tile partials buffer that a call over n elements asks for"""
    return per_tile * ((n + tile - 1) // tile) + 2


def test_samples_between_the_other_users_of_the_partials(rsx):
    """Eight calls enqueued back to back on one engine, one eng.sync() at the end.  The samples' lead / tail sums live in the buffer of
    the segmented reduction, the scan and the reduction by key, each with another layout and element type: the segmented reduction
    grows it behind a pending small sample, the long-layout sample grows it again, and the small sample after the scan and the
    reduction by key runs over their partials.  Each output equals its referee, and bit for bit the same call on a fresh engine."""
    t = _torch()
    rng = np.random.default_rng(660)
    n_in, off_in = R.inner_layout()
    n_long, off_long = R.long_layout()
    off_sr = SR.offsets_from([5, 30000, 0, 4096, 50000, 17, 15000], start=3)
    n_sr = int(off_sr[-1]) + 9
    print(f"partials asked for: sample (inner) {partials(n_in, 4)}, segmented reduce {partials(n_sr, 4, SR.TILE)}, sample (long) {partials(n_long, 4)}")
    assert partials(n_in, 4) < partials(n_sr, 4, SR.TILE) < partials(n_long, 4)                      # grows, grows again, then runs below the size
    n_scan, off_scan, keys_scan = scan_ragged(rng, np.uint32)
    off_r = SR.offsets_from(list(rng.integers(0, 40, 3000)), start=2)
    n_r = int(off_r[-1]) + 4
    n_h, off_h = R.crossing_layout()

    def sample(layout, what, Rr, fraction=False):
        n, off = layout
        w = W.case_weights(rng, np.float32 if fraction else np.uint32, n, off, 0)
        total = R.Referee(w, off).total
        tt = rng.random((len(off) - 1, Rr)) if fraction else random_targets(total, Rr, rng)
        return sample_call(t, w, off, tt, what, fraction)

    calls = [sample((n_in, off_in), "1 sample, inner", 5),
             segreduce_call(t, rng.integers(-1 << 40, 1 << 40, n_sr), off_sr, "2 segmented reduce"),
             sample((n_long, off_long), "3 sample, long", 8),
             scan_call(t, keys_scan, rng.integers(-1 << 30, 1 << 30, n_scan).astype(np.int32), off_scan, "4 scan by key"),
             reduce_call(t, u32(rng, n_r, 5), rng.integers(-1 << 40, 1 << 40, n_r), off_r, "5 reduce by key"),
             sample((n_in, off_in), "6 sample, inner, over stale partials", 5, fraction=True),
             whist_call(t, u32(rng, n_h, 70), W.case_weights(rng, np.float32, n_h, off_h, 0), off_h, 64, "7 weighted histogram"),
             sample((n_h, off_h), "8 sample, crossing", 3)]
    outs = [c.outputs() for c in calls]
    eng = rsx.Engine(np.uint32, FAMILY_CAP, payload=True)
    t.cuda.synchronize()                                                         # uploads and fills have landed; from here on nothing waits
    for c, o in zip(calls, outs):
        c.enqueue(eng, o)
    eng.sync()
    got = [o.read() for o in outs]
    eng.close()
    for c, g in zip(calls, got):
        c.verify(g)
    for c, g in zip(calls, got):                                                 # the same call on an engine of its own
        alone = c.outputs()
        with rsx.Engine(np.uint32, FAMILY_CAP, payload=True) as fresh:
            c.enqueue(fresh, alone)
            fresh.sync()
        for name, a in alone.read().items():
            assert np.array_equal(a, g[name]), f"{c.what}: {name} differs from the same call on a fresh engine"


def test_bad_sample_among_good_calls_of_other_kinds(rsx):
    """a good scan, a sample whose segment 2 ends before it begins, a good weighted histogram, a good sample, one wait: one report, the
    sample's; it wrote nothing, the good calls are right, and a second wait is silent"""
    t = _torch()
    rng = np.random.default_rng(670)
    n = 40000
    w = W.case_weights(rng, np.float32, n, None, 0)
    good_off = np.array([0, 100, 5000, 5001, n], dtype=np.uint64)
    bad_off = np.array([0, 100, 5000, 4000, n], dtype=np.uint64)
    n_scan, off_scan, keys_scan = scan_ragged(rng, np.uint32)
    tt = random_targets(R.Referee(w, good_off).total, 2, rng)
    bad = sample_call(t, w, bad_off, np.ones((4, 2), dtype=np.uint64), "sample, bad at segment 2")
    group = [scan_call(t, keys_scan, rng.integers(-1 << 30, 1 << 30, n_scan).astype(np.int32), off_scan, "scan before a bad sample"), bad,
             whist_call(t, u32(rng, n, 70), w, good_off, 64, "weighted histogram behind a bad sample"),
             sample_call(t, w, good_off, tt, "sample behind a bad sample")]
    outs = [c.outputs() for c in group]
    eng = rsx.Engine(np.uint32, FAMILY_CAP, payload=True)
    t.cuda.synchronize()
    for c, o in zip(group, outs):
        c.enqueue(eng, o)
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    assert ei.value.status == 4 and "rsx_segmented_sample" in str(ei.value) and "segment 2 " in str(ei.value)
    eng.sync()                                                                   # reported once
    got = [o.read() for o in outs]
    eng.close()
    assert np.all(got[1]["index"] == FILL32) and np.all(got[1]["mass"] == FILL64) and np.all(got[1]["total"] == FILL64)
    for i in (0, 2, 3):
        group[i].verify(got[i])
