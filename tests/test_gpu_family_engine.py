"""One engine, every kind of call of the family, one wait.

rsx_segmented_compact scans its per-tile counts in the buffers (seg_table, seg_gsum, seg_gsum2, seg_temp[0]) that the segmented sort,
the top-k, the select and the unique use with other shapes and strides, and grows them, which waits for and frees what pending calls
still use.  Compact and search both keep their first-bad-segment word at seg_temp + 1, and every call of the family reports through
the engine's one mapped status word, stored only while it is zero.  The `one engine` tests of the older members predate both calls.

  test_compact_and_search_between_the_table_users   eleven calls enqueued through the Engine methods back to back, one eng.sync() at the
      end: each output equals its referee, and equals bit for bit what the same call gives on a fresh engine of its own
  test_status_word_across_kinds   a bad call among good ones of other kinds, and two bad calls of two kinds before one wait: one
      report, the first; the good calls are correct, the bad ones wrote nothing

Every call has its own inputs and outputs; the outputs start out holding the sentinel and end in a guard band.  The referees are those
of the members' own suites.
"""
import re

import numpy as np
import pytest

import _compact_ref as CR
import _topk_ref as TR
from _compact_ref import compact_oracle
from _reduce_ref import reduce_oracle
from _search_ref import search_oracle
from _select_ref import random_ranks, select_oracle
from test_gpu_compact import check as compact_check
from test_gpu_compact import random_mask
from test_gpu_reduce import KIND, OPCODE
from test_gpu_reduce import check as reduce_check
from test_gpu_scan import check as scan_check
from test_gpu_scan import ragged as scan_ragged
from test_gpu_search import check as search_check
from test_gpu_segmented import _torch, covered, dev, offsets_from, seg_oracle
from test_gpu_select import check as select_check
from test_gpu_topk_shapes import expect as topk_expect
from test_gpu_unique import FILL32, LENGTHS
from test_gpu_unique import check as unique_check
from test_gpu_unique_reduce_paths import Outputs
from test_search import drawn_counts, pooled_queries, ragged_case

pytestmark = pytest.mark.gpu

CAP = 1 << 18


class Call:
    """one call of the family: inputs on the device, the sizes and types of its outputs, how to enqueue it and how to judge what it wrote"""

    def __init__(self, t, what, ins, sizes, types, launch, verify):
        self.t, self.what, self.sizes, self.types, self.launch, self.verify = t, what, sizes, types, launch, verify
        self.ins = {name: dev(t, np.asarray(a)) for name, a in ins.items()}

    def outputs(self):
        return Outputs(self.t, self.sizes, self.types)

    def enqueue(self, eng, outs):
        self.launch(eng, {name: buf.data_ptr() for name, buf in self.ins.items()}, outs.ptr)


def sort_call(t, x, off, what):
    n, nseg = x.size, len(off) - 1

    def launch(eng, i, o):
        eng.segmented_sort(i["keys"], n, i["off"], nseg, o("keys"), i["payload"], o("payload"))

    def verify(got):
        want, inside = seg_oracle(x, off, n), covered(off, n)
        assert np.array_equal(got["keys"], np.where(inside, x[want], np.uint32(FILL32))), f"{what}: keys"
        assert np.array_equal(got["payload"], np.where(inside, want.astype(np.uint32), np.uint32(FILL32))), f"{what}: payload"

    return Call(t, what, dict(keys=x, off=off, payload=np.arange(n, dtype=np.uint32)), dict(keys=4 * n, payload=4 * n), dict(keys=np.uint32, payload=np.uint32),
                launch, verify)


def compact_call(t, x, off, what, mask=None, bounds=None, partition=False, want=("keys", "index")):
    n, nseg = x.size, len(off) - 1
    ins = dict(keys=x, off=off, **(dict(mask=mask) if mask is not None else dict(bounds=bounds)))
    sizes = {"koff": 8 * (nseg + 1), **{name: 4 * n for name in want}}

    def launch(eng, i, o):
        eng.segmented_compact(i["keys"], n, i["off"], nseg, i.get("mask"), i.get("bounds"), o("keys") if "keys" in want else None,
                              o("index") if "index" in want else None, o("koff"), partition=partition)

    def verify(got):
        compact_check(got, compact_oracle(x, off, mask=mask, bounds=bounds, partition=partition), what)

    return Call(t, what, ins, sizes, dict(koff=np.uint64, keys=np.uint32, index=np.uint32), launch, verify)


def select_call(t, x, off, ranks, what):
    n, nseg, R = x.size, len(off) - 1, ranks.shape[1]

    def launch(eng, i, o):
        eng.segmented_select(i["keys"], n, i["off"], nseg, i["ranks"], R, o("keys"), o("index"))

    def verify(got):
        select_check(x, off, ranks, got["keys"].reshape(nseg, R), got["index"].reshape(nseg, R), referee=select_oracle)

    return Call(t, what, dict(keys=x, off=off, ranks=np.ascontiguousarray(ranks, dtype=np.uint32)), dict(keys=4 * nseg * R, index=4 * nseg * R),
                dict(keys=np.uint32, index=np.uint32), launch, verify)


def topk_call(t, x, off, k, what):
    n, nseg = x.size, len(off) - 1

    def launch(eng, i, o):
        eng.segmented_topk(i["keys"], n, i["off"], nseg, k, o("keys"), o("index"))

    def verify(got):
        topk_expect(TR.fast_topk(x, off, k, False), k, got["keys"].reshape(nseg, k), got["index"].reshape(nseg, k), what)

    return Call(t, what, dict(keys=x, off=off), dict(keys=4 * nseg * k, index=4 * nseg * k), dict(keys=np.uint32, index=np.uint32), launch, verify)


def unique_call(t, x, off, what):
    n, nseg = x.size, len(off) - 1

    def launch(eng, i, o):
        eng.segmented_unique(i["keys"], n, i["off"], nseg, o("keys"), o("run_offsets"), o("counts"), None, None)

    return Call(t, what, dict(keys=x, off=off), dict(keys=4 * n, run_offsets=8 * (nseg + 1), counts=4 * n),
                dict(keys=np.uint32, run_offsets=np.uint64, counts=np.uint32), launch, lambda got: unique_check(x, off, got))


def search_call(t, keys, off, queries, qoff, what, right=False):
    n, nq, nseg = keys.size, queries.size, len(off) - 1

    def launch(eng, i, o):
        eng.segmented_search(i["keys"], n, i["off"], nseg, i["queries"], nq, i["qoff"], o("out"), right=right)

    return Call(t, what, dict(keys=keys, off=off, queries=queries, qoff=qoff), dict(out=4 * nq), dict(out=np.uint32), launch,
                lambda got: search_check(got["out"], search_oracle(keys, off, queries, qoff, right), what))


def reduce_call(t, x, v, off, what):
    n, nseg = x.size, len(off) - 1

    def launch(eng, i, o):
        eng.segmented_reduce_by_key(i["keys"], i["values"], n, i["off"], nseg, OPCODE["sum"], KIND[v.dtype], o("keys"), o("run_offsets"), o("values"), o("counts"))

    return Call(t, what, dict(keys=x, values=v, off=off), dict(keys=4 * n, run_offsets=8 * (nseg + 1), values=v.dtype.itemsize * n, counts=4 * n),
                dict(keys=np.uint32, run_offsets=np.uint64, values={4: np.uint32, 8: np.uint64}[v.dtype.itemsize], counts=np.uint32), launch,
                lambda got: reduce_check(x, v, off, got, "sum", ref=reduce_oracle(x, v, off, "sum")))


def scan_call(t, keys, v, off, what):
    n, nseg = v.size, len(off) - 1

    def launch(eng, i, o):
        eng.segmented_scan(i["keys"], i["values"], n, i["off"], nseg, OPCODE["sum"], KIND[v.dtype], o("out"))

    return Call(t, what, dict(keys=keys, values=v, off=off), dict(out=v.dtype.itemsize * n), dict(out={4: np.uint32, 8: np.uint64}[v.dtype.itemsize]), launch,
                lambda got: scan_check(got["out"], v, off, keys, "sum"))


def u32(rng, n, hi=1 << 32):
    return rng.integers(0, hi, n, dtype=np.uint32)


def test_compact_and_search_between_the_table_users(rsx):
    t = _torch()
    rng = np.random.default_rng(800)
    T = CR.TILE
    # 1, 11: three large segments, about 60 k keys
    off_sort = offsets_from([20000, 25011, 15000], start=3)
    n_sort = int(off_sort[-1]) + 5
    # 2: about 150 k ragged elements
    off_c = offsets_from(CR.LENGTHS * 3 + [10000], start=3)
    n_c = int(off_c[-1]) + 5
    # 3, 4: two large segments between small ones
    off_sel = offsets_from([300, 50000, 7, 0, 45001, 4096, 1], start=2)
    n_sel = int(off_sel[-1]) + 3
    x_sel = u32(rng, n_sel, 1 << 12)                                             # ties
    # 5: 2^21 elements: its table is larger than anything before it
    n_big = 1 << 21
    off_big = np.concatenate([[5], np.sort(rng.integers(5, n_big - 9, 200)), [n_big - 9]]).astype(np.uint64)
    before = [16 * TR.seg_shape(n, nseg)[1] for n, nseg in ((n_sort, 3), (n_sel, len(off_sel) - 1))] + [CR.grid(n_c)[1]]
    assert CR.grid(n_big)[1] == 528 > max(before) >= 16 * 18 and n_big > CAP                       # (entries of seg_table)
    # 6: a ragged shape; 7: ragged search; 8, 9: reduce and scan by key; 10: count only
    off_u = offsets_from(LENGTHS, start=3)
    n_u = int(off_u[-1]) + 5
    keys_s, off_s = ragged_case(np.uint32, rng)
    queries, qoff = pooled_queries(keys_s, off_s, rng, drawn_counts(rng, len(off_s) - 1))
    off_r = offsets_from(list(rng.integers(0, 40, 3000)), start=2)
    n_r = int(off_r[-1]) + 4
    n_scan, off_scan, keys_scan = scan_ragged(rng, np.uint32)
    x_c = u32(rng, n_c, 50)
    calls = [sort_call(t, u32(rng, n_sort), off_sort, "1 segmented sort"),
             compact_call(t, x_c, off_c, "2 compact, mask", mask=random_mask(n_c, rng)),
             select_call(t, x_sel, off_sel, random_ranks(off_sel, 3, rng), "3 select, R = 3"),
             topk_call(t, x_sel, off_sel, 64, "4 top-k"),
             compact_call(t, u32(rng, n_big, 1000), off_big, "5 compact, bound, partition, 2^21", bounds=u32(rng, len(off_big) - 1, 1000), partition=True),
             unique_call(t, u32(rng, n_u, 300), off_u, "6 unique with counts"),
             search_call(t, keys_s, off_s, queries, qoff, "7 search, ragged"),
             reduce_call(t, u32(rng, n_r, 5), rng.integers(-1 << 40, 1 << 40, n_r), off_r, "8 reduce by key"),
             scan_call(t, keys_scan, rng.integers(-1 << 30, 1 << 30, n_scan).astype(np.int32), off_scan, "9 scan by key"),
             compact_call(t, x_c, off_c, "10 compact, count only", bounds=u32(rng, len(off_c) - 1, 50), want=()),
             sort_call(t, u32(rng, n_sort, 1 << 10), off_sort, "11 segmented sort again")]
    assert all(c.ins["keys"].numel() <= CAP for i, c in enumerate(calls) if i not in (4, 6))        # (compact and search are not bound by the capacity)
    outs = [c.outputs() for c in calls]
    eng = rsx.Engine(np.uint32, CAP, payload=True)
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
        with rsx.Engine(np.uint32, CAP, payload=True) as fresh:
            c.enqueue(fresh, alone)
            fresh.sync()
        for name, a in alone.read().items():
            assert np.array_equal(a, g[name]), f"{c.what}: {name} differs from the same call on a fresh engine"


def bad_segment(rsx, eng):
    """the one report of the next wait: (status, the segment the message names)"""
    with pytest.raises(rsx.RadixSortError) as ei:
        eng.sync()
    named = re.search(r"segment (\d+)", str(ei.value))
    assert named, str(ei.value)
    return ei.value.status, int(named.group(1))


def test_status_word_across_kinds(rsx):
    t = _torch()
    rng = np.random.default_rng(810)
    n = 40000
    x = u32(rng, n, 99)
    good_off = np.array([0, 100, 5000, 5001, 30000, n], dtype=np.uint64)
    bad_at_2 = np.array([0, 100, 5000, 4000, 30000, n], dtype=np.uint64)
    bad_at_3 = np.array([0, 100, 5000, 5001, n + 1, n], dtype=np.uint64)
    keys_s, off_s = ragged_case(np.uint32, rng)
    queries, qoff = pooled_queries(keys_s, off_s, rng, drawn_counts(rng, len(off_s) - 1))
    bad_qoff = qoff.copy()
    bad_qoff[2] = queries.size + 1                                               # segment 1 ends past the queries
    mask = random_mask(n, rng)
    bad_compact = compact_call(t, x, bad_at_2, "compact, bad at segment 2", mask=mask)
    search = search_call(t, keys_s, off_s, queries, qoff, "search behind a bad compact", right=True)
    sort = sort_call(t, u32(rng, n), good_off, "segmented sort behind a bad compact")
    bad_search = search_call(t, keys_s, off_s, queries, bad_qoff, "search, bad at segment 1")
    bad_compact3 = compact_call(t, x, bad_at_3, "compact, bad at segment 3", bounds=u32(rng, 5, 99), partition=True)
    good_compact = compact_call(t, x, good_off, "compact after two bad calls", mask=mask, partition=True)

    def untouched(call, got):
        for name, a in got.items():
            want = 0 if name == "koff" else FILL32                               # (a bad compact zeroes its kept offsets; a bad search writes nothing)
            assert np.all(a == want), f"{call.what}: {name} written"

    with rsx.Engine(np.uint32, CAP, payload=True) as eng:
        # (i) one bad call among good ones of other kinds
        group = [bad_compact, search, sort]
        outs = [c.outputs() for c in group]
        t.cuda.synchronize()
        for c, o in zip(group, outs):
            c.enqueue(eng, o)
        assert bad_segment(rsx, eng) == (4, 2)
        eng.sync()                                                               # reported once
        got = [o.read() for o in outs]
        untouched(bad_compact, got[0])
        search.verify(got[1])
        sort.verify(got[2])
        # (ii) two bad calls of two kinds before one wait: one report, the first call's
        group = [bad_search, bad_compact3]
        outs = [c.outputs() for c in group]
        t.cuda.synchronize()
        for c, o in zip(group, outs):
            c.enqueue(eng, o)
        assert bad_segment(rsx, eng) == (4, 1)
        eng.sync()
        for c, o in zip(group, outs):
            untouched(c, o.read())
        out = good_compact.outputs()
        t.cuda.synchronize()
        good_compact.enqueue(eng, out)
        eng.sync()
        good_compact.verify(out.read())
