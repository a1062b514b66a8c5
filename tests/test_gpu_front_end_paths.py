"""GPU checks of the paths that the wrappers' shared argument handling (radix-sort_amd/_tensor_args.py) owns, small: every one of the
fourteen wrappers gives the same result on contiguous, 16-byte aligned tensors and on the same data presented the awkward way (keys one
element into a longer tensor or as a stride-2 view; offsets, values, payloads, masks, queries and edges as stride-2 views), and leaves
the awkward inputs as they were; merge, set_op and join take an empty side; and each of the three engine caches gets an engine for a side
stream.  37 keys in 3 segments, one of them empty; int32 and int64 keys, whose 4- and 8-byte elements are where alignment differs."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A_LENGTHS, B_LENGTHS = [20, 0, 17], [9, 5, 0]
FILLER = -7          # what lies between the elements of a stride-2 view: reading it would change a result


def _torch():
    return pytest.importorskip("torch")


def sorted_segments(rng, lengths, np_dtype, base):
    keys = base + rng.integers(0, 12, sum(lengths)).astype(np_dtype)          # a narrow range: runs of equal keys
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    for s in range(len(lengths)):
        keys[off[s]:off[s + 1]].sort()
    return keys, off


def host_inputs(np_dtype):
    """the data of one case as numpy arrays; the int64 keys need all eight bytes"""
    rng = np.random.default_rng(37)
    base = np_dtype(0) if np_dtype == np.int32 else np_dtype(1 << 40)
    ks, off = sorted_segments(rng, A_LENGTHS, np_dtype, base)
    b, boff = sorted_segments(rng, B_LENGTHS, np_dtype, base)
    n, nb, nseg = ks.size, b.size, len(A_LENGTHS)
    return dict(
        ks=ks, k=rng.permutation(ks), off=off, b=b, boff=boff,
        v=rng.integers(-50, 50, n).astype(np.int32), p=np.arange(n, dtype=np.int32) + 100, pb=np.arange(nb, dtype=np.int32) + 500,
        q=base + rng.integers(-1, 13, 12).astype(np_dtype), qoff=np.array([0, 5, 9, 12], dtype=np.int64),
        mask=rng.integers(0, 2, n).astype(np.uint8), edges=base + np.array([0, 3, 4, 9, 12], dtype=np_dtype),
        per_segment=np.array([7, 8, 9], dtype=np.int32), starts=np.array([3, 0, 10], dtype=np.int64),
        ranks=np.array([[0, 5], [0, 1], [16, 3]], dtype=np.int64)[:nseg])


def present(t, host, how):
    """(inputs, buffers): the tensors of a case on the device - how None: fresh allocations, contiguous and 16-byte aligned; else the
    awkward way, keys by `how` and everything else as stride-2 views - and the buffers behind the awkward views"""
    views, buffers = {}, []
    for name, arr in host.items():
        x = t.from_numpy(arr).cuda()
        if how is None or name == "ranks":
            assert x.is_contiguous() and x.data_ptr() % 16 == 0
        elif how == "one_element_in" and name in ("k", "ks", "b"):
            buf = t.full((x.numel() + 1,), FILLER, dtype=x.dtype, device="cuda")
            buf[1:] = x
            x = buf[1:]
            assert x.is_contiguous() and x.data_ptr() % 16 != 0 and x.data_ptr() % x.element_size() == 0
            buffers.append(buf)
        else:
            buf = t.full((2 * x.numel(),), FILLER % 2 if name == "mask" else FILLER, dtype=x.dtype, device="cuda")
            buf[::2] = x
            x = buf[::2]
            assert not x.is_contiguous() and x.stride() == (2,)
            buffers.append(buf)
        views[name] = x
    views["mask"] = views["mask"].view(t.bool) if how is None else views["mask"]          # (bool and uint8 masks are both accepted)
    return types.SimpleNamespace(**views), buffers


WRAPPERS = {
    "sort": lambda r, c: r.segmented_sort(c.k, c.off, c.p),
    "topk": lambda r, c: r.segmented_topk(c.k, c.off, 3),
    "select": lambda r, c: r.segmented_select(c.k, c.off, c.ranks),
    "unique": lambda r, c: r.segmented_unique(c.k, c.off, return_inverse=True, return_counts=True, return_first=True),
    "reduce_by_key": lambda r, c: r.segmented_reduce_by_key(c.k, c.v, c.off, return_counts=True),
    "scan": lambda r, c: (r.segmented_scan(c.v, c.off, keys=c.k), r.segmented_scan(c.v, None, op="max")),
    "segreduce": lambda r, c: r.segmented_reduce(c.v, c.off, op="max", return_index=True),
    "expand": lambda r, c: r.segmented_expand(c.off, c.per_segment, n=37, return_segment=True, return_rank=True)
    + (r.segmented_expand(c.off, c.v, n=37, starts=c.starts),),
    "search": lambda r, c: (r.segmented_searchsorted(c.ks, c.off, c.q, value_offsets=c.qoff), r.segmented_searchsorted(c.ks, c.off, c.q, right=True)),
    "compact": lambda r, c: r.segmented_compact(c.k, c.off, mask=c.mask, return_index=True) + r.segmented_compact(c.k, None, bound=c.q[:1]),
    "histogram": lambda r, c: (r.segmented_histogram(c.k, c.off, c.edges), r.segmented_histogram(c.k, None, c.edges)),
    "merge": lambda r, c: r.segmented_merge(c.ks, c.off, c.b, c.boff, payload_a=c.p, payload_b=c.pb, return_index=True),
    "set_op": lambda r, c: r.segmented_set_op(c.ks, c.off, c.b, c.boff, "union", payload_a=c.p, payload_b=c.pb, return_index=True)
    + r.segmented_set_op(c.ks, c.off, c.b, c.boff, "intersection", return_match=True),
    "join": lambda r, c: r.segmented_join(c.ks, c.off, c.b, c.boff, how="left", return_keys=True)
    + r.segmented_join(c.ks, c.off, c.b, c.boff, how="inner", capacity=64),
}
assert len(WRAPPERS) == 14


@pytest.mark.parametrize("how", ["one_element_in", "stride_2"])
@pytest.mark.parametrize("np_dtype", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("wrapper", list(WRAPPERS))
def test_awkward_inputs_give_the_same_result(rsx, wrapper, np_dtype, how):
    t = _torch()
    host = host_inputs(np_dtype)
    plain, _ = present(t, host, None)
    awkward, buffers = present(t, host, how)
    before = [buf.clone() for buf in buffers]
    want = WRAPPERS[wrapper](rsx, plain)
    got = WRAPPERS[wrapper](rsx, awkward)
    t.cuda.synchronize()
    assert len(got) == len(want) and len(want) >= 2
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), i
        if w is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and t.equal(g, w), (wrapper, i)
    assert any(w is not None and w.numel() > 0 and bool((w != 0).any()) for w in want)       # (the call did something)
    for buf, b in zip(buffers, before):
        assert t.equal(buf, b)                                                                # the inputs are left alone


def test_plain_inputs_pass_through_by_identity(rsx):
    """contiguous, aligned inputs are handed to the engine as they are: the helpers copy nothing"""
    t = _torch()
    mod = rsx._args
    x = t.arange(16, dtype=t.int32, device="cuda")
    off = t.tensor([0, 16], dtype=t.int64, device="cuda")
    assert mod.aligned_copy(x) is x and mod.as_offsets(off) is off and mod.as_offsets(None) is None and rsx._aligned_copy is mod.aligned_copy
    assert mod.aligned_copy(x[1:]).data_ptr() % 16 == 0 and t.equal(mod.aligned_copy(x[1:]), x[1:])
    inter = t.stack([off, off + 5], dim=1).reshape(-1)[::2]
    assert mod.as_offsets(inter).is_contiguous() and t.equal(mod.as_offsets(inter), off)
    assert mod.ptr(None) is None and mod.ptr(x) == x.data_ptr() and mod.ptr_nonempty(x[:0]) is None and mod.ptr_nonempty(x) == x.data_ptr()
    assert mod.device_and_stream(x) == (x.device.index, t.cuda.current_stream(x.device).cuda_stream)
    i32 = t.tensor([-1, 5, -2], dtype=t.int32, device="cuda")
    assert mod.widen(i32).tolist() == [0xFFFFFFFF, 5, 0xFFFFFFFE] and mod.widen_keeping_none(i32).tolist() == [-1, 5, 0xFFFFFFFE]
    assert mod.widen(None) is None and mod.widen_keeping_none(None) is None


@pytest.mark.parametrize("empty", ["a", "b"])
def test_two_sided_calls_take_an_empty_side(rsx, empty):
    """pointer-or-None for a side without elements; merge and set_op need a stand-in address for its payload"""
    t = _torch()
    full = t.tensor([1, 3, 3, 8], dtype=t.int32, device="cuda")
    pay = t.tensor([10, 11, 12, 13], dtype=t.int32, device="cuda")
    none, nopay = full[:0], pay[:0]
    a, pa, b, pb = (none, nopay, full, pay) if empty == "a" else (full, pay, none, nopay)
    off_full, off_none = t.tensor([0, 1, 4], dtype=t.int64, device="cuda"), t.zeros(3, dtype=t.int64, device="cuda")
    aoff, boff = (off_none, off_full) if empty == "a" else (off_full, off_none)
    place = t.arange(4, device="cuda") - off_full[:-1].repeat_interleave(off_full[1:] - off_full[:-1])      # position in its segment
    for offs in ((None, None), (aoff, boff)):
        seg_place = t.arange(4, device="cuda") if offs[0] is None else place
        keys, ooff, payload, index = rsx.segmented_merge(a, offs[0], b, offs[1], payload_a=pa, payload_b=pb, return_index=True)
        assert t.equal(keys, full) and t.equal(payload, pay) and t.equal(index, seg_place)
        assert ooff.tolist() == ([0, 4] if offs[0] is None else [0, 1, 4])
        keys, ooff, payload, index = rsx.segmented_set_op(a, offs[0], b, offs[1], "union", payload_a=pa, payload_b=pb, return_index=True)
        assert t.equal(keys, full) and t.equal(payload, pay) and t.equal(index, seg_place)
        keys, ooff, payload = rsx.segmented_set_op(a, offs[0], b, offs[1], "intersection", payload_a=pa, payload_b=pb)
        assert keys.numel() == 0 and payload.numel() == 0 and int(ooff[-1]) == 0
        keys, ooff = rsx.segmented_set_op(a, offs[0], b, offs[1], "difference")
        assert t.equal(keys, a)
        ia, ib, ooff = rsx.segmented_join(a, offs[0], b, offs[1], how="inner")
        assert ia.numel() == 0 and ib.numel() == 0 and int(ooff[-1]) == 0
        ia, ib, ooff, jk = rsx.segmented_join(a, offs[0], b, offs[1], how="left", return_keys=True, capacity=6)
        rows = a.numel()
        assert int(ooff[-1]) == rows and t.equal(jk[:rows], a) and ib.tolist() == [-1] * 6
        assert ia.tolist() == (seg_place.tolist() if rows else []) + [-1] * (6 - rows)


def test_each_engine_kind_follows_the_stream(rsx):
    """one call of every engine kind under a side stream: the stream shows up in the matching cache"""
    t = _torch()
    k = t.tensor([5, 1, 4, 1, 9, 2], dtype=t.int32, device="cuda")
    off = t.tensor([0, 3, 6], dtype=t.int64, device="cuda")
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(side):
        sk, _ = rsx.segmented_sort(k, off)
        run = rsx.segmented_scan(k, off)
        pos = rsx.segmented_searchsorted(sk, off, t.tensor([4, 2], dtype=t.int32, device="cuda"))
    side.synchronize()
    assert sk.tolist() == [1, 4, 5, 1, 2, 9] and run.tolist() == [5, 6, 10, 1, 10, 12] and pos.tolist() == [1, 1]
    for cache in (rsx._SEG_ENGINES, rsx._SCAN_ENGINES, rsx._SEARCH_ENGINES):
        assert side.cuda_stream in {key[1] for key in cache}
    assert all(key[2] in (4, 8) for key in rsx._SCAN_ENGINES) and all(e.capacity <= 4096 for e in rsx._SCAN_ENGINES.values())
    assert all(e.capacity <= 4096 for e in rsx._SEARCH_ENGINES.values())
