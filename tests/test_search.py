"""CPU checks of the search in sorted segments: header, exports, binding and the Python callables agree on rsx_segmented_search; the two
forms of the host referee (tests/_search_ref.py) agree with each other and with a hand-made case; the layouts whose workgroups walk two
tiles of queries hold the (path, segment) transitions they are named for; and the call and the torch helpers fail
loudly instead of working on the CPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import _search_ref as R
from _search_ref import extremes, neighbours, order_map, order_unmap, search_count, search_oracle, sort_engine_order

HEADER_DTYPES = [np.uint32, np.int32, np.uint64, np.int64, np.float32, np.float64]
# the issue's haystack lengths (thread, vector and tile edges, empty segments, a long one) and query counts per segment
LENGTHS = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 9000, 0, 3, 20011]
QCOUNTS = [0, 1, 3, 255, 256, 257, 1024, 1025, 5000]


def header_text():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "radixsort_hip.h")).read()


def random_keys(dt, n, rng, narrow=False):
    """keys of the whole range of the type (floats: normals of every magnitude, subnormals, some specials), or of a narrow one (duplicates)"""
    dt = np.dtype(dt)
    if narrow:
        return rng.integers(0, 40, n).astype(dt) if dt.kind == "u" else (rng.integers(-20, 20, n).astype(dt) / (2 if dt.kind == "f" else 1)).astype(dt)
    if dt.kind == "f":
        u = R.UINT[dt.itemsize]
        x = rng.integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True).view(dt)       # every bit pattern: NaNs of both signs, infinities, subnormals
        pick = rng.integers(0, 8, n)
        x = np.where(pick < 5, (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(dt), x)
        sp = extremes(dt)
        return np.where(pick == 7, sp[rng.integers(0, sp.size, n)], x).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def ragged_case(dt, rng, descending=False, lengths=LENGTHS, start=3, tail=5):
    """(keys, off): segments of the given lengths sorted in the engine's order, every other one from a narrow range (runs of equal keys);
    off[0] = start, `tail` keys after off[S]; the keys outside the segments are random, so reading one would change an answer"""
    off = np.concatenate([[start], start + np.cumsum(lengths)]).astype(np.uint64)
    n = int(off[-1]) + tail
    keys = random_keys(dt, n, rng)
    for s, L in enumerate(lengths):
        a = int(off[s])
        keys[a:a + L] = sort_engine_order(random_keys(dt, L, rng, narrow=s % 2 == 1), descending)
    return keys, off


def query_pool(keys, off, s, rng, absent=64):
    """what segment s is asked: every key of it, each key's neighbours in the order, the type's extremes and random values"""
    seg = keys[int(off[s]):int(off[s + 1])]
    return np.concatenate([neighbours(seg), extremes(keys.dtype), random_keys(keys.dtype, absent, rng)])


def pooled_queries(keys, off, rng, counts=None):
    """(queries, qoff): per segment the whole pool, or counts[s] draws from it; qoff[0] = 2 and 3 unsearched queries at the end"""
    parts = []
    for s in range(len(off) - 1):
        pool = query_pool(keys, off, s, rng)
        parts.append(pool if counts is None else pool[rng.integers(0, pool.size, counts[s])])
    qoff = np.concatenate([[2], 2 + np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return np.concatenate([random_keys(keys.dtype, 2, rng)] + parts + [random_keys(keys.dtype, 3, rng)]).astype(keys.dtype), qoff


def drawn_counts(rng, nseg):
    """query counts per segment from QCOUNTS, every one of them at least once"""
    reps = (QCOUNTS * (nseg // len(QCOUNTS) + 1))[:max(nseg, len(QCOUNTS))]
    return [int(c) for c in rng.permutation(reps)[:nseg]] if nseg >= len(QCOUNTS) else [int(c) for c in rng.choice(QCOUNTS, nseg)]


def test_symbol_in_header_exports_and_binding(rsx):
    raw = header_text()
    assert re.search(r"#define\s+RSX_SEARCH_RIGHT\s+4\b", raw)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = re.search(r"int\s+rsx_segmented_search\s*\(([^)]*)\)\s*;", text)
    assert decl, "rsx_segmented_search is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_sorted", "uint64_t n", "const uint64_t* d_offsets", "uint64_t num_segments",
                      "const void* d_queries", "uint64_t num_queries", "const uint64_t* d_query_offsets", "uint32_t flags", "uint32_t* d_index_out"]
    assert "rsx_segmented_search" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_search
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_search\b", out)
    for name in ("segmented_searchsorted", "searchsorted", "bucketize"):
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_search)
    assert rsx.SEARCH_RIGHT == 4 and rsx.SEARCH_RIGHT & (rsx.UNIQUE_CONSECUTIVE | rsx.SCAN_EXCLUSIVE) == 0
    assert rsx.UNIQUE_CONSECUTIVE == 1 and rsx.SCAN_EXCLUSIVE == 2


def test_symbol_grid_constants_match_the_kernel_header():
    """tests/_search_ref.py states the kernel's grid; the numbers are those of rsx_search.hpp"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "radix-sort_amd", "csrc", "rsx_search.hpp")).read()
    num = lambda name: int(re.search(name + r"\s*=\s*(\d+)", src).group(1))
    assert (num("kSearchThreads"), 1 << num("kSearchTileShift"), num("kSearchSamples")) == (R.THREADS, R.TILE_Q, R.SAMPLES)
    assert (num("kSearchResidentPay"), num("kSearchSampledPay"), 1 << num("kSearchSampleShift")) == (R.RESIDENT_PAY, R.SAMPLED_PAY, R.SAMPLES)
    assert re.search(r"kSearchResidentMax\s*=\s*kSegTileKeys", src) and R.RESIDENT_MAX == 4096
    p = R.sample_positions(1024 * 1025 - 1)
    assert p[0] == 0 and p[1] == 1024 and p[-1] == 1023 * 1025 - 1 and R.sample_positions(4097)[-1] == 4092 and np.all(np.diff(R.sample_positions(4097).astype(np.int64)) >= 4)


def test_order_map_is_total_order():
    for dt in (np.float32, np.float64):
        x = np.array([-np.nan, -np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], dtype=dt)
        x[0] = np.copysign(np.nan, -1)
        y = order_map(x)
        assert np.all(y[1:] > y[:-1]) and np.all(order_map(x, True)[1:] < order_map(x, True)[:-1])
        assert np.array_equal(order_unmap(y, dt).view(y.dtype), x.view(y.dtype))
    for dt in (np.int32, np.int64, np.uint32, np.uint64):
        info = np.iinfo(dt)
        x = np.array([info.min, info.min + 1, 0 if info.min < 0 else 5, info.max - 1, info.max], dtype=dt)
        assert np.all(np.diff(order_map(x).astype(object)) > 0) and np.array_equal(order_unmap(order_map(x), dt), x)


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dt", HEADER_DTYPES, ids=lambda d: np.dtype(d).name)
def test_referee_forms_agree(dt, descending):
    rng = np.random.default_rng(HEADER_DTYPES.index(dt) * 2 + int(descending))
    lengths = LENGTHS
    keys, off = ragged_case(dt, rng, descending, lengths)
    queries, qoff = pooled_queries(keys, off, rng, drawn_counts(rng, len(lengths)))
    even = queries[:len(lengths) * 40]
    for right in (False, True):
        a, b = search_oracle(keys, off, queries, qoff, right, descending), search_count(keys, off, queries, qoff, right, descending)
        assert np.array_equal(a, b)
        assert np.all(a[:2] == -1) and np.all(a[-3:] == -1) and np.all(a[2:-3] >= 0)
        lens = np.repeat(np.diff(off.astype(np.int64)), np.diff(qoff.astype(np.int64)))
        assert np.all(a[2:-3] <= lens)
        assert np.array_equal(search_oracle(keys, off, even, None, right, descending), search_count(keys, off, even, None, right, descending))
        one = sort_engine_order(keys, descending)
        some = queries[::16]                                                     # (the brute force is quadratic)
        assert np.array_equal(search_oracle(one, None, some, None, right, descending), search_count(one, None, some, None, right, descending))
    lo, hi = search_oracle(keys, off, queries, qoff, False, descending), search_oracle(keys, off, queries, qoff, True, descending)
    assert np.all(lo <= hi) and np.any(hi - lo > 1)                              # runs of equal keys are met


def test_hand_made_example():
    """off[0] = 1, an empty haystack segment with queries, a run of equal keys across a segment boundary, a query segment that is empty"""
    keys = np.array([9, 2, 5, 5, 5, 5, 7, 1], dtype=np.uint32)
    off = np.array([1, 4, 4, 7], dtype=np.uint64)                                # [2 5 5] [] [5 5 7]
    queries = np.array([5, 0, 2, 6, 9, 5, 9, 5, 7, 8, 3], dtype=np.uint32)
    qoff = np.array([1, 5, 7, 10], dtype=np.uint64)                              # 0 2 6 9 | 5 9 | 5 7 8
    for form in (search_oracle, search_count):
        assert form(keys, off, queries, qoff).tolist() == [-1, 0, 0, 3, 3, 0, 0, 0, 2, 3, -1]
        assert form(keys, off, queries, qoff, right=True).tolist() == [-1, 0, 1, 3, 3, 0, 0, 2, 3, 3, -1]
        # the even form: 3 queries per segment
        assert form(keys, off, queries[:9], None).tolist() == [1, 0, 0, 0, 0, 0, 3, 0, 2]
        # one segment
        k = np.array([1, 3, 3, 8], dtype=np.int64)
        assert form(k, None, np.array([-5, 3, 4, 8, 9], dtype=np.int64), None).tolist() == [0, 1, 3, 3, 4]
        assert form(k, None, np.array([-5, 3, 4, 8, 9], dtype=np.int64), None, right=True).tolist() == [0, 3, 3, 4, 4]
        # descending: "before" is larger
        d = np.array([8, 3, 3, 1], dtype=np.int32)
        assert form(d, None, np.array([9, 8, 3, 2, 0], dtype=np.int32), None, descending=True).tolist() == [0, 0, 1, 3, 4]
        assert form(d, None, np.array([9, 8, 3, 2, 0], dtype=np.int32), None, True, True).tolist() == [0, 1, 3, 3, 4]
        # floats in totalOrder: -NaN -inf -0.0 +0.0 +inf +NaN; equal means equal by bits
        for dt in (np.float32, np.float64):
            f = np.array([np.nan, -np.inf, -0.0, 0.0, np.inf, np.nan], dtype=dt)
            f[0] = np.copysign(np.nan, -1)
            assert form(f, None, f, None).tolist() == [0, 1, 2, 3, 4, 5]
            assert form(f, None, f, None, right=True).tolist() == [1, 2, 3, 4, 5, 6]
            assert form(f[::-1].copy(), None, f, None, descending=True).tolist() == [5, 4, 3, 2, 1, 0]
            assert form(f, None, np.array([-1.0, 1.0], dtype=dt), None).tolist() == [2, 4]
        # an empty haystack: every result is 0
        assert form(np.zeros(0, dtype=np.uint64), None, np.array([0, 7], dtype=np.uint64), None, right=True).tolist() == [0, 0]


def test_tile_paths_of_the_referee():
    paths = R.tile_paths(10000, None, 3000, None)
    assert paths == ["sampled", "sampled", "sampled"] and R.tile_paths(10000, None, 3000, None, sampled=False) == ["direct"] * 3
    assert R.tile_paths(10000, None, 1024 + 255, None) == ["sampled", "direct"]
    assert R.tile_paths(4096, None, 1024 + 255, None) == ["resident", "direct"] and R.tile_paths(4080, None, 1024 + 255, None) == ["resident", "resident"]
    off = np.array([0, 4096, 8192], dtype=np.uint64)
    assert R.tile_paths(8192, off, 2048, None) == ["resident", "resident"] and R.tile_paths(8192, off, 32, None) == ["direct"]
    assert R.tile_paths(8192, off, 3000, np.array([1024, 2000, 2400], dtype=np.uint64)) == [None, "direct", "resident"]


def test_tile_walk_of_the_referee():
    """per workgroup the (path, staged segment) of its tiles, on a device of one CU: 16 workgroups, two or three tiles each"""
    walk = R.tile_walk(4000, None, 17 * 1024 + 5, None, cus=1)                    # 18 tiles: nine workgroups of two
    assert walk == [[("resident", 0), ("resident", 0)]] * 8 + [[("resident", 0), ("direct", None)]]
    off = np.array([0, 4096, 8192, 8192 + 5000], dtype=np.uint64)
    qoff = np.array([1024, 2000, 3072, 33 * 1024 - 7], dtype=np.uint64)
    walk = R.tile_walk(8192 + 5000, off, 33 * 1024, qoff, cus=1)                  # 33 tiles: eleven workgroups of three
    assert len(walk) == 11 and walk[0] == [(None, None), ("direct", None), ("resident", 1)] and walk[1] == [("sampled", 2)] * 3
    assert R.tile_walk(8192 + 5000, off, 33 * 1024, qoff, cus=1, sampled=False)[10] == [("direct", None)] * 3
    assert R.tile_walk(8192 + 5000, off, 33 * 1024, qoff, cus=3)[0] == [(None, None)] and R.tile_walk(8192, off[:3], 2048, None, cus=1) == [[("resident", 0)], [("resident", 1)]]
    assert R.pairs_of(walk) >= {((None, None), ("direct", None)), (("direct", None), ("resident", 1)), (("sampled", 2), ("sampled", 2))}


def kinds_of(walk):
    """the ordered pairs inside a workgroup as (path, path, 'same' | 'other' staged segment | None where one of the two stages nothing)"""
    return {(a[0], b[0], None if a[1] is None or b[1] is None else "same" if a[1] == b[1] else "other") for a, b in R.pairs_of(walk)}


def test_two_tile_layouts_reach_their_transitions():
    """the layouts of tests/test_gpu_search_paths.py at 256 CUs: every workgroup walks two tiles, and the ordered pairs of (path, segment)
    that each layout is there for occur inside one workgroup"""
    cus = 256
    two = lambda walk: len(walk) == 2049 and all(len(g) == 2 for g in walk[:-1]) and 1 <= len(walk[-1]) <= 2
    n, off, nq = R.even_layout(cus, 1536)
    assert n == 12948000 and nq == 2731 * 1536 and nq % (len(off) - 1) == 0
    walk = R.tile_walk(n, off, nq, None, cus)
    assert two(walk) and kinds_of(walk) >= {("resident", "resident", "other"), ("resident", "sampled", "other"), ("sampled", "resident", "other"),
                                            ("resident", "direct", None), ("direct", "resident", None), ("sampled", "direct", None),
                                            ("direct", "sampled", None)}
    plain = R.tile_walk(n, off, nq, None, cus, sampled=False)                     # RSX_SEARCH_SAMPLED=0: the sampled tiles take the direct path
    assert [[(p if p != "sampled" else "direct", s if p == "resident" else None) for p, s in g] for g in walk] == plain
    assert ("direct", "direct", None) in kinds_of(plain) and not any(p == "sampled" for g in plain for p, _ in g)
    n, off, nq = R.even_layout(cus, 2048)
    walk = R.tile_walk(n, off, nq, None, cus)
    assert two(walk) and kinds_of(walk) == {("resident", "resident", "same"), ("sampled", "sampled", "same")}
    for L, path in ((4000, "resident"), (50000, "sampled")):
        n, off, nq = R.one_segment_layout(cus, L)
        walk = R.tile_walk(n, off, nq, None, cus)
        assert two(walk) and walk[:-1] == [[(path, 0), (path, 0)]] * 2048 and walk[-1] == [("direct", None)]
    n, off, nq, qoff = R.ragged_dead_layout(cus)
    walk = R.tile_walk(n, off, nq, qoff, cus)
    S = len(off) - 1
    assert two(walk) and int(qoff[-1]) < nq and int(off[-1]) < n and len(qoff) == len(off)
    assert walk[0] == [(None, None), (None, None)] and walk[1] == [(None, None), ("resident", 0)]          # dead tiles at the head,
    assert walk[-2] == [("resident", S - 1), (None, None)] and walk[-1] == [(None, None), (None, None)]    # and at the tail
    assert (int(qoff[-1]) // R.TILE_Q) % 2 == 0 and int(qoff[-1]) % R.TILE_Q != 0
    assert {int(o) % 4 for o in off[:-1]} == {0, 1, 2, 3}
    assert kinds_of(walk) >= {("resident", "resident", "other"), ("resident", "sampled", "other"), ("sampled", "resident", "other")}
    o = off.astype(np.int64)
    both = 0                                                                     # second tiles that restage a segment with a head and a tail around its 16-byte vectors
    for g in walk:
        if len(g) == 2 and g[1][0] == "resident" and g[0][1] != g[1][1]:
            hs, L = o[g[1][1]], o[g[1][1] + 1] - o[g[1][1]]
            head = min((4 - hs % 4) % 4, L)
            both += int(head > 0 and (L - head) % 4 > 0 and L - head >= 4)
    assert both >= 100


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    assert lib.rsx_segmented_search(None, None, 16, None, 1, None, 4, None, 0, None) == 4       # a null engine is refused
    assert b"rsx_segmented_search" in lib.rsx_last_error()
    torch = pytest.importorskip("torch")
    keys = torch.arange(10, dtype=torch.int32)
    vals = torch.tensor([3, 7], dtype=torch.int32)
    offsets = torch.tensor([0, 10], dtype=torch.int64)
    with pytest.raises(ValueError):              # host tensors: no CPU fallback
        rsx.searchsorted(keys, vals)
    with pytest.raises(ValueError):
        rsx.searchsorted(keys.reshape(2, 5), vals.reshape(2, 1))
    with pytest.raises(ValueError):
        rsx.bucketize(vals, keys)
    with pytest.raises(ValueError):
        rsx.segmented_searchsorted(keys, offsets, vals)
    with pytest.raises(ValueError):              # side against right; an unknown side
        rsx.searchsorted(keys, vals, right=True, side="left")
    with pytest.raises(ValueError):
        rsx.searchsorted(keys, vals, side="middle")
    with pytest.raises(NotImplementedError):
        rsx.searchsorted(keys, vals, sorter=torch.arange(10))
    for dt in (torch.float16, torch.bfloat16, torch.bool):
        with pytest.raises(TypeError):           # key types outside the six
            rsx.searchsorted(keys.to(dt), vals.to(dt))
        with pytest.raises(TypeError):
            rsx.bucketize(vals.to(dt), keys.to(dt))
        with pytest.raises(TypeError):
            rsx.segmented_searchsorted(keys.to(dt), offsets, vals.to(dt))
    with pytest.raises(TypeError):               # values of another dtype than the haystack's
        rsx.searchsorted(keys, vals.to(torch.int64))
    with pytest.raises(TypeError):
        rsx.bucketize(vals.to(torch.float32), keys)
    with pytest.raises(TypeError):
        rsx.segmented_searchsorted(keys, offsets, vals.to(torch.float64))
    if not torch.cuda.is_available():
        with pytest.raises(rsx.RadixSortError) as ei:
            rsx.Engine(np.uint32, 16).segmented_search(0, 0, None, 1, 16, 4, None, 16)
        assert ei.value.status == 2              # INITIALIZATION_FAILED: no device, no silent CPU path
