"""Float keys (IEEE 754 totalOrder) and descending order on the GPU.

Every case is compared bit for bit with a numpy oracle, keys AND payload (payload = input index, so the payload is the exact
stable argsort): enc(x) as unsigned words, np.argsort(enc, kind="stable") ascending and np.argsort(~enc, kind="stable")
descending.  Sizes reach every path of the engine: the one-workgroup tile sort (<= 4096 keys), the self-scan on 1024-key tiles
(<= 2^19) and on 4096-key tiles (<= 2^22), the fused-scan chain, and the 8-bit chain (RSX_RADIX8_MIN_KEYS is 4096 under the
test configuration).
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "radix-sort_amd", "host", "bin")

UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64, np.dtype(np.uint32): np.uint32,
        np.dtype(np.int32): np.uint32, np.dtype(np.uint64): np.uint64, np.dtype(np.int64): np.uint64}


def enc(x: np.ndarray) -> np.ndarray:
    """The engine's encoding: unsigned order of enc(x) = sort order of x (totalOrder for floats)."""
    u = UINT[x.dtype]
    bits = np.dtype(u).itemsize * 8
    v = x.view(u)
    sign = u(1) << u(bits - 1)
    if x.dtype.kind == "f":
        return v ^ np.where(v & sign, u(~u(0)), sign).astype(u)
    if x.dtype.kind == "i":
        return v ^ sign
    return v.copy()


def oracle(x: np.ndarray, descending: bool = False, first: int = 0, last: int | None = None) -> np.ndarray:
    """Stable argsort by digits [first, last) (4-bit units) of the encoded key (~enc when descending)."""
    e = enc(x)
    if descending:
        e = ~e
    bits = x.dtype.itemsize * 8
    last = bits // 4 if last is None else last
    if (first, last) != (0, bits // 4):
        u = e.dtype.type
        width = 4 * (last - first)
        mask = u((1 << width) - 1) if width < bits else u(~u(0))
        e = (e >> u(4 * first)) & mask
    return np.argsort(e, kind="stable")


def random_bits(dtype, n, rng):
    u = UINT[np.dtype(dtype)]
    return rng.integers(0, np.iinfo(u).max, size=n, dtype=u, endpoint=True).view(dtype)


def special(dtype, n, rng):
    """NaNs of both signs with distinct payload bits, ±inf, ±0 interleaved, denormals, ties."""
    u = UINT[np.dtype(dtype)]
    f = np.finfo(dtype)
    bits = np.dtype(u).itemsize * 8
    sign = u(1) << u(bits - 1)
    nan = np.array([np.nan], dtype=dtype).view(u)[0]
    pool = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, f.tiny, -f.tiny, f.smallest_subnormal, -f.smallest_subnormal,
                     f.max, -f.max, 2.5, -2.5], dtype=dtype)
    x = pool[rng.integers(0, pool.size, size=n)].copy()
    xb = x.view(u)
    k = n // 4
    idx = rng.choice(n, size=k, replace=False)
    payloads = rng.integers(1, 1 << 20, size=k).astype(u)
    xb[idx] = (nan | payloads) ^ np.where(rng.integers(0, 2, size=k) == 1, sign, u(0)).astype(u)
    return x


def inputs(dtype, n, rng):
    base = random_bits(dtype, n, rng)
    yield "random", base
    if n > 1:
        yield "special", special(dtype, n, rng)
        fin = rng.standard_normal(n).astype(dtype)
        yield "sorted", np.sort(fin)
        yield "reverse", np.sort(fin)[::-1].copy()
        yield "equal", np.full(n, dtype(-3.5), dtype=dtype)
        yield "zeros", np.where(np.arange(n) % 2 == 0, dtype(0.0), dtype(-0.0)).astype(dtype)
        yield "ties", rng.integers(-3, 4, size=n).astype(dtype)


def check(rsx, x, descending, payload=True, options=(), first=0, last=None):
    n = x.size
    order = oracle(x, descending, first, last)
    with rsx.Engine(x.dtype, max(n, 1), payload=payload, descending=descending) as e:
        for opt, val in options:
            e.set_option(opt, val)
        if first != 0 or last is not None:
            e.set_option(rsx.OPT_FIRST_PASS, first)
            e.set_option(rsx.OPT_LAST_PASS, x.dtype.itemsize * 2 if last is None else last)
        e.upload(x, np.arange(n, dtype=np.uint32) if payload else None)
        e.sort()
        got = e.download(want_perm=payload)
    keys, perm = (got if payload else (got, None))
    want = x[order]
    assert keys.view(UINT[x.dtype]).tobytes() == want.view(UINT[x.dtype]).tobytes()
    if payload:
        assert np.array_equal(perm, order.astype(np.uint32))


def test_oracle_agrees_with_numpy_without_negative_zero_and_nan():
    rng = np.random.default_rng(0)
    for dt in (np.float32, np.float64):
        x = rng.standard_normal(5000).astype(dt)
        x[::7] = np.inf
        x[::11] = -np.inf
        x[::13] = 0.0
        x[::5] = x[::10].repeat(2)[: x[::5].size]          # ties
        assert np.array_equal(oracle(x), np.argsort(x, kind="stable"))
        assert np.array_equal(oracle(x, descending=True), np.argsort(-x, kind="stable"))


SIZES = [0, 1, 17, 4096, 4097, 1 << 19, 1 << 21, 1 << 23]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_float_sort_every_path(rsx, dtype, descending, n):
    rng = np.random.default_rng(n + (7 if descending else 0))
    for name, x in inputs(dtype, n, rng):
        if n >= (1 << 21) and name not in ("random", "special"):
            continue
        check(rsx, x, descending, payload=True)
    check(rsx, random_bits(dtype, n, rng), descending, payload=False)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("descending", [False, True])
def test_float_sort_2_26(rsx, dtype, descending):
    rng = np.random.default_rng(26)
    check(rsx, random_bits(dtype, 1 << 26, rng), descending, payload=True)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("n", [5000, 1 << 19, (1 << 21) + 3])
def test_float_sort_8bit_digits(rsx, dtype, descending, n):
    rng = np.random.default_rng(n)
    for payload in (True, False):
        check(rsx, special(dtype, n, rng), descending, payload=payload, options=[(rsx.OPT_RADIX_BITS, 8)])
        check(rsx, random_bits(dtype, n, rng), descending, payload=payload, options=[(rsx.OPT_RADIX_BITS, 8)])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("options", ["nolookahead", "graph", "nosmall", "noself"])
def test_float_sort_options(rsx, dtype, descending, options):
    opt = {"nolookahead": [(rsx.OPT_LOOKAHEAD, 0)], "graph": [(rsx.OPT_GRAPH, 1)],
           "nosmall": [(rsx.OPT_TILE_SORT, 0), (rsx.OPT_SMALL_TILE_MAX_KEYS, 0)], "noself": [(rsx.OPT_SELF_SCAN, 0)]}[options]
    rng = np.random.default_rng(3)
    for n in (17, 4096, 70000, 1 << 20):
        check(rsx, special(dtype, n, rng), descending, options=opt)


@pytest.mark.parametrize("dtype", [np.uint32, np.int32, np.uint64, np.int64])
@pytest.mark.parametrize("n", [1, 4096, 100003, 1 << 22])
@pytest.mark.parametrize("radix_bits", [4, 8])
def test_integer_descending(rsx, dtype, n, radix_bits):
    rng = np.random.default_rng(n)
    info = np.iinfo(dtype)
    x = rng.integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)
    check(rsx, x, True, options=[(rsx.OPT_RADIX_BITS, radix_bits)])
    ties = rng.integers(-2 if info.min < 0 else 0, 3, size=n).astype(dtype)
    check(rsx, ties, True, options=[(rsx.OPT_RADIX_BITS, radix_bits)])
    if info.min < 0:
        assert np.array_equal(oracle(x, True), np.argsort(-x.astype(np.float64) if x.itemsize == 4 else ~x, kind="stable"))


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
@pytest.mark.parametrize("descending", [False, True])
def test_step_api_equals_sort(rsx, dtype, descending):
    rng = np.random.default_rng(5)
    for n in (4096 * 3 + 5, 1 << 18):
        x = special(dtype, n, rng) if np.dtype(dtype).kind == "f" else rng.integers(-5, 5, size=n).astype(dtype)
        order = oracle(x, descending)
        with rsx.Engine(dtype, n, payload=True, descending=descending) as e:
            e.upload(x, np.arange(n, dtype=np.uint32))
            for p in range(x.itemsize * 2):
                e.histogram(p)
                e.scan()
                e.paste()
                e.reorder(p)
            keys, perm = e.download(want_perm=True)
        assert keys.tobytes() == x[order].tobytes() and np.array_equal(perm, order.astype(np.uint32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("descending", [False, True])
def test_pass_ranges(rsx, dtype, descending):
    """Option ranges and rsx_sort_from_to sort by digits of the ENCODED key; an odd range from a byte boundary under 8-bit digits
    runs the mixed chain (8-bit passes, then one 4-bit pass)."""
    import torch
    rng = np.random.default_rng(11)
    P = np.dtype(dtype).itemsize * 2
    for n in (3000, 70000, 1 << 20):
        x = special(dtype, n, rng)
        for first, last in ((0, 2), (1, P - 1), (2, P), (0, P - 1), (3, 4)):
            check(rsx, x, descending, first=first, last=last)
        u = UINT[np.dtype(dtype)]
        t = torch.from_numpy(x.view(u).view(np.int32 if u is np.uint32 else np.int64)).cuda()
        pay = torch.arange(n, dtype=torch.int32, device="cuda")
        for bits in (4, 8):
            for first, last in ((0, P), (0, P - 1), (2, P - 1), (1, 2)):
                out = torch.empty(n + 4, dtype=t.dtype, device="cuda")
                pout = torch.empty(n + 4, dtype=torch.int32, device="cuda")
                with rsx.Engine(dtype, n, payload=True, descending=descending) as e:
                    e.set_option(rsx.OPT_RADIX_BITS, bits)
                    e.sort_from_to(t.data_ptr(), n, first, last, out[4:].data_ptr(), pay.data_ptr(), pout[4:].data_ptr())
                    e.sync()
                order = oracle(x, descending, first, last)
                got = out[4:].cpu().numpy().view(u)
                assert got.tobytes() == x[order].view(u).tobytes(), (bits, first, last, n)
                assert np.array_equal(pout[4:].cpu().numpy().view(np.uint32), order.astype(np.uint32))
        # sort_from on device input, whole range
        with rsx.Engine(dtype, n, payload=True, descending=descending) as e:
            e.sort_from(t.data_ptr(), n, pay.data_ptr())
            keys, perm = e.download(want_perm=True)
        order = oracle(x, descending)
        assert keys.view(u).tobytes() == x[order].view(u).tobytes() and np.array_equal(perm, order.astype(np.uint32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pipeline_submit(rsx, dtype):
    rng = np.random.default_rng(8)
    n = 300001
    for descending in (False, True):
        with rsx.Engine(dtype, n, payload=True, descending=descending) as e:
            ins = [special(dtype, n, rng), random_bits(dtype, n, rng), special(dtype, n, rng)]
            outs = [np.empty(n, dtype=dtype) for _ in ins]
            perm = np.arange(n, dtype=np.uint32)
            pouts = [np.empty(n, dtype=np.uint32) for _ in ins]
            for k, o, po in zip(ins, outs, pouts):
                e.pipeline_submit(k, o, perm, po)
            e.pipeline_wait()
        for k, o, po in zip(ins, outs, pouts):
            order = oracle(k, descending)
            assert o.tobytes() == k[order].tobytes() and np.array_equal(po, order.astype(np.uint32))


def test_fill_pad_values(rsx):
    """rsx_fill_pad writes dec(all-ones - 1): the key that sorts next-to-last in the engine's order."""
    want = {
        (np.uint32, False): 0xFFFFFFFE, (np.int32, False): 0x7FFFFFFE, (np.uint64, False): 0xFFFFFFFFFFFFFFFE,
        (np.int64, False): 0x7FFFFFFFFFFFFFFE,
        (np.uint32, True): 1, (np.int32, True): 0x80000001, (np.uint64, True): 1, (np.int64, True): 0x8000000000000001,
        (np.float32, False): 0x7FFFFFFE, (np.float64, False): 0x7FFFFFFFFFFFFFFE,      # the NaN just below the largest +NaN
        (np.float32, True): 0xFFFFFFFE, (np.float64, True): 0xFFFFFFFFFFFFFFFE,        # the NaN just above the smallest -NaN
    }
    for (dt, desc), bits in want.items():
        u = UINT[np.dtype(dt)]
        with rsx.Engine(dt, 64, descending=desc) as e:
            e.upload(np.zeros(64, dtype=dt))
            e.fill_pad(np.dtype(dt).itemsize * 10)
            got = e.download().view(u)
        assert np.all(got[:10] == 0) and np.all(got[10:] == u(bits)), (dt, desc)
        # and the pad does sort next-to-last
        x = np.array([bits], dtype=u)
        e_ = enc(x.view(dt))
        if desc:
            e_ = ~e_
        assert e_[0] == u(~u(0)) - u(1)


@pytest.mark.parametrize("dtype,descending", [(np.float32, False), (np.float64, True), (np.uint32, True)])
def test_codec_engines_refuse_the_sharded_entry_points(rsx, dtype, descending):
    import torch
    n = 10000
    rng = np.random.default_rng(2)
    x = special(dtype, n, rng) if np.dtype(dtype).kind == "f" else rng.integers(0, 1000, size=n).astype(dtype)
    u = UINT[np.dtype(dtype)]
    t = torch.from_numpy(x.view(u).view(np.int32 if u is np.uint32 else np.int64)).cuda()
    out = torch.empty_like(t)
    counts = torch.zeros(256, dtype=torch.int64, device="cuda")
    with rsx.Engine(dtype, n, descending=descending) as e:
        calls = [
            lambda: e.partition(t.data_ptr(), n, 0, 4, out.data_ptr()),
            lambda: e.partition_count(t.data_ptr(), n, 0, 4),
            lambda: e.partition_count_split(t.data_ptr(), n, [5]),
            lambda: e.sample_keys(t.data_ptr(), n, 16),
            lambda: e.key_range(t.data_ptr(), n),
            lambda: e.msd_count(t.data_ptr(), n, 8, 2, counts.data_ptr()),
            lambda: e.set_option(rsx.OPT_REF_DIAGNOSTICS, 1),
        ]
        for call in calls:
            with pytest.raises(rsx.RadixSortError) as info:
                call()
            assert info.value.status != 0
            assert "float keys or descending order" in str(info.value)
        e.upload(x)
        e.sort()
        assert e.download().tobytes() == x[oracle(x, descending)].tobytes()
    from radix_sort_amd import distributed
    with rsx.Engine(dtype, n, descending=descending) as e:
        with pytest.raises(ValueError, match="integer keys in ascending order"):
            distributed.ShardedSorter(e, 0, 1, x.itemsize * 8)


def test_basic_sort_float_and_descending():
    for args in (["1000003", "--float32", "--descending", "--argsort"], ["300001", "--float64"], ["77777", "--float64", "--descending"],
                 ["4000", "--float32", "--argsort"], ["123457", "--int64", "--descending", "--argsort"]):
        proc = subprocess.run([os.path.join(BIN, "basic_sort")] + args, capture_output=True, text=True, timeout=600)
        assert proc.returncode == 0 and "Result: PASSED" in proc.stdout, (args, proc.stdout[-1000:] + proc.stderr[-1000:])
