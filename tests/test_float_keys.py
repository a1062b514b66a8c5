"""CPU checks of float keys and descending order: the header and the binding agree on the key kinds and RSX_OPT_DESCENDING, the
numpy totalOrder oracle of tests/test_gpu_float_keys.py orders hand-picked special values as IEEE 754 says, a float engine fails
like every other engine without a GPU (no TypeError), and the host library instantiates RadixSortGPU<float> and <double>."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_float_keys import enc, oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "radixsort_hip.h")
HOST_LIB = os.path.join(ROOT, "radix-sort_amd", "host", "libradixsort_host.so")


def test_key_kinds_and_descending_match_the_header(rsx):
    text = open(HEADER).read()
    kinds = {n: int(v) for n, v in re.findall(r"#define RSX_KEY_([A-Z]+) (\d+)", text)}
    assert kinds == {"UNSIGNED": rsx.KEY_UNSIGNED, "SIGNED": rsx.KEY_SIGNED, "FLOAT": rsx.KEY_FLOAT} == {"UNSIGNED": 0, "SIGNED": 1, "FLOAT": 2}
    assert int(re.search(r"RSX_OPT_DESCENDING\s*=\s*(\d+)", text).group(1)) == rsx.OPT_DESCENDING >= 21
    assert rsx._KEY_DTYPES["float32"] == (4, 2) and rsx._KEY_DTYPES["float64"] == (8, 2)
    assert "int key_kind" in text


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_orders_special_values_as_total_order(dtype):
    u = np.uint32 if dtype == np.float32 else np.uint64
    bits = np.dtype(u).itemsize * 8
    sign = u(1) << u(bits - 1)
    qnan = np.array([np.nan], dtype=dtype).view(u)[0]
    f = np.finfo(dtype)
    # ascending IEEE 754 totalOrder, by hand: -NaNs (larger payload first), -inf .. -0.0, +0.0 .. +inf, +NaNs
    vals = np.array([-np.inf, -f.max, -1.0, -f.tiny, -f.smallest_subnormal, -0.0, 0.0, f.smallest_subnormal, f.tiny, 1.0,
                     f.max, np.inf], dtype=dtype).view(u)
    want = np.concatenate([np.array([qnan | sign | u(5), qnan | sign], dtype=u), vals, np.array([qnan, qnan | u(5)], dtype=u)])
    shuffled = np.random.default_rng(1).permutation(want)
    x = shuffled.view(dtype)
    assert np.array_equal(x[oracle(x)].view(u), want)
    assert np.array_equal(x[oracle(x, descending=True)].view(u), want[::-1])
    # encoded order is unsigned order; the encoding is a bijection
    e = enc(want.view(dtype))
    assert all(e[i] < e[i + 1] for i in range(e.size - 1)) and np.unique(e).size == e.size
    # stability of ties in both directions, and agreement with numpy away from -0.0 and NaN
    t = np.array([2.0, 1.0, 2.0, -1.0, 1.0], dtype=dtype)
    assert list(oracle(t)) == [3, 1, 4, 0, 2]
    assert list(oracle(t, descending=True)) == [0, 2, 1, 4, 3]
    assert np.array_equal(oracle(t), np.argsort(t, kind="stable"))


def test_float_engine_without_gpu_fails_with_status_2(rsx):
    try:
        devices = rsx.device_count()
    except rsx.RadixSortError:
        devices = 0
    if devices > 0:          # (a HIP device is visible: float and descending engines are created, no TypeError)
        for dtype in (np.float32, np.float64):
            with rsx.Engine(dtype, 8, descending=True) as e:
                assert e.codec
        return
    for dtype in (np.float32, np.float64):
        with pytest.raises(rsx.RadixSortError) as info:
            rsx.Engine(dtype, 8)
        assert info.value.status == 2
    with pytest.raises(rsx.RadixSortError) as info:
        rsx.Engine(np.uint32, 8, descending=True)
    assert info.value.status == 2


def test_host_library_instantiates_float_and_double():
    if not os.path.exists(HOST_LIB):
        subprocess.run(["make", "-C", os.path.dirname(HOST_LIB), "libradixsort_host.so"], check=True, capture_output=True, timeout=600)
    out = subprocess.run(["nm", "-C", "--defined-only", HOST_LIB], capture_output=True, text=True, check=True, timeout=120).stdout
    assert "RadixSortGPU<float>::" in out and "RadixSortGPU<double>::" in out
