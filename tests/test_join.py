"""CPU checks of the join: header, exports, binding and the Python callables agree on rsx_segmented_join; the host referee
(tests/_join_ref.py) agrees with a brute-force double loop over bit equality for the four kinds, six key types and both directions, signed
zeros and NaN bit patterns included; every layout the GPU tests run reaches the kernel path it is named for; the stand-alone join_selftest —
the row rule, the two-level split and the tile stores the kernels call, compiled by g++ — gives the referee's figures on those layouts,
plain and as a second stand-alone binary built with -fsanitize=address,undefined (nothing is loaded into Python under a sanitizer); and the
call and the torch helpers fail loudly instead of working on the CPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _join_ref as R
from _join_ref import ANTI, INNER, LEFT, SEMI, TILE
from _search_ref import sort_engine_order
from test_expand import stores_of
from test_search import header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "radix-sort_amd", "host", "bin")
SELFTESTS = {"plain": os.path.join(BIN, "join_selftest"), "sanitized": os.path.join(BIN, "join_selftest_san")}
HELPERS = ("segmented_join", "join_sorted", "isin_sorted")


def test_header_binding_and_exports_agree(rsx):
    text = re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S)
    m = re.search(r"int\s+rsx_segmented_join\s*\(([^;]*)\)\s*;", text)
    assert m, "rsx_segmented_join is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["rsx_engine* e", "const void* d_a", "uint64_t na", "const uint64_t* d_a_offsets", "const void* d_b", "uint64_t nb",
                      "const uint64_t* d_b_offsets", "uint64_t num_segments", "uint32_t op", "uint32_t flags", "uint64_t out_capacity", "void* d_keys_out",
                      "uint32_t* d_a_index_out", "uint32_t* d_b_index_out", "uint64_t* d_out_offsets"]
    for name, value in (("INNER", 0), ("LEFT", 1), ("SEMI", 2), ("ANTI", 3)):
        d = re.search(rf"#define\s+RSX_JOIN_{name}\s+(\d+)", header_text())
        assert d and int(d.group(1)) == value == getattr(rsx, "JOIN_" + name) == R.KINDS[name.lower()]
    assert "rsx_segmented_join" in rsx.SYMBOLS
    fn = rsx.load_library().rsx_segmented_join
    P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert fn.argtypes == [P, P, U64, P, P, U64, P, U64, U32, U32, U64, P, P, P, P]
    assert fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", rsx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rsx_segmented_join\b", out)
    for name in HELPERS:
        assert callable(getattr(rsx, name)), name
    assert callable(rsx.Engine.segmented_join)


def test_no_cpu_path(rsx):
    lib = rsx.load_library()
    assert lib.rsx_segmented_join(None, None, 0, None, None, 0, None, 1, 0, 0, 0, None, None, None, None) == 4        # a null engine is refused
    assert lib.rsx_last_error() == b"rsx_segmented_join: null engine"
    torch = pytest.importorskip("torch")
    a, b = torch.tensor([1, 2, 2], dtype=torch.int32), torch.tensor([2, 3], dtype=torch.int32)
    off = torch.tensor([0, 3], dtype=torch.int64)
    for call in (lambda: rsx.segmented_join(a, off, b, torch.tensor([0, 2])), lambda: rsx.join_sorted(a, b), lambda: rsx.join_sorted(a, b, how="left", capacity=8),
                 lambda: rsx.isin_sorted(a, b), lambda: rsx.isin_sorted(a, b, invert=True)):
        with pytest.raises(ValueError):                            # host tensors: no CPU fallback
            call()
    with pytest.raises(TypeError):
        rsx.join_sorted(a, b.to(torch.int64))
    with pytest.raises(TypeError):
        rsx.join_sorted(a.to(torch.float16), b.to(torch.float16))
    with pytest.raises(TypeError):
        rsx.isin_sorted(a > 1, b > 1)


# -- the referee ---------------------------------------------------------------------------------------------------------------------------

def special_keys(dt):
    """small keys with duplicates; floats: both zeros and NaNs of three bit patterns among them"""
    dt = np.dtype(dt)
    vals = np.arange(-3 if dt.kind != "u" else 0, 6).astype(dt)
    if dt.kind == "f":
        u = R.UINT[dt.itemsize]
        nan = np.array([np.nan], dtype=dt).view(u)[0]
        extra = np.array([0, 1 << (8 * dt.itemsize - 1), nan, nan | u(1), nan | u(1 << (8 * dt.itemsize - 1))], dtype=u).view(dt)
        vals = np.concatenate([vals, extra])
    return vals


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_referee_against_brute_force(dtype, descending):
    rng = np.random.default_rng(len(dtype) + descending)
    pool = special_keys(dtype)
    for trial in range(12):
        S = int(rng.integers(1, 6))
        la, lb = rng.integers(0, 9, S), rng.integers(0, 9, S)
        aoff, boff = R.offsets_from(la, int(rng.integers(0, 3))), R.offsets_from(lb, int(rng.integers(0, 3)))
        a, b = pool[rng.integers(0, pool.size, int(aoff[-1]) + 2)], pool[rng.integers(0, pool.size, int(boff[-1]) + 1)]
        for x, off in ((a, aoff), (b, boff)):
            for s0, s1 in R.bounds(x.size, off):
                x[s0:s1] = sort_engine_order(x[s0:s1], descending)
        for op in (INNER, LEFT, SEMI, ANTI):
            ia, ib, keys, ooff = R.join_oracle(a, aoff, b, boff, op, descending)
            bia, bib, booff = R.join_brute(a, aoff, b, boff, op)
            assert np.array_equal(ia, bia) and np.array_equal(ib, bib) and np.array_equal(ooff, booff), (dtype, descending, op, trial)
            seg = np.repeat(np.arange(S), np.diff(ooff.astype(np.int64)))
            u = R.UINT[np.dtype(dtype).itemsize]
            assert np.array_equal(keys.view(u), a.view(u)[aoff.astype(np.int64)[seg] + ia])
            if op in (INNER, SEMI):
                assert np.array_equal(keys.view(u), b.view(u)[boff.astype(np.int64)[seg] + ib])      # partners are equal bit for bit
    if np.dtype(dtype).kind == "f":
        z = np.array([-0.0, 0.0], dtype=dtype)
        assert R.join_oracle(z[:1], None, z[1:], None, INNER)[0].size == 0                             # -0.0 and +0.0 do not join
        nan = np.array([np.nan], dtype=dtype)
        assert R.join_oracle(nan, None, nan.copy(), None, INNER)[0].size == 1                          # NaNs of equal bits do


# -- the layouts of the GPU tests ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_layouts_reach_the_paths_they_are_named_for(name):
    make, op, want = R.LAYOUTS[name]
    a, aoff, b, boff = make()
    got = R.paths(a, aoff, b, boff, op)
    assert want <= got, (name, sorted(want - got))


def test_layout_sizes_are_the_ones_asked_for():
    la, lb = R.ragged_lengths()
    assert len(la) == len(lb) == 37 and max(la) == max(lb) == 9000 and min(la) == min(lb) == 0
    assert any(x == 0 and y > 0 for x, y in zip(la, lb)) and any(x > 0 and y == 0 for x, y in zip(la, lb)) and any(x == 0 and y == 0 for x, y in zip(la, lb))
    a, aoff, b, boff = R.layout_ragged()
    c = R.counts(a, aoff, b, boff)[1]
    assert np.any(c == 0) and np.any(c == 1) and np.any(c > 1)
    for P in R.TOTALS:
        assert R.model(*R.layout_total(P), INNER)["total"] == P
    for na in R.ONE_PARTNER:
        a, _, b, _ = R.layout_one_partner(na)
        assert a.size == na and R.model(a, None, b, None, INNER)["total"] == na
    a, _, b, _ = R.layout_sparse()
    m = R.model(a, None, b, None, INNER)
    assert a.size == b.size == 3 * TILE + 5 and m["total"] == 7 and m["ttot"][1] == 0
    assert np.flatnonzero(m["cnt"]).tolist() == list(R.SPARSE_MATCHES) and np.max(np.diff(np.flatnonzero(m["cnt"]))) >= TILE
    assert R.model(a, None, b, None, LEFT)["total"] == a.size
    a, aoff, b, boff = R.layout_many_segments()
    assert aoff.size == boff.size == 4097
    a, aoff, b, boff = R.layout_zipf()
    assert a.size == b.size == 1 << 16 and np.any(np.diff(aoff.astype(np.int64)) == 0) and np.any(np.diff(boff.astype(np.int64)) == 0)
    assert R.model(*R.layout_all_equal(4097, 4097), INNER)["total"] == 4097 * 4097


# -- the stand-alone program: the kernels' own functions on the CPU ----------------------------------------------------------------------------

def selftest(tmp_path, which, op, c, cap, addr, eb):
    path = tmp_path / "case.txt"
    path.write_text(f"{op} {len(c)} {cap} {addr} {eb}\n" + " ".join(str(int(v)) for v in c) + "\n")
    proc = subprocess.run([SELFTESTS[which], str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    assert proc.stderr == "", proc.stderr[-2000:]                  # a sanitizer report would stand here
    out = {"t": []}
    for line in proc.stdout.splitlines():
        f = line.split()
        if f[0] == "t":
            out["t"].append([int(v) for v in f[1:]])
        else:
            out[f[0]] = np.array([int(v) for v in f[1:]], dtype=np.int64)
    return out


def absolute_counts(a, aoff, b, boff):
    """partner counts per absolute A position of [0, na): 0 outside [aoff[0], aoff[S])"""
    c = np.zeros(a.size, dtype=np.int64)
    lo = 0 if aoff is None else int(aoff[0])
    live = R.counts(a, aoff, b, boff)[1]
    c[lo:lo + live.size] = live
    return c, lo, lo + live.size


SELFTEST_LAYOUTS = ["ragged", "all equal 5000 x 3", "all equal 3 x 10000", "sparse inner", "many segments"]


@pytest.mark.parametrize("which", list(SELFTESTS))
@pytest.mark.parametrize("name", SELFTEST_LAYOUTS)
def test_selftest_on_the_layouts(tmp_path, name, which):
    a, aoff, b, boff = R.LAYOUTS[name][0]()
    c, lo, hi = absolute_counts(a, aoff, b, boff)
    for op, (addr, eb), cap in ((INNER, (0, 4), 1 << 34), (LEFT, (4, 4), 5000), (SEMI, (8, 8), 1 << 34), (ANTI, (12, 4), 4097)):
        live = np.zeros(c.size, dtype=bool)
        live[lo:hi] = True
        # (the kernel counts 0 outside the live range whatever the kind; the case file carries c, so dead positions are cut off here)
        got = selftest(tmp_path, which, op, c[lo:hi], cap, addr, eb)
        e = R.effective(c[lo:hi], op)
        assert np.array_equal(got["e"], e)
        assert np.array_equal(got["f"], np.where((c[lo:hi] == 0) & (op == LEFT), 0xFFFFFFFF, np.arange(hi - lo)))
        Rj = np.concatenate([[0], np.cumsum(e)])
        assert np.array_equal(got["r"], Rj) and int(got["p"][0]) == int(Rj[-1])
        total, written = int(Rj[-1]), min(int(Rj[-1]), cap)
        npos = -(-(hi - lo) // TILE) * TILE
        Rpad = np.concatenate([Rj[:-1], np.full(npos - (hi - lo), total)])          # the padding starts its (no) rows at P
        assert len(got["t"]) == -(-written // TILE) + 1
        for u, s_lo, s_hi, ra, rb, head, nvec, tail in got["t"]:
            assert (s_lo, s_hi) == (int(np.count_nonzero(Rpad < u * TILE)), int(np.count_nonzero(Rpad < (u + 1) * TILE)))
            if u * TILE >= written:
                assert ra >= rb
                continue
            assert (ra, rb) == (u * TILE, min((u + 1) * TILE, written))
            assert (head, nvec, tail) == stores_of(addr, eb, ra, rb)
            assert head + nvec * (16 // eb) + tail == rb - ra
            if s_lo == s_hi:                                       # a pure fill: one owner, and it has every row of the tile
                assert s_lo >= 1 and Rpad[s_lo - 1] <= ra and Rpad[s_lo - 1] + e[s_lo - 1] >= rb


def test_selftest_64_bit_totals(tmp_path):
    """65537 A elements with 65536 partners each: P = 2^32 + 65536; one element of 2^31 partners spans 2^19 tiles"""
    for which in SELFTESTS:
        got = selftest(tmp_path, which, INNER, np.full(65537, 65536), 8192, 0, 4)
        assert int(got["p"][0]) == (1 << 32) + 65536 and int(got["r"][-2]) == 1 << 32
        assert [t[1:3] for t in got["t"]] == [[0, 1], [1, 1], [1, 1]] and [t[3:5] for t in got["t"]] == [[0, 4096], [4096, 8192], [8192, 8192]]
        got = selftest(tmp_path, which, INNER, [1 << 31, 1 << 31, 3], 1, 0, 8)
        assert got["r"].tolist() == [0, 1 << 31, 1 << 32, (1 << 32) + 3]


def test_selftest_refuses_bad_cases(tmp_path):
    for text in ("4 2 10 0 4\n1 1\n", "0 2 10 2 4\n1 1\n", "0 2 10 0 3\n1 1\n", "0 3 10 0 4\n1 1\n", "0 1 10 0 4\n4294967296\n"):
        path = tmp_path / "bad.txt"
        path.write_text(text)
        for exe in SELFTESTS.values():
            assert subprocess.run([exe, str(path)], capture_output=True, text=True).returncode == 1, text
