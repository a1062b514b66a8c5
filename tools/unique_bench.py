#!/usr/bin/env python3
"""rsx_segmented_unique against its sort partners and against the torch composition it replaces, one JSON line per (shape, keys, form).

Forms: "counts" = keys + counts, partner = the sort of the same input WITHOUT payload; "all" = keys + counts + first + inverse, partner =
the same sort WITH an iota payload.  The partner is rsx_sort_from for one segment (NULL offsets) and rsx_segmented_sort for segment shapes.
Call and partner are measured alternately in one process, PAIR_REPEATS repeats of the pair, so that the partner's spread is known.
Bar (a): call <= partner x (model bytes of the call / model bytes of the partner) x (1 + max(10 %, 2 x partner spread)); the byte model is
DESIGN.md §4d's.  Bar (b): call < composition = the partner's sort followed by torch ops on its output (shifted !=, cumsum, nonzero, diff,
scatter).  A consecutive-mode row (sorted input) and the Python helper against torch.unique are reported without a bar.
Times are HIP events on one stream around each call, median of --iters after --warmup.

    python tools/unique_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/unique_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

rsx = load_package()

PAIR_REPEATS = 5
TILE = 4096


def zipf_lengths(total, rng):
    """segment lengths as tools/segmented_bench.py draws them: empties, single keys and a few huge segments"""
    lens = np.minimum(rng.zipf(1.2, size=1 << 22), 1 << 24) - 1
    lens = lens[np.cumsum(lens) <= total]
    return np.append(lens, total - lens.sum()).astype(np.int64)


SHAPES = [      # name, dtype, n, lengths (None: NULL offsets)
    ("1x2^28_u32", "uint32", 1 << 28, None),
    ("1x2^27_u64", "uint64", 1 << 27, None),
    ("4096x2^16_u32", "uint32", 1 << 28, lambda rng: np.full(4096, 1 << 16, dtype=np.int64)),
    ("2^16x4096_u32", "uint32", 1 << 28, lambda rng: np.full(1 << 16, 4096, dtype=np.int64)),
    ("zipf_2^26_u32", "uint32", 1 << 26, lambda rng: zipf_lengths(1 << 26, rng)),
]
KEYSETS = ["random_bits", "2^16_values"]


def timed(fn, stream, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def make_keys(dtype, n, keyset, gen):
    tdt = {"uint32": torch.int32, "uint64": torch.int64, "int64": torch.int64}[dtype]
    if keyset == "random_bits":
        info = torch.iinfo(tdt)
        return torch.randint(info.min, info.max, (n,), dtype=tdt, device="cuda", generator=gen)
    return torch.randint(0, 1 << 16, (n,), dtype=tdt, device="cuda", generator=gen)


def sort_bytes(kb, pay, lens, n):
    """HBM bytes of the partner sort.  Flat chain (4-bit digits, P = 2 * key bytes passes): one histogram read + P passes of
    read + write.  Segmented: segments of at most one tile are read and written once; larger ones take P passes of histogram read + read + write."""
    P = 2 * kb
    if lens is None:
        return n * (kb + P * 2 * (kb + pay))
    small = int(lens[lens <= TILE].sum())
    large = int(lens[lens > TILE].sum())
    return small * 2 * (kb + pay) + large * P * (3 * kb + 2 * pay)


def unique_extra_bytes(kb, n, runs, form):
    """what the unique passes move beyond the sort: the count pass reads the keys, the write pass reads the keys (and the
    positions), scatters the inverse map and stores key + first + head position per run; the counts pass reads the head positions back."""
    if form == "counts":
        return n * (kb + kb) + runs * (kb + 4 + 4 + 4)
    return n * (kb + kb + 4 + 4) + runs * (kb + 4 + 4 + 4 + 4)


def run_shape(name, dtype, n, lens_fn, keyset, iters, warmup, rng, gen):
    stream = torch.cuda.current_stream()
    kb = 8 if dtype.endswith("64") else 4
    keys = make_keys(dtype, n, keyset, gen)
    lens = None if lens_fn is None else lens_fn(rng)
    offs = None
    nseg = 1
    if lens is not None:
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        nseg = len(lens)
    optr = None if offs is None else offs.data_ptr()
    iota = torch.arange(n, dtype=torch.int32, device="cuda")
    vals = torch.empty_like(keys)
    uoff = torch.empty(nseg + 1, dtype=torch.int64, device="cuda")
    cnt, fst, inv = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    sk = torch.empty_like(keys)
    sp = torch.empty_like(iota)
    rows = []
    for form in ("counts", "all"):
        pay = form == "all"
        eng = rsx.Engine(dtype, n, payload=pay)
        eng.set_stream(stream.cuda_stream)

        def unique():
            eng.segmented_unique(keys.data_ptr(), n, optr, nseg, vals.data_ptr(), uoff.data_ptr(), cnt.data_ptr(), fst.data_ptr() if pay else None,
                                 inv.data_ptr() if pay else None)

        def partner():
            if offs is None:
                eng.sort_from(keys.data_ptr(), n, iota.data_ptr() if pay else None)
            else:
                eng.segmented_sort(keys.data_ptr(), n, optr, nseg, sk.data_ptr(), iota.data_ptr() if pay else None, sp.data_ptr() if pay else None)

        def composition():
            # the same sort, then the finishing step in torch ops on its output
            partner()
            if offs is None:
                eng.copy_result(sk.data_ptr(), sp.data_ptr() if pay else None)          # (a user of rsx_sort_from takes the result out like this)
            flag = torch.ones(n, dtype=torch.bool, device="cuda")
            flag[1:] = sk[1:] != sk[:-1]
            if offs is not None:
                flag[offs[:-1][offs[:-1] < n]] = True
            heads = torch.nonzero(flag).reshape(-1)
            v = sk[heads]
            c = torch.diff(torch.cat([heads, heads.new_tensor([n])]))
            if not pay:
                return v, c
            g = torch.cumsum(flag, 0) - 1
            f = sp[heads]
            iv = torch.empty(n, dtype=torch.int64, device="cuda").scatter_(0, sp.to(torch.int64), g)
            return v, c, f, iv

        uni, par = [], []
        for _ in range(PAIR_REPEATS):                               # alternate the two, so that drift hits both
            par.append(timed(partner, stream, iters, warmup))
            uni.append(timed(unique, stream, iters, warmup))
        comp = timed(composition, stream, max(iters // 2, 3), 1)
        eng.sync()
        runs = int(uoff[-1].item())
        eng.close()
        p_ms, u_ms = float(np.median(par)), float(np.median(uni))
        spread = (max(par) - min(par)) / p_ms
        pb = sort_bytes(kb, 4 if pay else 0, lens, n)
        ub = pb + unique_extra_bytes(kb, n, runs, form)
        margin = max(0.10, 2 * spread)
        bound = p_ms * ub / pb * (1 + margin)
        rows.append({"shape": name, "keys": keyset, "form": form, "n": n, "segments": nseg, "dtype": dtype, "runs": runs,
                     "unique_ms": u_ms, "unique_repeats_ms": uni, "partner": ("rsx_sort_from" if offs is None else "rsx_segmented_sort") + (" + iota payload" if pay else ""),
                     "partner_ms": p_ms, "partner_repeats_ms": par, "partner_spread": spread, "partner_model_bytes": pb, "unique_model_bytes": ub,
                     "byte_ratio": ub / pb, "time_ratio": u_ms / p_ms, "margin": margin, "bar_a_bound_ms": bound, "bar_a": "met" if u_ms <= bound else "missed",
                     "composition_ms": comp, "bar_b": "met" if u_ms < comp else "missed"})
        torch.cuda.empty_cache()
    return rows


def run_consecutive(iters, warmup, gen):
    """1 x 2^28 uint32, sorted input, consecutive mode, keys + counts: model bytes over time as a share of 8 TB/s (report only)"""
    stream = torch.cuda.current_stream()
    n = 1 << 28
    rows = []
    for keyset in KEYSETS:
        keys = torch.sort(make_keys("uint32", n, keyset, gen)).values
        vals = torch.empty_like(keys)
        uoff = torch.empty(2, dtype=torch.int64, device="cuda")
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        eng = rsx.Engine("uint32", n)
        eng.set_stream(stream.cuda_stream)
        ms = timed(lambda: eng.segmented_unique(keys.data_ptr(), n, None, 1, vals.data_ptr(), uoff.data_ptr(), cnt.data_ptr(), consecutive=True), stream, iters, warmup)
        eng.sync()
        runs = int(uoff[-1].item())
        eng.close()
        moved = unique_extra_bytes(4, n, runs, "counts")
        rows.append({"shape": "1x2^28_u32_sorted_consecutive", "keys": keyset, "form": "counts", "n": n, "runs": runs, "unique_ms": ms, "model_bytes": moved,
                     "tb_per_s": moved / ms / 1e9, "share_of_8tb_s": moved / ms / 1e9 / 8.0})
        del keys, vals, cnt
        torch.cuda.empty_cache()
    return rows


def run_helper(iters, warmup, gen):
    """rsx.unique(return_inverse, return_counts) against torch.unique, 2^24 int64 with 2^16 distinct values (report only)"""
    stream = torch.cuda.current_stream()
    x = make_keys("int64", 1 << 24, "2^16_values", gen)
    ours = timed(lambda: rsx.unique(x, return_inverse=True, return_counts=True), stream, iters, warmup)
    theirs = timed(lambda: torch.unique(x, return_inverse=True, return_counts=True), stream, iters, warmup)
    return [{"shape": "1x2^24_i64_helper", "keys": "2^16_values", "form": "unique(return_inverse, return_counts)", "n": 1 << 24, "helper_ms": ours,
             "torch_unique_ms": theirs, "vs_torch": ours / theirs}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = args.only.split(",") if args.only else None
    rng = np.random.default_rng(2026)
    gen = torch.Generator(device="cuda").manual_seed(2026)
    out = []

    def emit(rows):
        for row in rows:
            row["device"] = rsx.device_name(0)
            print(json.dumps(row), flush=True)
            out.append(row)
        if args.out:                                            # rewritten after every shape: a cut-short run keeps what it measured
            with open(args.out, "w") as f:
                for r in out:
                    f.write(json.dumps(r) + "\n")

    for name, dtype, n, lens_fn in SHAPES:
        if only and name not in only:
            continue
        keysets = KEYSETS if lens_fn is None else KEYSETS[:1]
        for keyset in keysets:
            emit(run_shape(name, dtype, n, lens_fn, keyset, args.iters, args.warmup, rng, gen))
    if not only or "consecutive" in only:
        emit(run_consecutive(args.iters, args.warmup, gen))
    if not only or "helper" in only:
        emit(run_helper(args.iters, args.warmup, gen))
    for r in out:
        if "partner_ms" in r:
            print(f"{r['shape']:>16} {r['keys']:>12} {r['form']:>6}  unique {r['unique_ms']:.3f} ms | {r['partner']} {r['partner_ms']:.3f} (spread {r['partner_spread']:.1%}) | "
                  f"x{r['time_ratio']:.2f} measured, x{r['byte_ratio']:.2f} by bytes -> (a) {r['bar_a']} | composition {r['composition_ms']:.3f} -> (b) {r['bar_b']}",
                  file=sys.stderr)


if __name__ == "__main__":
    main()
