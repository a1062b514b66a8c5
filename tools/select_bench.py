#!/usr/bin/env python3
"""Radix select (rsx_segmented_select) against its baselines, one JSON line per shape (and a table on stderr).

Big shapes (one segment): R = 1 at rank n/2 against rsx_segmented_topk with k = 1 on the same input — measured alternately, several
repeats of the pair, so that the spread of the comparison partner is known —, R = 8 at the octiles against eight R = 1 calls and
against rsx_segmented_sort of the shape.  Row shapes: the engine call behind median / kthvalue / quantile against sort_rows plus a
gather; the Python helper and torch.median / torch.kthvalue / torch.quantile are reported beside them.
Times are HIP events on one stream around each call, median of --iters after --warmup.

    python tools/select_bench.py [--iters 10] [--warmup 3] [--only NAME] [--out profiles/select_bench.jsonl]
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

BIG = [      # name, dtype, n
    ("1x2^28_u32", "uint32", 1 << 28),
    ("1x2^27_u64", "uint64", 1 << 27),
]
ROWS = [     # name, dtype, rows, cols, what, argument
    ("64x2^17_f32_median", "float32", 64, 1 << 17, "median", None),
    ("4096x4096_f32_median", "float32", 4096, 4096, "median", None),
    ("1024x50257_f32_quantile4", "float32", 1024, 50257, "quantile", [0.05, 0.25, 0.75, 0.95]),
    ("256x2^17_i32_kth65536", "int32", 256, 1 << 17, "kthvalue", 1 << 16),
]
PAIR_REPEATS = 5


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


def launches(bits, rows, cols):
    """Kernels the host enqueues for one rsx_segmented_select of `rows` segments of `cols` keys (sized from n and S only, not from R)."""
    n = rows * cols
    count = 4                                                   # classify, scan, classify, init
    count += sum(1 for m in (2, 257, 1025) if min(rows, n // m) > 0)      # small classes
    if min(rows, n // 4097) > 0:
        count += 2 * (bits // 8) + 4                            # select rounds (hist + pick), count, 2 scans, locate
    return count


def make_keys(dtype, n, rng):
    npdt = {"uint32": np.uint32, "int32": np.int32, "uint64": np.uint64, "float32": np.float32}[dtype]
    if dtype == "float32":
        x = rng.standard_normal(n, dtype=np.float32)
        return torch.from_numpy(x).cuda()
    x = rng.integers(np.iinfo(npdt).min, np.iinfo(npdt).max, size=n, dtype=npdt, endpoint=True)
    return torch.from_numpy(x.view({4: np.int32, 8: np.int64}[x.itemsize])).cuda()


def run_big(name, dtype, n, iters, warmup, rng):
    stream = torch.cuda.current_stream()
    keys = make_keys(dtype, n, rng)
    offs = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    eng = rsx.Engine(dtype, n)
    eng.set_stream(stream.cuda_stream)
    vout = torch.empty(8, dtype=keys.dtype, device="cuda")
    iout = torch.empty(8, dtype=torch.int32, device="cuda")
    r1 = torch.tensor([n // 2], dtype=torch.int32, device="cuda")
    r8 = torch.tensor([(2 * j + 1) * (n // 16) for j in range(8)], dtype=torch.int64, device="cuda").to(torch.int32)     # the 8 octile midpoints
    singles = [r8[j:j + 1].clone() for j in range(8)]

    def select(ranks, R):
        eng.segmented_select(keys.data_ptr(), n, offs.data_ptr(), 1, ranks.data_ptr(), R, vout.data_ptr(), iout.data_ptr())

    def topk1():
        eng.segmented_topk(keys.data_ptr(), n, offs.data_ptr(), 1, 1, vout.data_ptr(), iout.data_ptr())

    def eight_singles():
        for r in singles:
            select(r, 1)

    row = {"shape": name, "n": n, "dtype": dtype, "launches": launches(keys.element_size() * 8, 1, n)}
    sel, top = [], []
    for _ in range(PAIR_REPEATS):                               # alternate the two, so that drift hits both
        top.append(timed(topk1, stream, iters, warmup))
        sel.append(timed(lambda: select(r1, 1), stream, iters, warmup))
    row["select_r1_ms"] = float(np.median(sel))
    row["select_r1_repeats_ms"] = sel
    row["topk_k1_ms"] = float(np.median(top))
    row["topk_k1_repeats_ms"] = top
    row["topk_k1_spread"] = (max(top) - min(top)) / float(np.median(top))
    row["r1_vs_topk_k1"] = row["select_r1_ms"] / row["topk_k1_ms"]
    row["r1_margin"] = max(0.10, 2 * row["topk_k1_spread"])
    row["select_r8_ms"] = timed(lambda: select(r8, 8), stream, iters, warmup)
    row["eight_r1_calls_ms"] = timed(eight_singles, stream, iters, warmup)
    row["r8_vs_r1"] = row["select_r8_ms"] / row["select_r1_ms"]
    sout = torch.empty_like(keys)
    row["segmented_sort_ms"] = timed(lambda: eng.segmented_sort(keys.data_ptr(), n, offs.data_ptr(), 1, sout.data_ptr()), stream, iters, warmup)
    row["sort_from_ms"] = timed(lambda: eng.sort_from(keys.data_ptr(), n), stream, iters, warmup)
    eng.sync()
    eng.close()
    row["r8_vs_segmented_sort"] = row["select_r8_ms"] / row["segmented_sort_ms"]
    row["gkeys_r1"] = n / row["select_r1_ms"] / 1e6
    return row


def run_rows(name, dtype, rows, cols, what, arg, iters, warmup, rng):
    stream = torch.cuda.current_stream()
    n = rows * cols
    x = make_keys(dtype, n, rng).reshape(rows, cols)
    offs = torch.arange(0, rows + 1, dtype=torch.int64, device="cuda") * cols
    if what == "median":
        lo = hi = torch.tensor([(cols - 1) // 2])
        weight = None
    elif what == "kthvalue":
        lo = hi = torch.tensor([arg - 1])
        weight = None
    else:
        lo, hi, weight = rsx.select_ranks(cols, q=torch.tensor(arg, dtype=x.dtype), interpolation="linear")
    rank_row = lo if weight is None else torch.cat([lo, hi])
    R = rank_row.numel()
    ranks = rank_row.to(torch.int32).reshape(1, R).expand(rows, R).contiguous().cuda()
    gather_at = rank_row.to(torch.int64).cuda()
    eng = rsx.Engine(dtype, n)
    eng.set_stream(stream.cuda_stream)
    vout = torch.empty(rows * R, dtype=x.dtype, device="cuda")
    iout = torch.empty(rows * R, dtype=torch.int32, device="cuda")
    row = {"shape": name, "rows": rows, "cols": cols, "n": n, "dtype": dtype, "what": what, "ranks_per_row": R,
           "launches": launches(x.element_size() * 8, rows, cols)}
    sel, srt = [], []

    def sort_gather():
        sv, si = rsx.sort_rows(x)
        return sv[:, gather_at], si[:, gather_at]

    for _ in range(3):                                          # alternate the two
        srt.append(timed(sort_gather, stream, iters, warmup))
        sel.append(timed(lambda: eng.segmented_select(x.data_ptr(), n, offs.data_ptr(), rows, ranks.data_ptr(), R, vout.data_ptr(), iout.data_ptr()),
                         stream, iters, warmup))
    eng.sync()
    eng.close()
    row["select_engine_ms"] = float(np.median(sel))
    row["sort_rows_gather_ms"] = float(np.median(srt))
    row["vs_sort_rows_gather"] = row["select_engine_ms"] / row["sort_rows_gather_ms"]
    if what == "median":
        row["helper_ms"] = timed(lambda: rsx.median(x), stream, iters, warmup)
        row["torch_ms"] = timed(lambda: torch.median(x, dim=-1), stream, iters, warmup)
    elif what == "kthvalue":
        row["helper_ms"] = timed(lambda: rsx.kthvalue(x, arg), stream, iters, warmup)
        row["torch_ms"] = timed(lambda: torch.kthvalue(x, arg, dim=-1), stream, iters, warmup)
    else:
        q = torch.tensor(arg, dtype=x.dtype, device="cuda")
        row["helper_ms"] = timed(lambda: rsx.quantile(x, q), stream, iters, warmup)
        try:
            row["torch_ms"] = timed(lambda: torch.quantile(x, q, dim=-1), stream, iters, warmup)
        except RuntimeError as err:                             # torch.quantile refuses inputs above 16 M elements
            row["torch_ms"] = None
            row["torch_note"] = str(err).splitlines()[0][:120]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(2026)
    out = []
    for name, dtype, n in BIG:
        if args.only and args.only != name:
            continue
        row = run_big(name, dtype, n, args.iters, args.warmup, rng)
        row["device"] = rsx.device_name(0)
        print(json.dumps(row), flush=True)
        out.append(row)
        torch.cuda.empty_cache()
    for name, dtype, rows, cols, what, arg in ROWS:
        if args.only and args.only != name:
            continue
        row = run_rows(name, dtype, rows, cols, what, arg, args.iters, args.warmup, rng)
        row["device"] = rsx.device_name(0)
        print(json.dumps(row), flush=True)
        out.append(row)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")
    fmt = lambda v: "—" if v is None else f"{v:.3f}"      # noqa: E731
    for r in out:
        if "select_r1_ms" in r:
            print(f"{r['shape']:>26}  R=1 {r['select_r1_ms']:.3f} ms | top-k k=1 {r['topk_k1_ms']:.3f} (spread {r['topk_k1_spread']:.1%}) | R=8 {r['select_r8_ms']:.3f} "
                  f"(x{r['r8_vs_r1']:.2f} of R=1) | 8 x R=1 {r['eight_r1_calls_ms']:.3f} | segmented_sort {r['segmented_sort_ms']:.3f} | sort_from "
                  f"{r['sort_from_ms']:.3f} | {r['launches']} launches", file=sys.stderr)
        else:
            print(f"{r['shape']:>26}  select {r['select_engine_ms']:.3f} ms ({fmt(r['helper_ms'])} helper) | sort_rows + gather {r['sort_rows_gather_ms']:.3f} "
                  f"(x{r['vs_sort_rows_gather']:.2f}) | torch {fmt(r['torch_ms'])} | {r['launches']} launches", file=sys.stderr)


if __name__ == "__main__":
    main()
