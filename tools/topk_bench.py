#!/usr/bin/env python3
"""Top-k by radix select against its baselines, one JSON line per shape (and a table on stderr).

For each shape: radix_sort_amd.topk / segmented_topk (rsx_segmented_topk), torch.topk, the full segmented sort plus a slice
(sort_rows on row shapes, segmented_sort of the one segment otherwise) and rsx_sort_from of the same n (context: one sort over
everything).  Times are HIP events on one stream around each call, median of --iters after --warmup; Gkeys/s = n / time.
The launch count of the rsx_segmented_topk chain is reported with every shape.

    python tools/topk_bench.py [--iters 10] [--warmup 3] [--only NAME] [--out profiles/topk_bench.jsonl]
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

SHAPES = [   # name, dtype, largest, rows, keys per row, k
    ("1x2^28_u32_k1000", "uint32", False, 1, 1 << 28, 1000),
    ("1x2^27_u64_k1000", "uint64", False, 1, 1 << 27, 1000),
    ("64x2^17_f32_largest_k50", "float32", True, 64, 1 << 17, 50),
    ("1x2^17_f32_largest_k50", "float32", True, 1, 1 << 17, 50),
    ("4096x4096_f32_largest_k32", "float32", True, 4096, 4096, 32),
    ("256x2^17_i32_largest_k4096", "int32", True, 256, 1 << 17, 4096),
]
TORCH_DT = {"uint32": torch.int32, "int32": torch.int32, "uint64": torch.int64, "float32": torch.float32}


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


def launches(bits, rows, cols, k):
    """Kernels the host enqueues for one rsx_segmented_topk of `rows` segments of `cols` keys (sized from n and S only)."""
    n = rows * cols
    count = 4                                                   # classify, scan, classify, init
    count += sum(1 for m in (2, 257, 1025) if min(rows, n // m) > 0)      # small classes
    if min(rows, n // 4097) > 0:
        count += 2 * (bits // 8) + 4 + 1                       # select rounds (hist + pick), count, 2 scans, compact, final sort
    return count


def run_shape(name, dtype, largest, rows, cols, k, iters, warmup, rng):
    n = rows * cols
    npdt = {"uint32": np.uint32, "int32": np.int32, "uint64": np.uint64, "float32": np.float32}[dtype]
    if dtype == "float32":
        x = rng.standard_normal(n, dtype=np.float32)
    else:
        x = rng.integers(np.iinfo(npdt).min, np.iinfo(npdt).max, size=n, dtype=npdt, endpoint=True)
    stream = torch.cuda.current_stream()
    sv = {4: np.int32, 8: np.int64}[x.itemsize]
    keys = torch.from_numpy(x.view(sv) if dtype != "float32" else x).cuda()
    offs = torch.arange(0, rows + 1, dtype=torch.int64, device="cuda") * cols
    row = {"shape": name, "rows": rows, "cols": cols, "n": n, "k": k, "dtype": dtype, "largest": largest,
           "launches": launches(x.itemsize * 8, rows, cols, k)}

    # rsx_segmented_topk through the engine (the Python helpers add allocation and a fill)
    eng = rsx.Engine(dtype, n, descending=largest)
    eng.set_stream(stream.cuda_stream)
    vout = torch.empty(rows * k, dtype=keys.dtype, device="cuda")
    iout = torch.empty(rows * k, dtype=torch.int32, device="cuda")
    ms = timed(lambda: eng.segmented_topk(keys.data_ptr(), n, offs.data_ptr(), rows, k, vout.data_ptr(), iout.data_ptr()), stream, iters, warmup)
    eng.sync()
    row["topk_engine_ms"] = ms
    row["topk_engine_gkeys"] = n / ms / 1e6
    # rsx_sort_from of the same n
    ms = timed(lambda: eng.sort_from(keys.data_ptr(), n), stream, iters, warmup)
    eng.sync()
    row["sort_from_ms"] = ms
    eng.close()

    if dtype in ("int32", "float32"):                           # torch types: the public helper and torch.topk on the same tensor
        t2 = keys.reshape(rows, cols)
        ms = timed(lambda: rsx.topk(t2, k, largest=largest), stream, iters, warmup)
        row["topk_ms"] = ms
        ms = timed(lambda: torch.topk(t2, k, dim=-1, largest=largest), stream, iters, warmup)
        row["torch_topk_ms"] = ms
        if rows > 1:
            ms = timed(lambda: rsx.sort_rows(t2, descending=largest)[0][:, :k], stream, iters, warmup)
            row["sort_slice_ms"] = ms
            row["sort_slice_note"] = "sort_rows + slice"
    else:
        row["topk_ms"] = None
        if dtype == "uint32":
            tw = keys.to(torch.int64) & 0xFFFFFFFF              # torch has no unsigned 32-bit topk: widened
            ms = timed(lambda: torch.topk(tw, k, largest=largest), stream, iters, warmup)
            row["torch_topk_ms"] = ms
            row["torch_note"] = "int64 keys (uint32 widened)"
            del tw
        else:
            row["torch_topk_ms"] = None                         # no unsigned 64-bit topk in torch
    if "sort_slice_ms" not in row:
        seng = rsx.Engine(dtype, n, descending=largest)
        seng.set_stream(stream.cuda_stream)
        sout = torch.empty_like(keys)
        ms = timed(lambda: seng.segmented_sort(keys.data_ptr(), n, offs.data_ptr(), rows, sout.data_ptr()), stream, iters, warmup)
        seng.sync()
        seng.close()
        del sout
        row["sort_slice_ms"] = ms
        row["sort_slice_note"] = "segmented_sort (no payload) + slice"
    row["vs_sort_from"] = row["topk_engine_ms"] / row["sort_from_ms"]
    row["vs_sort_slice"] = row["topk_engine_ms"] / row["sort_slice_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(2026)
    rows = []
    for name, dtype, largest, r, c, k in SHAPES:
        if args.only and args.only != name:
            continue
        row = run_shape(name, dtype, largest, r, c, k, args.iters, args.warmup, rng)
        row["device"] = rsx.device_name(0)
        print(json.dumps(row), flush=True)
        rows.append(row)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    fmt = lambda v: "—" if v is None else f"{v:.3f}"      # noqa: E731
    for r in rows:
        print(f"{r['shape']:>28}  topk {r['topk_engine_ms']:8.3f} ms ({fmt(r['topk_ms'])} helper) | torch.topk {fmt(r['torch_topk_ms'])} | "
              f"sort+slice {r['sort_slice_ms']:.3f} | sort_from {r['sort_from_ms']:.3f}  (x{r['vs_sort_from']:.2f}) | {r['launches']} launches",
              file=sys.stderr)


if __name__ == "__main__":
    main()
