#!/usr/bin/env python3
"""rsx_segmented_weighted_histogram against the reproducible composition it replaces and against the unweighted histogram of its keys, one
JSON line per row.

Bar (b), the requirement: call x (1 + margin) < composition, margin = max(10 %, 2 x the composition's spread).  The composition is what a
user of this library had before the call: the bin id of every key as a torch tensor (segment * B + bin; even form: torch arithmetic on
the keys, the segment's base precomputed outside the timing; edges form: rsx_segmented_search with RSX_SEARCH_RIGHT in the edges, then torch
arithmetic), then Engine.segmented_reduce_by_key with REDUCE_SUM over the weights on those ids as 32-bit keys (a full payload sort; its sums
come packed per distinct id, not per bin).
Bar (a), reported only: call <= rsx_segmented_histogram on the same keys x ((kb + wb) / kb) x (1 + max(10 %, 2 x its spread)).
torch.bincount(ids, weights=w) is reported beside the bars, without a bar (its float atomic sums are not reproducible).
Call and partners are measured alternately in one process, PAIR_REPEATS repeats, so that the partners' spreads are known; outputs are
preallocated.  Times are HIP events on one stream around each call, median of --iters after --warmup.

    python tools/whistogram_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/whistogram_bench.jsonl]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from unique_bench import PAIR_REPEATS, timed  # noqa: E402

rsx = load_package()
TORCH_DT = {"int32": torch.int32, "float32": torch.float32}

# name, key dtype, n, segments (None: NULL offsets) x length, bins, form
SHAPES = [
    ("1x2^28_i32_f32_B256", "int32", 1 << 28, None, 256, "even"),
    ("4096x2^16_i32_f32_B64", "int32", 1 << 28, (4096, 1 << 16), 64, "even"),
    ("2^20x50_i32_f32_B16", "int32", 50 << 20, (1 << 20, 50), 16, "even"),
    ("1x2^26_i32_f32_B50257", "int32", 1 << 26, None, 50257, "even"),
    ("1x2^26_f32_f32_edges_B1024", "float32", 1 << 26, None, 1024, "edges"),
]
FLOAT_RANGE = (-4.0, 4.0)
WEIGHT_EXP = 0                      # weights in [-1, 1)


def spread(xs):
    return (max(xs) - min(xs)) / float(np.median(xs))


def run_shape(name, dtype, n, segs, B, form, iters, warmup, gen):
    stream = torch.cuda.current_stream()
    tdt = TORCH_DT[dtype]
    kb, wb = 4, 4
    if form == "edges":
        keys = torch.randn(n, dtype=tdt, device="cuda", generator=gen)
    else:
        keys = torch.randint(0, B, (n,), dtype=tdt, device="cuda", generator=gen)
    weights = torch.rand(n, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1
    offs, nseg, seg_base = None, 1, None
    if segs is not None:
        nseg, length = segs
        offs = torch.arange(nseg + 1, dtype=torch.int64, device="cuda") * length
        seg_base = torch.repeat_interleave(torch.arange(nseg, dtype=torch.int32, device="cuda") * B, length)        # (outside the timing)
    base = {"shape": name, "form": form, "keys": dtype, "weights": "float32", "n": n, "segments": nseg, "bins": B}
    sums = torch.empty(nseg * B, dtype=torch.int64, device="cuda")
    counts = torch.empty(nseg * B, dtype=torch.int32, device="cuda")
    eng = rsx.Engine(dtype, 4096)
    eng.set_stream(stream.cuda_stream)
    optr = None if offs is None else offs.data_ptr()
    edges = None
    if form == "edges":
        edges = torch.linspace(*FLOAT_RANGE, B + 1, dtype=tdt, device="cuda")

    def call():
        eng.segmented_weighted_histogram(keys.data_ptr(), weights.data_ptr(), n, optr, nseg, B, sums.data_ptr(), rsx.WEIGHT_FLOAT32, WEIGHT_EXP, rsx.WHIST_SIGNED,
                                         d_edges=None if edges is None else edges.data_ptr())

    def unweighted():
        eng.segmented_histogram(keys.data_ptr(), n, optr, nseg, B, counts.data_ptr(), d_edges=None if edges is None else edges.data_ptr())

    sorter = rsx.Engine("int32", n, payload=True)
    sorter.set_stream(stream.cuda_stream)
    ids_out = torch.empty(n, dtype=torch.int32, device="cuda")
    run_off = torch.empty(2, dtype=torch.int64, device="cuda")
    vals_out = torch.empty(n, dtype=torch.float32, device="cuda")
    pos = torch.empty(n, dtype=torch.int32, device="cuda") if form == "edges" else None

    def bin_ids():
        if form == "edges":
            eng.segmented_search(edges.data_ptr(), B + 1, None, 1, keys.data_ptr(), n, None, pos.data_ptr(), right=True)
            b = pos - 1
            b = torch.where((b == B) & (keys == edges[-1]), B - 1, b)
            return torch.where((b >= 0) & (b < B), b, B)                  # (dropped keys: one id past the bins)
        return keys if seg_base is None else keys + seg_base

    def composition():
        ids = bin_ids()
        sorter.segmented_reduce_by_key(ids.data_ptr(), weights.data_ptr(), n, None, 1, rsx.REDUCE_SUM, rsx.VALUE_FLOAT32, ids_out.data_ptr(), run_off.data_ptr(),
                                       vals_out.data_ptr())
    what = "bin ids (torch" + (" after rsx_segmented_search" if form == "edges" else "") + ") + Engine.segmented_reduce_by_key sum on 32-bit ids"

    call_ms, hist_ms, comp_ms = [], [], []
    for _ in range(PAIR_REPEATS):                               # alternate the three, so that drift hits all
        hist_ms.append(timed(unweighted, stream, iters, warmup))
        call_ms.append(timed(call, stream, iters, warmup))
        comp_ms.append(timed(composition, stream, max(iters // 2, 3), 1))
    eng.sync()
    sorter.sync()
    c, h, q = float(np.median(call_ms)), float(np.median(hist_ms)), float(np.median(comp_ms))
    cb = n * (kb + wb) + 16 * nseg * B
    ratio = (kb + wb) / kb
    margin_a, margin_b = max(0.10, 2 * spread(hist_ms)), max(0.10, 2 * spread(comp_ms))
    row = {**base, "call_ms": c, "call_repeats_ms": call_ms, "call_model_bytes": cb, "call_tb_per_s": cb / c / 1e9,
           "composition": what, "composition_ms": q, "composition_repeats_ms": comp_ms, "composition_spread": spread(comp_ms), "margin_b": margin_b,
           "speedup": q / c, "bar_b": "met" if c * (1 + margin_b) < q else "missed",
           "histogram_ms": h, "histogram_repeats_ms": hist_ms, "histogram_spread": spread(hist_ms), "byte_ratio": ratio, "time_ratio": c / h,
           "margin_a": margin_a, "bar_a_bound_ms": h * ratio * (1 + margin_a), "bar_a": "met" if c <= h * ratio * (1 + margin_a) else "missed"}
    # the result: the sum of the masses is the sum of the quantised weights; torch's float sums beside it
    call()
    eng.sync()
    got = sums.to(torch.float64) * 2.0 ** (WEIGHT_EXP - 31)
    ids64 = bin_ids().to(torch.int64)
    want = torch.bincount(ids64, weights=weights.double(), minlength=nseg * B + 1)[:nseg * B]
    row["max_abs_difference_to_float64_bincount"] = float((got - want).abs().max())
    row["quantisation_bound"] = float(torch.bincount(ids64, minlength=nseg * B + 1)[:nseg * B].max()) * 2.0 ** (WEIGHT_EXP - 31)
    row["torch_bincount_weights_ms"] = timed(lambda: torch.bincount(ids64, weights=weights, minlength=nseg * B), stream, max(iters // 2, 3), 1)
    eng.close()
    sorter.close()
    del keys, weights, sums, counts, ids_out, vals_out, ids64, seg_base
    torch.cuda.empty_cache()
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = args.only.split(",") if args.only else None
    gen = torch.Generator(device="cuda").manual_seed(2026)
    out = []
    for shape in SHAPES:
        if only and shape[0] not in only:
            continue
        for row in run_shape(*shape, args.iters, args.warmup, gen):
            row["device"] = rsx.device_name(0)
            print(json.dumps(row), flush=True)
            out.append(row)
        if args.out:                                            # rewritten after every shape: a cut-short run keeps what it measured
            with open(args.out, "w") as f:
                for r in out:
                    f.write(json.dumps(r) + "\n")
    for r in out:
        print(f"{r['shape']:>28} call {r['call_ms']:.3f} ms ({r['call_tb_per_s']:.2f} TB/s) | composition {r['composition_ms']:.3f} (spread "
              f"{r['composition_spread']:.1%}) x{r['speedup']:.1f} -> (b) {r['bar_b']} | histogram {r['histogram_ms']:.3f} x{r['time_ratio']:.2f} measured, "
              f"x{r['byte_ratio']:.2f} by bytes -> (a) {r['bar_a']} | torch.bincount(weights) {r['torch_bincount_weights_ms']:.3f}", file=sys.stderr)


if __name__ == "__main__":
    main()
