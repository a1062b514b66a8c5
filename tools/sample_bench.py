#!/usr/bin/env python3
"""rsx_segmented_sample against the composition it replaces and against one pass over the same bytes, one JSON line per row.

Shapes: float32 dyadic rows (multiples of 2^-24 that sum to 1), the probabilities their own weights, a descending engine, a top-p bound
per row (p a multiple of 1/1024; the threshold is rsx.top_p's, computed outside the timing), R uniforms per row.
Bar (b), the requirement: call x (1 + margin) < composition, margin = max(10 %, 2 x the composition's spread).  The composition is what a
user of this library had before the call: compact_rows(bound, descending=True, return_index=True) -> the nucleus masses and their int64
cumsum -> the target rule in torch -> segmented_searchsorted -> a gather of the columns.  The call and the composition must give the same
index in every slot, which is checked.
Bar (a), reported only: call <= rsx_segmented_reduce (sum, float32) over the same weights x (1 + max(10 %, 2 x its spread)): one pass over
the same bytes.  torch.multinomial(probs, R, replacement=True) on the unfiltered rows is reported beside the bars, without a bar.
The call and its partners are measured alternately in one process, PAIR_REPEATS repeats, so that the partners' spreads are known; the
call's outputs are preallocated.  Times are HIP events on one stream around each call, median of --iters after --warmup.

    python tools/sample_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/sample_bench.jsonl]
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

# name, rows, columns, R
SHAPES = [
    ("1024x50257_R1", 1024, 50257, 1),
    ("1024x50257_R16", 1024, 50257, 16),
    ("64x2^17_R1", 64, 1 << 17, 1),
    ("4096x4096_R1", 4096, 4096, 1),
    ("1x2^28_R1", 1, 1 << 28, 1),
    ("2^20x50_R1", 1 << 20, 50, 1),
]
UNITS = 1 << 24


def spread(xs):
    return (max(xs) - min(xs)) / float(np.median(xs))


def dyadic_rows(rows, cols, gen):
    """[rows, cols] float32 on the device: non-negative multiples of 2^-24 that sum to 1 in every row (the gaps of sorted random cuts)."""
    cuts = torch.randint(0, UNITS + 1, (rows, cols - 1), dtype=torch.int32, device="cuda", generator=gen).sort(dim=1).values
    edges = torch.cat([torch.zeros((rows, 1), dtype=torch.int32, device="cuda"), cuts, torch.full((rows, 1), UNITS, dtype=torch.int32, device="cuda")], dim=1)
    del cuts
    return ((edges[:, 1:] - edges[:, :-1]).to(torch.float32) / float(UNITS)).contiguous()


def run_shape(name, rows, cols, R, iters, warmup, gen):
    stream = torch.cuda.current_stream()
    n = rows * cols
    probs = dyadic_rows(rows, cols, gen)
    flat = probs.reshape(-1)
    offs = torch.arange(0, rows + 1, dtype=torch.int64, device="cuda") * cols
    p = torch.randint(1, 1025, (rows,), device="cuda", generator=gen).to(torch.float64) / 1024.0
    u = torch.rand((rows, R), dtype=torch.float64, device="cuda", generator=gen)
    thr = rsx.top_p(probs, p)[0].contiguous()                     # (outside the timing)
    idx = torch.full((rows, R), -1, dtype=torch.int32, device="cuda")
    sums = torch.empty(rows, dtype=torch.float32, device="cuda")
    eng = rsx.Engine("float32", 4096, descending=True)
    eng.set_stream(stream.cuda_stream)
    voff = torch.arange(0, rows + 1, dtype=torch.int64, device="cuda") * R

    def call():
        eng.segmented_sample(flat.data_ptr(), None, n, offs.data_ptr(), rows, thr.data_ptr(), u.data_ptr(), R, rsx.WSELECT_FRACTION, rsx.WEIGHT_FLOAT32, 0,
                             idx.data_ptr())

    def reduce():
        eng.segmented_reduce(flat.data_ptr(), n, offs.data_ptr(), rows, rsx.REDUCE_SUM, rsx.VALUE_FLOAT32, sums.data_ptr())

    def composition():
        nucleus, row_off, col = rsx.compact_rows(probs, bound=thr, descending=True, return_index=True)
        m = (nucleus.to(torch.float64) * float(1 << 31)).to(torch.int64)              # exact for multiples of 2^-24
        run = torch.cat([m.new_zeros(1), torch.cumsum(m, 0)])
        base = run[row_off[:-1]]
        total = run[row_off[1:]] - base
        td = total.to(torch.float64)[:, None]
        x = td * u
        T = torch.where(x > 1.0, torch.where(x >= td, total[:, None], torch.ceil(x).to(torch.int64)), torch.ones_like(x, dtype=torch.int64))
        pos = rsx.segmented_searchsorted(run[1:], row_off, (T + base[:, None]).reshape(-1), voff).reshape(rows, R)
        return col[row_off[:-1, None] + pos]

    what = "compact_rows(bound, return_index) + int64 cumsum + target rule + segmented_searchsorted + gather"
    call_ms, red_ms, comp_ms = [], [], []
    for _ in range(PAIR_REPEATS):                               # alternate the three, so that drift hits all
        red_ms.append(timed(reduce, stream, iters, warmup))
        call_ms.append(timed(call, stream, iters, warmup))
        comp_ms.append(timed(composition, stream, max(iters // 2, 3), 1))
    eng.sync()
    c, h, q = float(np.median(call_ms)), float(np.median(red_ms)), float(np.median(comp_ms))
    margin_a, margin_b = max(0.10, 2 * spread(red_ms)), max(0.10, 2 * spread(comp_ms))
    call()
    eng.sync()
    same = bool(torch.equal(idx.to(torch.int64), composition()))
    row = {"shape": name, "rows": rows, "cols": cols, "R": R, "n": n, "call_ms": c, "call_repeats_ms": call_ms, "call_spread": spread(call_ms),
           "call_gb_per_s": n * 4 / c / 1e6, "composition": what, "composition_ms": q, "composition_repeats_ms": comp_ms,
           "composition_spread": spread(comp_ms), "margin_b": margin_b, "speedup": q / c, "same_index_in_every_slot": same,
           "bar_b": "met" if same and c * (1 + margin_b) < q else "missed",
           "reduce_ms": h, "reduce_repeats_ms": red_ms, "reduce_spread": spread(red_ms), "time_ratio": c / h, "margin_a": margin_a,
           "bar_a_bound_ms": h * (1 + margin_a), "bar_a": "met" if c <= h * (1 + margin_a) else "missed",
           "torch_multinomial_ms": timed(lambda: torch.multinomial(probs, R, replacement=True), stream, max(iters // 2, 3), 1) if cols < (1 << 24) else None}
    eng.close()
    del probs, flat, idx, u
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
        tm = r["torch_multinomial_ms"]
        print(f"{r['shape']:>16} call {r['call_ms']:.3f} ms ({r['call_gb_per_s']:.0f} GB/s) | composition {r['composition_ms']:.3f} (spread "
              f"{r['composition_spread']:.1%}) x{r['speedup']:.1f} same={r['same_index_in_every_slot']} -> (b) {r['bar_b']} | reduce {r['reduce_ms']:.3f} "
              f"x{r['time_ratio']:.2f} -> (a) {r['bar_a']} | torch.multinomial {'-' if tm is None else f'{tm:.3f}'}", file=sys.stderr)


if __name__ == "__main__":
    main()
