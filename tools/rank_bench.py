#!/usr/bin/env python3
"""rsx_segmented_rank against the compositions it replaces and against the sort it contains, one JSON line per shape and method.

Shapes: rows x cols of random float32 keys (standard normal), the last one a single row of random uint32 bits through the NULL-offsets
form.  Per method the call (outputs preallocated, no tie counts) and its partner, what a user of this library had before the call:
    average   segmented_sort (keys only) + segmented_searchsorted left and right + the add           bar (b), THE REQUIREMENT
    min       segmented_sort (keys only) + one segmented_searchsorted                                reported with a verdict
    max       segmented_sort (keys only) + one segmented_searchsorted (right)                        reported with a verdict
    ordinal   segmented_sort with an iota payload + torch scatter_                                   reported with a verdict
    dense     segmented_unique(return_inverse=True)                                                  reported with a verdict
Bar (b): call x (1 + margin) < partner, margin = max(10 %, 2 x the partner's spread).  Every answer of the call is compared with the
partner's, entry for entry.
Bar (a), reported only: call <= rsx_segmented_sort with payload on the same shape x the byte ratio of DESIGN 4s's model x
(1 + max(10 %, 2 x its spread)).
The call and its partners are measured alternately in one process, PAIR_REPEATS repeats, so that the partners' spreads are known.  Times
are HIP events on one stream around each call, median of --iters after --warmup.

    python tools/rank_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--methods average,min,...] [--out profiles/rank_bench.jsonl]
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

# name, rows, columns, dtype
SHAPES = [
    ("2^16x1000", 1 << 16, 1000, "float32"),
    ("4096x4096", 4096, 4096, "float32"),
    ("2^20x50", 1 << 20, 50, "float32"),
    ("1024x50257", 1024, 50257, "float32"),
    ("64x2^17", 64, 1 << 17, "float32"),
    ("1x2^28_u32", 1, 1 << 28, "uint32"),
]
METHODS = ["average", "min", "max", "ordinal", "dense"]
TILE = 4096


def spread(xs):
    return (max(xs) - min(xs)) / float(np.median(xs))


def model_bytes(rows, cols, kb, flat):
    """(rank, sort with payload) bytes of DESIGN 4s's model, no tie counts.  Small segments: the keys read, the ranks written, against
    keys and payload read and written.  Large segments: the chain of P 4-bit passes (histogram: keys; scatter: keys and payload in and
    out) for both; the rank adds the heads' pass over the keys, the write pass over keys and positions and one 4-byte store per key.
    The flat form runs 8-bit passes (one histogram pass up front) where the sort partner runs the segmented chain."""
    n = rows * cols
    if cols <= TILE and not flat:
        return n * (kb + 4), 2 * n * (kb + 4)
    passes = 2 * kb
    chain = passes * n * (kb + 2 * (kb + 4))
    extra = n * (kb + (kb + 4) + 4)
    if flat:
        return kb * (n * 2 * (kb + 4)) + n * kb + extra, chain
    return chain + extra, chain


def run_shape(name, rows, cols, dtype, methods, iters, warmup, gen):
    stream = torch.cuda.current_stream()
    n = rows * cols
    flat_form = rows == 1
    if dtype == "float32":
        flat = torch.randn(n, dtype=torch.float32, device="cuda", generator=gen)
    else:
        flat = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=gen).view(torch.uint32)
    offs = torch.arange(0, rows + 1, dtype=torch.int64, device="cuda") * cols
    iota = torch.arange(n, dtype=torch.int64, device="cuda").to(torch.int32)
    rel = (torch.arange(n, dtype=torch.int64, device="cuda") % cols)                  # the position inside the row of every sorted slot
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    scat = torch.zeros(n, dtype=torch.int64, device="cuda")
    k_out = torch.empty_like(flat)
    p_out = torch.empty(n, dtype=torch.int32, device="cuda")
    eng = rsx.Engine(dtype, n, payload=True)
    eng.set_stream(stream.cuda_stream)
    optr = None if flat_form else offs.data_ptr()

    def sort_payload():
        eng.segmented_sort(flat.data_ptr(), n, offs.data_ptr(), rows, k_out.data_ptr(), iota.data_ptr(), p_out.data_ptr())

    def partner_of(method):
        if method == "average":
            def f():
                s, _ = rsx.segmented_sort(flat, offs)
                return rsx.segmented_searchsorted(s, offs, flat, offs) + rsx.segmented_searchsorted(s, offs, flat, offs, right=True) - 1
            return f, "segmented_sort (keys only) + segmented_searchsorted left and right + add"
        if method in ("min", "max"):
            def f():
                s, _ = rsx.segmented_sort(flat, offs)
                return rsx.segmented_searchsorted(s, offs, flat, offs, right=method == "max") - (1 if method == "max" else 0)
            return f, "segmented_sort (keys only) + one segmented_searchsorted"
        if method == "ordinal":
            def f():
                _, perm = rsx.segmented_sort(flat, offs, iota)
                return scat.scatter_(0, perm.to(torch.int64), rel)
            return f, "segmented_sort with an iota payload + torch scatter_"

        def f():
            return rsx.segmented_unique(flat, offs, return_inverse=True)[2]
        return f, "segmented_unique(return_inverse=True)"

    rows_out = []
    rb, sb = model_bytes(rows, cols, flat.element_size(), flat_form)
    for method in methods:
        code = rsx.RANK_METHODS[method]
        partner, what = partner_of(method)

        def call():
            eng.segmented_rank(flat.data_ptr(), n, optr, rows, code, out.data_ptr())

        call_ms, sort_ms, comp_ms = [], [], []
        for _ in range(PAIR_REPEATS):                               # alternate the three, so that drift hits all
            sort_ms.append(timed(sort_payload, stream, iters, warmup))
            call_ms.append(timed(call, stream, iters, warmup))
            comp_ms.append(timed(partner, stream, max(iters // 2, 3), 1))
        eng.sync()
        c, h, q = float(np.median(call_ms)), float(np.median(sort_ms)), float(np.median(comp_ms))
        margin_a, margin_b = max(0.10, 2 * spread(sort_ms)), max(0.10, 2 * spread(comp_ms))
        out.zero_()
        call()
        eng.sync()
        same = bool(torch.equal(out.to(torch.int64) & 0xFFFFFFFF, partner()))
        bound_a = h * rb / sb * (1 + margin_a)
        row = {"shape": name, "rows": rows, "cols": cols, "dtype": dtype, "n": n, "method": method, "call_ms": c, "call_repeats_ms": call_ms,
               "call_spread": spread(call_ms), "call_gkeys_per_s": n / c / 1e6, "partner": what, "partner_ms": q, "partner_repeats_ms": comp_ms,
               "partner_spread": spread(comp_ms), "margin_b": margin_b, "speedup": q / c, "same_in_every_entry": same,
               "required": method == "average", "bar_b": "met" if same and c * (1 + margin_b) < q else "missed",
               "sort_payload_ms": h, "sort_payload_repeats_ms": sort_ms, "sort_payload_spread": spread(sort_ms), "model_rank_bytes": rb,
               "model_sort_bytes": sb, "margin_a": margin_a, "bar_a_bound_ms": bound_a, "bar_a": "met" if c <= bound_a else "missed"}
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    del flat, iota, rel, out, scat, k_out, p_out
    torch.cuda.empty_cache()
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = args.only.split(",") if args.only else None
    gen = torch.Generator(device="cuda").manual_seed(2026)
    out = []
    for shape in SHAPES:
        if only and shape[0] not in only:
            continue
        for row in run_shape(*shape, args.methods.split(","), args.iters, args.warmup, gen):
            row["device"] = rsx.device_name(0)
            out.append(row)
        if args.out:                                            # rewritten after every shape: a cut-short run keeps what it measured
            with open(args.out, "w") as f:
                for r in out:
                    f.write(json.dumps(r) + "\n")
    for r in out:
        print(f"{r['shape']:>12} {r['method']:>8} call {r['call_ms']:.3f} ms ({r['call_gkeys_per_s']:.1f} Gkeys/s) | partner {r['partner_ms']:.3f} (spread "
              f"{r['partner_spread']:.1%}) x{r['speedup']:.2f} same={r['same_in_every_entry']} -> (b) {r['bar_b']}{' REQUIRED' if r['required'] else ''} | "
              f"sort+payload {r['sort_payload_ms']:.3f}, bound {r['bar_a_bound_ms']:.3f} -> (a) {r['bar_a']}", file=sys.stderr)


if __name__ == "__main__":
    main()
