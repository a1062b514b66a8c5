#!/usr/bin/env python3
"""rsx_segmented_reduce against the compositions it replaces and against a device-to-device copy of its values, one JSON line per shape
and op.

Partners, each timed whole and alternated with the call in one process, PAIR_REPEATS repeats, so that every partner's spread is known:
  by_key   Engine.segmented_reduce_by_key in consecutive mode on a zero uint32 key array of n entries, engine of capacity n (sum, max)
  scan     Engine.segmented_scan followed by a torch gather at off[s+1] - 1 (sum, max)
  topk     Engine.segmented_topk with k = 1 on a descending float32 engine of capacity n (argmax on float32)
  copy     rsx_copy_on_device of the values (2 * n * vb bytes)
Bar (b), the requirement: the call is faster than each composition by more than max(10 %, 2 x that composition's spread).
Bar (a), reported: call <= copy x byte ratio x (1 + max(10 %, 2 x copy spread)), byte ratio = (n vb + S (vb [+ 4]) + 16 (S + 1) +
partials) / (2 n vb); the partials are DESIGN.md §4l's: per tile a lead, a tail (both read back) and three words.
The results are compared entry for entry where the compositions define them: non-empty segments, integers and max.  torch.sum / amax /
argmax are reported without a bar.  Times are HIP events on one stream around each call, median of --iters after --warmup; outputs are
preallocated.

    python tools/segreduce_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/segreduce_bench.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from unique_bench import PAIR_REPEATS, timed, zipf_lengths  # noqa: E402

rsx = load_package()
TILE = 4096

SHAPES = [      # name, value dtype, n, ops, lengths (None: NULL offsets), rows for torch (None: flat or ragged)
    ("1x2^28_f32", torch.float32, 1 << 28, ("sum",), None, None),
    ("1x2^27_f64", torch.float64, 1 << 27, ("sum",), None, None),
    ("4096x2^16_f32", torch.float32, 1 << 28, ("sum",), lambda rng: np.full(4096, 1 << 16, dtype=np.int64), (4096, 1 << 16)),
    ("2^16x4096_f32", torch.float32, 1 << 28, ("max", "argmax"), lambda rng: np.full(1 << 16, 4096, dtype=np.int64), (1 << 16, 4096)),
    ("2^22x32_i32", torch.int32, 1 << 27, ("sum",), lambda rng: np.full(1 << 22, 32, dtype=np.int64), (1 << 22, 32)),
    ("1024x50257_f32", torch.float32, 1024 * 50257, ("argmax",), lambda rng: np.full(1024, 50257, dtype=np.int64), (1024, 50257)),
    ("zipf_2^26_i64", torch.int64, 1 << 26, ("sum",), lambda rng: zipf_lengths(1 << 26, rng), None),
]
KIND = {torch.int32: rsx.VALUE_INT32, torch.int64: rsx.VALUE_INT64, torch.float32: rsx.VALUE_FLOAT32, torch.float64: rsx.VALUE_FLOAT64}
OPCODE = {"sum": rsx.REDUCE_SUM, "max": rsx.REDUCE_MAX, "argmax": rsx.REDUCE_ARGMAX}


def model_bytes(vb, n, nseg, arg, offsets):
    tiles = (n + TILE - 1) // TILE
    return n * vb + nseg * (vb + (4 if arg else 0)) + (16 * (nseg + 1) if offsets else 0) + tiles * (4 * vb + (24 if arg else 8))


def alternate(call, partners, stream, iters, warmup):
    """{name: [ms per repeat]} for the call and every partner, taken in turn"""
    times = {name: [] for name in ("call", *partners)}
    for _ in range(PAIR_REPEATS):
        for name, fn in partners.items():
            times[name].append(timed(fn, stream, iters, warmup))
        times["call"].append(timed(call, stream, iters, warmup))
    return times


def run_op(name, vdt, n, op, lens, rows, values, offs, iters, warmup):
    stream = torch.cuda.current_stream()
    vb = values.element_size()
    nseg = 1 if lens is None else len(lens)
    arg = op == "argmax"
    optr = None if offs is None else offs.data_ptr()
    eng = rsx.Engine("uint32", 4096)
    eng.set_stream(stream.cuda_stream)
    vout = torch.empty(nseg, dtype=vdt, device="cuda")
    iout = torch.empty(nseg, dtype=torch.int32, device="cuda") if arg else None

    def call():
        eng.segmented_reduce(values.data_ptr(), n, optr, nseg, OPCODE[op], KIND[vdt], vout.data_ptr(), None if iout is None else iout.data_ptr())

    def copy():
        assert eng.lib.rsx_copy_on_device(eng._h, C.c_void_p(scratch.data_ptr()), C.c_void_p(values.data_ptr()), n * vb) == 0

    scratch = torch.empty_like(values)                              # the copy's target and the scan's output
    partners, engines, checks = {"copy": copy}, [], {}
    ends = (torch.tensor([n - 1], device="cuda") if offs is None else offs[1:] - 1).clamp_(min=0)
    live = None if offs is None else (offs[1:] > offs[:-1])
    if not arg:
        big = rsx.Engine("uint32", n)
        big.set_stream(stream.cuda_stream)
        engines.append(big)
        zeros = torch.zeros(n, dtype=torch.int32, device="cuda")
        kout = torch.empty(nseg + 1, dtype=torch.int32, device="cuda")
        roff = torch.empty(nseg + 1, dtype=torch.int64, device="cuda")
        packed = torch.empty(nseg + 1, dtype=vdt, device="cuda")

        def by_key():
            big.segmented_reduce_by_key(zeros.data_ptr(), values.data_ptr(), n, optr, nseg, OPCODE[op], KIND[vdt], kout.data_ptr(), roff.data_ptr(),
                                        packed.data_ptr(), consecutive=True)

        gathered = torch.empty(nseg, dtype=vdt, device="cuda")

        def scan():
            eng.segmented_scan(None, values.data_ptr(), n, optr, nseg, OPCODE[op], KIND[vdt], scratch.data_ptr())
            torch.index_select(scratch, 0, ends, out=gathered)

        partners.update(by_key=by_key, scan=scan)
        checks["by_key"] = lambda: packed[:int(live.sum()) if live is not None else 1]
        checks["scan"] = lambda: gathered if live is None else gathered[live]
    elif vdt == torch.float32:
        desc = rsx.Engine("float32", n, payload=True, descending=True)
        desc.set_stream(stream.cuda_stream)
        engines.append(desc)
        tk = torch.empty(nseg, dtype=vdt, device="cuda")
        ti = torch.empty(nseg, dtype=torch.int32, device="cuda")
        one = offs if offs is not None else torch.tensor([0, n], dtype=torch.int64, device="cuda")

        def topk():
            desc.segmented_topk(values.data_ptr(), n, one.data_ptr(), nseg, 1, tk.data_ptr(), ti.data_ptr())

        partners["topk"] = topk
        checks["topk"] = lambda: ti if live is None else ti[live]

    times = alternate(call, partners, stream, iters, warmup)
    for e in (eng, *engines):
        e.sync()
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    row = {"shape": name, "op": op, "n": n, "segments": nseg, "values": str(vdt).replace("torch.", ""), "call_ms": med["call"],
           "call_repeats_ms": times["call"]}
    mine = (iout if arg else vout) if live is None else (iout if arg else vout)[live]
    exact = arg or op == "max" or not vdt.is_floating_point
    for p in partners:
        row[p + "_ms"], row[p + "_repeats_ms"], row[p + "_spread"] = med[p], times[p], spread[p]
        if p == "copy":
            continue
        margin = max(0.10, 2 * spread[p])
        row[p + "_margin"] = margin
        row["bar_b_" + p] = "met" if med["call"] < med[p] / (1 + margin) else "missed"
        if exact:
            row[p + "_equal"] = bool(torch.equal(mine, checks[p]()))
    pb, cb = 2 * n * vb, model_bytes(vb, n, nseg, arg, offs is not None)
    margin = max(0.10, 2 * spread["copy"])
    row.update(byte_ratio=cb / pb, time_ratio=med["call"] / med["copy"], bar_a_bound_ms=med["copy"] * cb / pb * (1 + margin),
               call_tb_per_s=cb / med["call"] / 1e9, copy_tb_per_s=pb / med["copy"] / 1e9)
    row["bar_a"] = "met" if med["call"] <= row["bar_a_bound_ms"] else "missed"
    if lens is None or rows is not None:                            # report only: torch on the flat and row shapes
        x = values if rows is None else values.reshape(rows)
        fn = {"sum": torch.sum, "max": torch.amax, "argmax": torch.argmax}[op]
        row["torch_ms"] = timed((lambda: fn(x)) if rows is None else (lambda: fn(x, -1)), stream, max(iters // 2, 3), 1)
    for e in (eng, *engines):
        e.close()
    return row


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
    for name, vdt, n, ops, lens_fn, rows in SHAPES:
        if only and name not in only:
            continue
        if vdt.is_floating_point:
            values = torch.randn(n, dtype=vdt, device="cuda", generator=gen)
        else:
            values = torch.randint(-1000, 1000, (n,), dtype=vdt, device="cuda", generator=gen)
        lens = None if lens_fn is None else lens_fn(rng)
        offs = None if lens is None else torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        for op in ops:
            row = run_op(name, vdt, n, op, lens, rows, values, offs, args.iters, args.warmup)
            row["device"] = rsx.device_name(0)
            print(json.dumps(row), flush=True)
            out.append(row)
            torch.cuda.empty_cache()
            if args.out:                                            # rewritten after every row: a cut-short run keeps what it measured
                with open(args.out, "w") as f:
                    for r in out:
                        f.write(json.dumps(r) + "\n")
        del values
        torch.cuda.empty_cache()
    for r in out:
        parts = "".join(f" | {p} {r[p + '_ms']:.3f} (b) {r['bar_b_' + p]}" for p in ("by_key", "scan", "topk") if p + "_ms" in r)
        print(f"{r['shape']:>16} {r['op']:>6}  call {r['call_ms']:.3f} ms ({r['call_tb_per_s']:.2f} TB/s) | copy {r['copy_ms']:.3f} "
              f"x{r['time_ratio']:.2f} measured, x{r['byte_ratio']:.2f} by bytes (a) {r['bar_a']}{parts}"
              + (f" | torch {r['torch_ms']:.3f}" if "torch_ms" in r else ""), file=sys.stderr)


if __name__ == "__main__":
    main()
