#!/usr/bin/env python3
"""rsx_segmented_expand against the composition a user has without it and against a device-to-device copy, one JSON line per shape.

Partners, each timed whole and alternated with the call in one process, PAIR_REPEATS repeats, so that every partner's spread is known:
  search   Engine.segmented_search with RSX_SEARCH_RIGHT of arange(n) in offsets[1:] (one bisection per output element: the segment
           ids); for the fill form a torch gather values[ids] follows
  compact  the packing shape only: Engine.segmented_compact of the padded batch with a prebuilt byte mask (what compact_rows runs)
  copy     rsx_copy_on_device of n * vb bytes (2 * n * vb bytes of traffic)
Bar (b), the requirement: the call is faster than the composition by more than max(10 %, 2 x that composition's spread).
Bar (a), reported: call <= copy x byte ratio x (1 + max(10 %, 2 x copy spread)); byte ratio = DESIGN.md §4m's bytes / (2 n vb): read
8 (S + 1) + vb S, plus 8 S and n vb in gather form; written n (vb + 4 + 4) over the outputs asked for.
torch.repeat_interleave(..., output_size=n) is reported without a bar.  Results are compared entry for entry.  Times are HIP events on
one stream around each call, median of --iters after --warmup; outputs are preallocated.  Shapes and partners are not tuned to move a
verdict: a missed bar is printed as missed.

    python tools/expand_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/expand_bench.jsonl]
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

SHAPES = [      # name, value dtype (None: segment ids only), form, lengths
    ("1x2^28_f32_fill", torch.float32, "fill", lambda rng: np.array([1 << 28], dtype=np.int64)),
    ("2^16x4096_f32_fill", torch.float32, "fill", lambda rng: np.full(1 << 16, 4096, dtype=np.int64)),
    ("2^22x64_f32_fill", torch.float32, "fill", lambda rng: np.full(1 << 22, 64, dtype=np.int64)),
    ("2^26x1_f32_fill", torch.float32, "fill", lambda rng: np.ones(1 << 26, dtype=np.int64)),
    ("zipf_2^26_i64_fill", torch.int64, "fill", lambda rng: zipf_lengths(1 << 26, rng)),
    ("4096x2^16_ids", None, "ids", lambda rng: np.full(4096, 1 << 16, dtype=np.int64)),
    ("2^16x4096_f32_pack", torch.float32, "pack", lambda rng: rng.integers(0, 4097, 1 << 16).astype(np.int64)),
    ("1x2^27_f64_fill", torch.float64, "fill", lambda rng: np.array([1 << 27], dtype=np.int64)),
]
PACK_WIDTH = 4096


def model_bytes(vb, n, nseg, form):
    if form == "ids":
        return 8 * (nseg + 1) + 4 * n
    if form == "pack":
        return 8 * (nseg + 1) + 8 * nseg + n * vb + n * vb
    return 8 * (nseg + 1) + vb * nseg + n * vb


def alternate(call, partners, stream, iters, warmup):
    """{name: [ms per repeat]} for the call and every partner, taken in turn"""
    times = {name: [] for name in ("call", *partners)}
    for _ in range(PAIR_REPEATS):
        for name, fn in partners.items():
            times[name].append(timed(fn, stream, iters, warmup))
        times["call"].append(timed(call, stream, iters, warmup))
    return times


def run_shape(name, vdt, form, lens, gen, iters, warmup):
    stream = torch.cuda.current_stream()
    nseg = len(lens)
    n = int(lens.sum())
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
    vb = 4 if vdt is None else torch.empty(0, dtype=vdt).element_size()
    eng = rsx.Engine("uint32", 4096)
    eng.set_stream(stream.cuda_stream)
    eng64 = rsx.Engine("int64", 4096)                                # the search's haystack is the int64 offsets
    eng64.set_stream(stream.cuda_stream)
    engines = [eng, eng64]
    partners, checks = {}, {}

    if form == "pack":
        src = torch.randn(nseg * PACK_WIDTH, dtype=vdt, device="cuda", generator=gen)
        starts = torch.arange(0, nseg, dtype=torch.int64, device="cuda") * PACK_WIDTH
        out = torch.empty(n, dtype=vdt, device="cuda")

        def call():
            eng.segmented_expand(src.data_ptr(), src.numel(), vb, offs.data_ptr(), nseg, n, starts.data_ptr(), out.data_ptr(), None, None)

        mask = (torch.arange(PACK_WIDTH, device="cuda")[None, :] < torch.from_numpy(lens).cuda()[:, None]).to(torch.uint8).reshape(-1).contiguous()
        row_offs = torch.arange(0, nseg + 1, dtype=torch.int64, device="cuda") * PACK_WIDTH
        ceng = rsx.Engine("float32", 4096)
        ceng.set_stream(stream.cuda_stream)
        engines.append(ceng)
        packed = torch.empty(src.numel(), dtype=vdt, device="cuda")      # (the compaction's output is sized by its input)
        kept = torch.empty(nseg + 1, dtype=torch.int64, device="cuda")

        def compact():
            ceng.segmented_compact(src.data_ptr(), src.numel(), row_offs.data_ptr(), nseg, mask.data_ptr(), None, packed.data_ptr(), None, kept.data_ptr())

        partners["compact"] = compact
        checks["compact"] = lambda: torch.equal(out.view(torch.int32), packed[:n].view(torch.int32)) and torch.equal(kept, offs)
        copy_src = out
    else:
        values = None if vdt is None else (torch.randn(nseg, dtype=vdt, device="cuda", generator=gen) if vdt.is_floating_point
                                           else torch.randint(-1000, 1000, (nseg,), dtype=vdt, device="cuda", generator=gen))
        out = None if vdt is None else torch.empty(n, dtype=vdt, device="cuda")
        ids = torch.empty(n, dtype=torch.int32, device="cuda") if vdt is None else None

        def call():
            eng.segmented_expand(None if values is None else values.data_ptr(), nseg if values is not None else 0, vb, offs.data_ptr(), nseg, n, None,
                                 None if out is None else out.data_ptr(), None if ids is None else ids.data_ptr(), None)

        queries = torch.arange(n, dtype=torch.int64, device="cuda")
        found = torch.empty(n, dtype=torch.int32, device="cuda")
        gathered = None if vdt is None else torch.empty(n, dtype=vdt, device="cuda")
        hay = offs[1:].clone()                                      # (a copy: the search wants its keys 16-byte aligned)

        def search():
            eng64.segmented_search(hay.data_ptr(), nseg, None, 1, queries.data_ptr(), n, None, found.data_ptr(), right=True)
            if gathered is not None:
                torch.index_select(values, 0, found, out=gathered)

        partners["search"] = search
        checks["search"] = (lambda: torch.equal(ids, found)) if vdt is None else (lambda: torch.equal(out.view(torch.int32), gathered.view(torch.int32)))
        copy_src = out if out is not None else ids

    scratch = torch.empty_like(copy_src)
    cbytes = copy_src.numel() * copy_src.element_size()

    def copy():
        assert eng.lib.rsx_copy_on_device(eng._h, C.c_void_p(scratch.data_ptr()), C.c_void_p(copy_src.data_ptr()), cbytes) == 0

    partners["copy"] = copy
    times = alternate(call, partners, stream, iters, warmup)
    for e in engines:
        e.sync()
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    row = {"shape": name, "form": form, "n": n, "segments": nseg, "values": "none" if vdt is None else str(vdt).replace("torch.", ""),
           "call_ms": med["call"], "call_repeats_ms": times["call"], "call_spread": spread["call"]}
    for p in partners:
        row[p + "_ms"], row[p + "_repeats_ms"], row[p + "_spread"] = med[p], times[p], spread[p]
        if p == "copy":
            continue
        margin = max(0.10, 2 * spread[p])
        row[p + "_margin"] = margin
        row["bar_b_" + p] = "met" if med["call"] < med[p] / (1 + margin) else "missed"
        row[p + "_equal"] = bool(checks[p]())
    pb, cb = 2 * cbytes, model_bytes(vb, n, nseg, form)
    margin = max(0.10, 2 * spread["copy"])
    row.update(byte_ratio=cb / pb, time_ratio=med["call"] / med["copy"], bar_a_bound_ms=med["copy"] * cb / pb * (1 + margin),
               call_tb_per_s=cb / med["call"] / 1e9, copy_tb_per_s=pb / med["copy"] / 1e9)
    row["bar_a"] = "met" if med["call"] <= row["bar_a_bound_ms"] else "missed"
    if form == "fill":                                              # report only
        reps = torch.from_numpy(lens).cuda()
        row["torch_ms"] = timed(lambda: torch.repeat_interleave(values, reps, output_size=n), stream, max(iters // 2, 3), 1)
    elif form == "ids":
        reps = torch.from_numpy(lens).cuda()
        row["torch_ms"] = timed(lambda: torch.repeat_interleave(reps, output_size=n), stream, max(iters // 2, 3), 1)
    for e in engines:
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
    for name, vdt, form, lens_fn in SHAPES:
        if only and name not in only:
            continue
        row = run_shape(name, vdt, form, lens_fn(rng), gen, args.iters, args.warmup)
        row["device"] = rsx.device_name(0)
        print(json.dumps(row), flush=True)
        out.append(row)
        torch.cuda.empty_cache()
        if args.out:                                                # rewritten after every row: a cut-short run keeps what it measured
            with open(args.out, "w") as f:
                for r in out:
                    f.write(json.dumps(r) + "\n")
    for r in out:
        parts = "".join(f" | {p} {r[p + '_ms']:.3f} (b) {r['bar_b_' + p]} equal {r[p + '_equal']}" for p in ("search", "compact") if p + "_ms" in r)
        print(f"{r['shape']:>20}  call {r['call_ms']:.3f} ms ({r['call_tb_per_s']:.2f} TB/s) | copy {r['copy_ms']:.3f} x{r['time_ratio']:.2f} measured, "
              f"x{r['byte_ratio']:.2f} by bytes (a) {r['bar_a']}{parts}" + (f" | torch {r['torch_ms']:.3f}" if "torch_ms" in r else ""), file=sys.stderr)


if __name__ == "__main__":
    main()
