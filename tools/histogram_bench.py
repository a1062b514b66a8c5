#!/usr/bin/env python3
"""rsx_segmented_histogram against the composition it replaces and against a device-to-device copy of its keys, one JSON line per row.

Bar (b), the requirement: call x (1 + margin) < composition, margin = max(10 %, 2 x the composition's spread).  The composition is what a
user of this library had before the call.  Even form: Engine.segmented_unique with counts on the same input (a full sort; its counts come
packed per distinct key, not per bin; only it is timed).  Edges form: rsx_segmented_search with RSX_SEARCH_RIGHT of the keys in the edges,
then torch arithmetic and torch.bincount on the bin.
Bar (a), reported: call <= copy x ((n kb + 8 S B) / (2 n kb)) x (1 + max(10 %, 2 x the copy's spread)); the copy is rsx_copy_on_device of the
keys (2 n kb bytes) on the same buffers.  torch.bincount / torch.histc are reported beside the bars without a bar where they apply.
Call and partners are measured alternately in one process, PAIR_REPEATS repeats, so that the partners' spreads are known; outputs are
preallocated.  Times are HIP events on one stream around each call, median of --iters after --warmup.

    python tools/histogram_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/histogram_bench.jsonl]
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
TORCH_DT = {"uint32": torch.int32, "int32": torch.int32, "uint64": torch.int64, "float32": torch.float32}

# name, key dtype, n, lengths (None: NULL offsets), bins, form, keys
SHAPES = [
    ("1x2^28_u32_B256", "uint32", 1 << 28, None, 256, "even", "uniform"),
    ("1x2^28_u32_B256_one_value", "uint32", 1 << 28, None, 256, "even", "equal"),
    ("1x2^28_f32_B4096", "float32", 1 << 28, None, 4096, "even", "normal"),
    ("1x2^27_u64_B2^16", "uint64", 1 << 27, None, 1 << 16, "even", "uniform"),
    ("256x8192_i32_B50257", "int32", 256 * 8192, lambda rng: np.full(256, 8192, dtype=np.int64), 50257, "even", "uniform"),
    ("2^16x4096_u32_B64", "uint32", 1 << 28, lambda rng: np.full(1 << 16, 4096, dtype=np.int64), 64, "even", "uniform"),
    ("2^20x50_u32_B16", "uint32", 50 << 20, lambda rng: np.full(1 << 20, 50, dtype=np.int64), 16, "even", "uniform"),
    ("zipf_2^26_u32_B256", "uint32", 1 << 26, lambda rng: zipf_lengths(1 << 26, rng), 256, "even", "uniform"),
    ("1x2^28_f32_edges_B64", "float32", 1 << 28, None, 64, "edges", "normal"),
    ("1x2^28_f32_edges_B4096", "float32", 1 << 28, None, 4096, "edges", "normal"),
]
FLOAT_RANGE = (-4.0, 4.0)


def spread(xs):
    return (max(xs) - min(xs)) / float(np.median(xs))


def run_shape(name, dtype, n, lens_fn, B, form, keyset, iters, warmup, rng, gen):
    stream = torch.cuda.current_stream()
    tdt = TORCH_DT[dtype]
    kb = torch.empty(0, dtype=tdt).element_size()
    if keyset == "normal":
        keys = torch.randn(n, dtype=tdt, device="cuda", generator=gen)
    elif keyset == "equal":
        keys = torch.full((n,), 77, dtype=tdt, device="cuda")
    else:
        keys = torch.randint(0, B, (n,), dtype=tdt, device="cuda", generator=gen)
    lens = None if lens_fn is None else lens_fn(rng)
    offs, nseg = None, 1
    if lens is not None:
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        nseg = len(lens)
    base = {"shape": name, "form": form, "keys": dtype, "keyset": keyset, "n": n, "segments": nseg, "bins": B}
    if nseg * B > 1 << 31:
        return [{**base, "skipped": "num_segments x num_bins exceeds 2^31"}]
    counts = torch.empty(nseg * B, dtype=torch.int32, device="cuda")
    spare = torch.empty(n, dtype=tdt, device="cuda")            # the copy's destination, the unique's keys
    eng = rsx.Engine(dtype, 4096)
    eng.set_stream(stream.cuda_stream)
    optr = None if offs is None else offs.data_ptr()
    edges = None
    lo, hi = (FLOAT_RANGE if tdt.is_floating_point else (0, 0))
    if form == "edges":
        edges = torch.linspace(lo, hi, B + 1, dtype=tdt, device="cuda")
        lo = hi = 0

    def call():
        eng.segmented_histogram(keys.data_ptr(), n, optr, nseg, B, counts.data_ptr(), d_edges=None if edges is None else edges.data_ptr(), lo=lo, hi=hi)

    def copy():
        assert eng.lib.rsx_copy_on_device(eng._h, C.c_void_p(spare.data_ptr()), C.c_void_p(keys.data_ptr()), n * kb) == 0

    if form == "even":
        sorter = rsx.Engine(dtype, n)
        sorter.set_stream(stream.cuda_stream)
        run_off = torch.empty(nseg + 1, dtype=torch.int64, device="cuda")
        ucounts = torch.empty(n, dtype=torch.int32, device="cuda")

        def composition():
            sorter.segmented_unique(keys.data_ptr(), n, optr, nseg, spare.data_ptr(), run_off.data_ptr(), ucounts.data_ptr())
        what = "Engine.segmented_unique with counts"
    else:
        sorter = None
        pos = torch.empty(n, dtype=torch.int32, device="cuda")
        last = edges[-1]

        def composition():
            eng.segmented_search(edges.data_ptr(), B + 1, None, 1, keys.data_ptr(), n, None, pos.data_ptr(), right=True)
            b = pos.to(torch.int64) - 1
            b = torch.where((b == B) & (keys == last), B - 1, b)
            return torch.bincount(b[(b >= 0) & (b < B)], minlength=B)
        what = "rsx_segmented_search (right) + torch arithmetic + torch.bincount"

    call_ms, copy_ms, comp_ms = [], [], []
    for _ in range(PAIR_REPEATS):                               # alternate the three, so that drift hits all
        copy_ms.append(timed(copy, stream, iters, warmup))
        call_ms.append(timed(call, stream, iters, warmup))
        comp_ms.append(timed(composition, stream, max(iters // 2, 3), 1))
    eng.sync()
    c, p, q = float(np.median(call_ms)), float(np.median(copy_ms)), float(np.median(comp_ms))
    cb, pb = n * kb + 8 * nseg * B, 2 * n * kb
    margin_a, margin_b = max(0.10, 2 * spread(copy_ms)), max(0.10, 2 * spread(comp_ms))
    row = {**base, "call_ms": c, "call_repeats_ms": call_ms, "call_model_bytes": cb, "call_tb_per_s": cb / c / 1e9,
           "composition": what, "composition_ms": q, "composition_repeats_ms": comp_ms, "composition_spread": spread(comp_ms), "margin_b": margin_b,
           "speedup": q / c, "bar_b": "met" if c * (1 + margin_b) < q else "missed",
           "copy_ms": p, "copy_repeats_ms": copy_ms, "copy_spread": spread(copy_ms), "copy_model_bytes": pb, "byte_ratio": cb / pb, "time_ratio": c / p,
           "margin_a": margin_a, "bar_a_bound_ms": p * cb / pb * (1 + margin_a), "bar_a": "met" if c <= p * cb / pb * (1 + margin_a) else "missed"}
    # the result, against torch where torch has the operation
    call()
    eng.sync()
    got = counts.to(torch.int64).reshape(nseg, B)
    if form == "edges":
        row["equals_composition"] = bool(torch.equal(got[0], composition()))
    if not tdt.is_floating_point:
        ids = keys.to(torch.int64) if offs is None else keys.to(torch.int64) + torch.repeat_interleave(torch.arange(nseg, device="cuda") * B, offs[1:] - offs[:-1])
        row["equals_torch_bincount"] = bool(torch.equal(got.reshape(-1), torch.bincount(ids, minlength=nseg * B)))
        if offs is None:
            row["torch_bincount_ms"] = timed(lambda: torch.bincount(keys, minlength=B), stream, max(iters // 2, 3), 1)
        else:
            row["torch_bincount_of_offset_ids_ms"] = timed(lambda: torch.bincount(ids, minlength=nseg * B), stream, max(iters // 2, 3), 1)
        del ids
    elif form == "even":
        row["torch_histc_ms"] = timed(lambda: torch.histc(keys, bins=B, min=lo, max=hi), stream, max(iters // 2, 3), 1)
        row["torch_histc_bins_that_differ"] = int((torch.histc(keys, bins=B, min=lo, max=hi).to(torch.int64) != got[0]).sum())
    eng.close()
    if sorter is not None:
        sorter.close()
    del keys, spare, counts
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
    rng = np.random.default_rng(2026)
    gen = torch.Generator(device="cuda").manual_seed(2026)
    out = []
    for shape in SHAPES:
        if only and shape[0] not in only:
            continue
        for row in run_shape(*shape, args.iters, args.warmup, rng, gen):
            row["device"] = rsx.device_name(0)
            print(json.dumps(row), flush=True)
            out.append(row)
        if args.out:                                            # rewritten after every shape: a cut-short run keeps what it measured
            with open(args.out, "w") as f:
                for r in out:
                    f.write(json.dumps(r) + "\n")
    for r in out:
        if "skipped" in r:
            print(f"{r['shape']:>28} skipped: {r['skipped']}", file=sys.stderr)
            continue
        extra = "".join(f" | {k.replace('_ms', '')} {r[k]:.3f}" for k in ("torch_bincount_ms", "torch_bincount_of_offset_ids_ms", "torch_histc_ms") if k in r)
        print(f"{r['shape']:>28} call {r['call_ms']:.3f} ms ({r['call_tb_per_s']:.2f} TB/s) | composition {r['composition_ms']:.3f} (spread "
              f"{r['composition_spread']:.1%}) x{r['speedup']:.1f} -> (b) {r['bar_b']} | copy {r['copy_ms']:.3f} x{r['time_ratio']:.2f} measured, "
              f"x{r['byte_ratio']:.2f} by bytes -> (a) {r['bar_a']}{extra}", file=sys.stderr)


if __name__ == "__main__":
    main()
