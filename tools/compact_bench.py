#!/usr/bin/env python3
"""rsx_segmented_compact against a device-to-device copy of its keys and against the composition it replaces, one JSON line per row.

Partner: rsx_copy_on_device of the keys into the call's key output (2 * n * kb bytes), on the same buffers.  Call and partner are measured
alternately in one process, PAIR_REPEATS repeats of the pair, so that the partner's spread is known.
Bar (a): call <= copy x (model bytes of the call / (2 * n * kb)) x (1 + max(10 %, 2 x copy spread)); the byte model is DESIGN.md §4h's:
the predicate's input in both passes (2 n mask bytes, or 2 n keys), n keys once more in mask form, and what is written at the MEASURED
keep rate r: r n keys (n in partition mode) and as many index words where the index is asked for.
Bar (b): call < composition / (1 + margin), the composition being what a user of this library has today: rsx.segmented_scan of the flags as
int32 (exclusive, no offsets), a torch scatter_ of the kept keys to those positions, a gather of the scan at the offsets for the counts.
torch.masked_select / torch.nonzero are reported beside the bars without a bar.
Times are HIP events on one stream around each call, median of --iters after --warmup.

    python tools/compact_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/compact_bench.jsonl]
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
RATES = [(1, 64), (1, 2), (63, 64)]

MASK_SHAPES = [      # name, key dtype, n, lengths (None: NULL offsets), also in partition mode
    ("1x2^28_u32", "uint32", 1 << 28, None, True),
    ("1x2^27_u64", "uint64", 1 << 27, None, False),
    ("4096x2^16_u32", "uint32", 1 << 28, lambda rng: np.full(4096, 1 << 16, dtype=np.int64), True),
    ("2^16x4096_f32", "float32", 1 << 28, lambda rng: np.full(1 << 16, 4096, dtype=np.int64), False),
    ("zipf_2^26_u32", "uint32", 1 << 26, lambda rng: zipf_lengths(1 << 26, rng), False),
]
BOUND_SHAPE = ("1024x50257_f32_desc", "float32", 1024, 50257, 50)      # rows, cols, the rank the bounds come from
TORCH_DT = {"uint32": torch.int32, "uint64": torch.int64, "float32": torch.float32}


def model_bytes(n, kb, bound, rate, partition, index):
    """DESIGN.md §4h"""
    tiles = (n + TILE - 1) // TILE
    reads = 2 * n * kb if bound else 2 * n + n * kb
    written = n if partition else rate * n
    return reads + written * (kb + (4 if index else 0)) + 3 * 4 * tiles


def measure(eng, stream, call, keys, kout, n, kb, iters, warmup):
    def partner():
        rc = eng.lib.rsx_copy_on_device(eng._h, C.c_void_p(kout.data_ptr()), C.c_void_p(keys.data_ptr()), n * kb)
        assert rc == 0

    call_ms, par = [], []
    for _ in range(PAIR_REPEATS):                               # alternate the two, so that drift hits both
        par.append(timed(partner, stream, iters, warmup))
        call_ms.append(timed(call, stream, iters, warmup))
    eng.sync()
    return call_ms, par


def verdict_row(base, call_ms, par, n, kb, bound, rate, partition, index):
    p_ms, c_ms = float(np.median(par)), float(np.median(call_ms))
    spread = (max(par) - min(par)) / p_ms
    pb, cb = 2 * n * kb, model_bytes(n, kb, bound, rate, partition, index)
    margin = max(0.10, 2 * spread)
    limit = p_ms * cb / pb * (1 + margin)
    return {**base, "n": n, "keep_rate": rate, "partition": partition, "index": index, "call_ms": c_ms, "call_repeats_ms": call_ms,
            "partner": "rsx_copy_on_device of the keys", "partner_ms": p_ms, "partner_repeats_ms": par, "partner_spread": spread,
            "partner_model_bytes": pb, "call_model_bytes": cb, "byte_ratio": cb / pb, "time_ratio": c_ms / p_ms, "margin": margin,
            "bar_a_bound_ms": limit, "bar_a": "met" if c_ms <= limit else "missed", "call_tb_per_s": cb / c_ms / 1e9, "copy_tb_per_s": pb / p_ms / 1e9}


def run_mask_shape(name, dtype, n, lens_fn, also_partition, iters, warmup, rng, gen):
    stream = torch.cuda.current_stream()
    tdt = TORCH_DT[dtype]
    kb = torch.empty(0, dtype=tdt).element_size()
    keys = torch.randn(n, dtype=tdt, device="cuda", generator=gen) if tdt.is_floating_point else \
        torch.randint(-2**31, 2**31 - 1, (n,), dtype=tdt, device="cuda", generator=gen)
    lens = None if lens_fn is None else lens_fn(rng)
    offs, nseg = None, 1
    if lens is not None:
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        nseg = len(lens)
    kout = torch.empty(n + 1, dtype=tdt, device="cuda")        # (one slot more: the composition's dump slot)
    koff = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
    eng = rsx.Engine(dtype, 4096)
    eng.set_stream(stream.cuda_stream)
    optr = None if offs is None else offs.data_ptr()
    rows = []
    for num, den in RATES:
        mask = torch.randint(0, den, (n,), device="cuda", generator=gen) < num
        for partition in ((False, True) if also_partition else (False,)):
            def call():
                eng.segmented_compact(keys.data_ptr(), n, optr, nseg, mask.data_ptr(), None, kout.data_ptr(), None, koff.data_ptr(), partition=partition)

            call_ms, par = measure(eng, stream, call, keys, kout, n, kb, iters, warmup)
            call()
            eng.sync()
            rate = int(koff[-1]) / n
            row = verdict_row({"shape": name, "form": "mask", "keys": dtype, "segments": nseg, "nominal_rate": f"{num}/{den}"}, call_ms, par, n, kb, False,
                              rate, partition, False)
            if not partition:
                want = torch.masked_select(keys, mask)
                row["equals_masked_select"] = bool(torch.equal(kout[:want.numel()], want))
                flags = mask.to(torch.int32)
                off_idx = torch.tensor([0, n], dtype=torch.int64, device="cuda") if offs is None else offs

                def composition():
                    pos = rsx.segmented_scan(flags, None, exclusive=True)
                    idx = torch.where(mask, pos, torch.full_like(pos, n)).to(torch.int64)
                    kout.scatter_(0, idx, keys)
                    return torch.where(off_idx < n, pos[off_idx.clamp(max=n - 1)].to(torch.int64), (pos[-1] + flags[-1]).to(torch.int64))

                counts = composition()
                row["composition_equal"] = bool(torch.equal(kout[:want.numel()], want)) and bool(torch.equal(counts, koff))
                row["composition_ms"] = timed(composition, stream, max(iters // 2, 3), 1)
                row["bar_b"] = "met" if row["call_ms"] * (1 + row["margin"]) < row["composition_ms"] else "missed"
                row["torch_masked_select_ms"] = timed(lambda: torch.masked_select(keys, mask), stream, max(iters // 2, 3), 1)
                row["torch_nonzero_ms"] = timed(lambda: torch.nonzero(mask), stream, max(iters // 2, 3), 1)
                del want, flags, counts
            rows.append(row)
        del mask
    eng.close()
    del keys, kout
    torch.cuda.empty_cache()
    return rows


def run_bound_shape(iters, warmup, gen):
    name, dtype, nrows, cols, rank = BOUND_SHAPE
    stream = torch.cuda.current_stream()
    n, kb = nrows * cols, 4
    keys = torch.softmax(torch.randn((nrows, cols), device="cuda", generator=gen), dim=-1).reshape(-1).contiguous()
    offs = torch.arange(0, nrows + 1, device="cuda", dtype=torch.int64) * cols
    bounds = rsx.segmented_select(keys, offs, torch.full((nrows,), rank, dtype=torch.int64, device="cuda"), descending=True)[0].reshape(-1).contiguous()
    kout = torch.empty(n, dtype=torch.float32, device="cuda")
    iout = torch.empty(n, dtype=torch.int32, device="cuda")
    koff = torch.zeros(nrows + 1, dtype=torch.int64, device="cuda")
    eng = rsx.Engine(dtype, 4096, descending=True)
    eng.set_stream(stream.cuda_stream)
    rows = []
    for index in (False, True):
        def call():
            eng.segmented_compact(keys.data_ptr(), n, offs.data_ptr(), nrows, None, bounds.data_ptr(), kout.data_ptr(), iout.data_ptr() if index else None,
                                  koff.data_ptr())

        call_ms, par = measure(eng, stream, call, keys, kout, n, kb, iters, warmup)
        call()
        eng.sync()
        kept = int(koff[-1])
        row = verdict_row({"shape": name, "form": "bound", "keys": dtype, "segments": nrows, "bounds": f"segmented_select at rank {rank}"}, call_ms, par, n, kb,
                          True, kept / n, False, index)
        row["kept_per_row_min"] = int((koff[1:] - koff[:-1]).min())
        rows.append(row)
    eng.close()
    return rows


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

    for name, dtype, n, lens_fn, also_partition in MASK_SHAPES:
        if only and name not in only:
            continue
        emit(run_mask_shape(name, dtype, n, lens_fn, also_partition, args.iters, args.warmup, rng, gen))
    if not only or BOUND_SHAPE[0] in only:
        emit(run_bound_shape(args.iters, args.warmup, gen))
    for r in out:
        extra = "".join(f" | {k.replace('_ms', '')} {r[k]:.3f}" for k in ("composition_ms", "torch_masked_select_ms", "torch_nonzero_ms") if k in r)
        mode = ("partition" if r["partition"] else "compact") + (" +index" if r["index"] else "")
        print(f"{r['shape']:>22} {r['form']:5} {mode:16} keep {r['keep_rate']:.4f}  call {r['call_ms']:.3f} ms ({r['call_tb_per_s']:.2f} TB/s) | copy "
              f"{r['partner_ms']:.3f} (spread {r['partner_spread']:.1%}) | x{r['time_ratio']:.2f} measured, x{r['byte_ratio']:.2f} by bytes -> (a) {r['bar_a']}{extra}"
              + (f" -> (b) {r['bar_b']}" if "bar_b" in r else ""), file=sys.stderr)


if __name__ == "__main__":
    main()
