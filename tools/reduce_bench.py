#!/usr/bin/env python3
"""rsx_segmented_reduce_by_key (sum, with counts) against the payload sort of the same input and against the composition it replaces, one
JSON line per (shape, keys).

Partner: rsx_sort_from with an iota payload for one segment (NULL offsets), rsx_segmented_sort with payload otherwise.  Call and partner are
measured alternately in one process, PAIR_REPEATS repeats of the pair, so that the partner's spread is known.
Bar (a): call <= partner x (model bytes of the call / model bytes of the partner) x (1 + max(10 %, 2 x partner spread)); the byte model is
DESIGN.md §4e's (the gather of the values counted as one 32-byte sector per 4-byte value, 64 bytes per 8-byte value).
Bar (b): call < composition = Engine.segmented_unique with inverse and counts into preallocated outputs, then torch.zeros(runs).index_add_
(the inverse map of a segment shape is made global with a precomputed segment-id tensor first).
A consecutive-mode row on sorted input is reported with its achieved TB/s by the byte model, without a bar.
Times are HIP events on one stream around each call, median of --iters after --warmup.

    python tools/reduce_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/reduce_bench.jsonl]
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
from unique_bench import PAIR_REPEATS, make_keys, sort_bytes, timed, zipf_lengths  # noqa: E402

rsx = load_package()

SHAPES = [      # name, key dtype, value dtype, n, lengths (None: NULL offsets), keysets
    ("1x2^28_u32_f32", "uint32", torch.float32, 1 << 28, None, ["random_bits", "2^16_values"]),
    ("1x2^27_u64_f64", "uint64", torch.float64, 1 << 27, None, ["random_bits"]),
    ("4096x2^16_u32_f32", "uint32", torch.float32, 1 << 28, lambda rng: np.full(4096, 1 << 16, dtype=np.int64), ["random_bits"]),
    ("2^16x4096_u32_f32", "uint32", torch.float32, 1 << 28, lambda rng: np.full(1 << 16, 4096, dtype=np.int64), ["random_bits"]),
    ("zipf_2^26_u32_f32", "uint32", torch.float32, 1 << 26, lambda rng: zipf_lengths(1 << 26, rng), ["random_bits"]),
]
KIND = {torch.float32: rsx.VALUE_FLOAT32, torch.float64: rsx.VALUE_FLOAT64}


def sector(vb):
    return 32 if vb == 4 else 64


def reduce_extra_bytes(kb, vb, n, runs, tiles, sorted_mode):
    """what the reduce passes move beyond the sort.  The count pass reads the keys; the tile pass reads the keys again, the
    positions (sorted mode) and one sector per gathered value (consecutive mode: the values as a stream), stores key + value + head
    position per run and three partial words per tile; the carry reads those; the counts pass reads the head positions and stores the counts."""
    values = n * (4 + sector(vb)) if sorted_mode else n * vb
    return n * (kb + kb) + values + runs * (kb + vb + 4 + 4 + 4) + tiles * 2 * (2 * vb + 4)


def run_shape(name, dtype, vdt, n, lens_fn, keyset, iters, warmup, rng, gen):
    stream = torch.cuda.current_stream()
    kb = 8 if dtype.endswith("64") else 4
    vb = 8 if vdt == torch.float64 else 4
    keys = make_keys(dtype, n, keyset, gen)
    values = torch.randn(n, dtype=vdt, device="cuda", generator=gen)
    lens = None if lens_fn is None else lens_fn(rng)
    offs, seg_of, nseg = None, None, 1
    if lens is not None:
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        nseg = len(lens)
        seg_of = torch.repeat_interleave(torch.arange(nseg, dtype=torch.int32, device="cuda"), torch.from_numpy(lens).cuda())
    optr = None if offs is None else offs.data_ptr()
    iota = torch.arange(n, dtype=torch.int32, device="cuda")
    ukeys = torch.empty_like(keys)
    red = torch.empty_like(values)
    uoff = torch.empty(nseg + 1, dtype=torch.int64, device="cuda")
    cnt, inv = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    sk, sp = torch.empty_like(keys), torch.empty_like(iota)
    eng = rsx.Engine(dtype, n, payload=True)
    eng.set_stream(stream.cuda_stream)

    def reduce():
        eng.segmented_reduce_by_key(keys.data_ptr(), values.data_ptr(), n, optr, nseg, rsx.REDUCE_SUM, KIND[vdt], ukeys.data_ptr(), uoff.data_ptr(),
                                    red.data_ptr(), cnt.data_ptr())

    def partner():
        if offs is None:
            eng.sort_from(keys.data_ptr(), n, iota.data_ptr())
        else:
            eng.segmented_sort(keys.data_ptr(), n, optr, nseg, sk.data_ptr(), iota.data_ptr(), sp.data_ptr())

    reduce()
    eng.sync()
    runs = int(uoff[-1].item())

    def composition():
        eng.segmented_unique(keys.data_ptr(), n, optr, nseg, ukeys.data_ptr(), uoff.data_ptr(), cnt.data_ptr(), None, inv.data_ptr())
        gid = inv if seg_of is None else inv + uoff[seg_of].to(torch.int32)
        return torch.zeros(runs, dtype=vdt, device="cuda").index_add_(0, gid, values)

    red_ms, par = [], []
    for _ in range(PAIR_REPEATS):                               # alternate the two, so that drift hits both
        par.append(timed(partner, stream, iters, warmup))
        red_ms.append(timed(reduce, stream, iters, warmup))
    comp = timed(composition, stream, max(iters // 2, 3), 1)
    eng.sync()
    eng.close()
    p_ms, r_ms = float(np.median(par)), float(np.median(red_ms))
    spread = (max(par) - min(par)) / p_ms
    tiles = (n + 4095) // 4096
    pb = sort_bytes(kb, 4, lens, n)
    rb = pb + reduce_extra_bytes(kb, vb, n, runs, tiles, True)
    margin = max(0.10, 2 * spread)
    bound = p_ms * rb / pb * (1 + margin)
    torch.cuda.empty_cache()
    return [{"shape": name, "keys": keyset, "op": "sum", "n": n, "segments": nseg, "dtype": dtype, "values": str(vdt).replace("torch.", ""), "runs": runs,
             "reduce_ms": r_ms, "reduce_repeats_ms": red_ms, "partner": ("rsx_sort_from" if offs is None else "rsx_segmented_sort") + " + iota payload",
             "partner_ms": p_ms, "partner_repeats_ms": par, "partner_spread": spread, "partner_model_bytes": pb, "reduce_model_bytes": rb,
             "byte_ratio": rb / pb, "time_ratio": r_ms / p_ms, "margin": margin, "bar_a_bound_ms": bound, "bar_a": "met" if r_ms <= bound else "missed",
             "composition_ms": comp, "bar_b": "met" if r_ms < comp else "missed"}]


def run_consecutive(iters, warmup, gen):
    """1 x 2^28 uint32 keys, float32 values, sorted input, consecutive mode: model bytes over time (report only)"""
    stream = torch.cuda.current_stream()
    n = 1 << 28
    rows = []
    for keyset in ("random_bits", "2^16_values"):
        keys = torch.sort(make_keys("uint32", n, keyset, gen)).values
        values = torch.randn(n, dtype=torch.float32, device="cuda", generator=gen)
        ukeys, red = torch.empty_like(keys), torch.empty_like(values)
        uoff = torch.empty(2, dtype=torch.int64, device="cuda")
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        eng = rsx.Engine("uint32", n)
        eng.set_stream(stream.cuda_stream)
        ms = timed(lambda: eng.segmented_reduce_by_key(keys.data_ptr(), values.data_ptr(), n, None, 1, rsx.REDUCE_SUM, rsx.VALUE_FLOAT32, ukeys.data_ptr(),
                                                       uoff.data_ptr(), red.data_ptr(), cnt.data_ptr(), consecutive=True), stream, iters, warmup)
        eng.sync()
        runs = int(uoff[-1].item())
        eng.close()
        moved = reduce_extra_bytes(4, 4, n, runs, (n + 4095) // 4096, False)
        rows.append({"shape": "1x2^28_u32_f32_sorted_consecutive", "keys": keyset, "op": "sum", "n": n, "runs": runs, "reduce_ms": ms, "model_bytes": moved,
                     "tb_per_s": moved / ms / 1e9, "share_of_8tb_s": moved / ms / 1e9 / 8.0})
        del keys, values, ukeys, red, cnt
        torch.cuda.empty_cache()
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

    for name, dtype, vdt, n, lens_fn, keysets in SHAPES:
        if only and name not in only:
            continue
        for keyset in keysets:
            emit(run_shape(name, dtype, vdt, n, lens_fn, keyset, args.iters, args.warmup, rng, gen))
    if not only or "consecutive" in only:
        emit(run_consecutive(args.iters, args.warmup, gen))
    for r in out:
        if "partner_ms" in r:
            print(f"{r['shape']:>18} {r['keys']:>12}  reduce {r['reduce_ms']:.3f} ms | {r['partner']} {r['partner_ms']:.3f} (spread {r['partner_spread']:.1%}) | "
                  f"x{r['time_ratio']:.2f} measured, x{r['byte_ratio']:.2f} by bytes -> (a) {r['bar_a']} | composition {r['composition_ms']:.3f} -> (b) {r['bar_b']}",
                  file=sys.stderr)


if __name__ == "__main__":
    main()
