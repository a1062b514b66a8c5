#!/usr/bin/env python3
"""rsx_segmented_scan (inclusive sum) against a device-to-device copy of its values and against the composition it replaces, one JSON line
per shape.

Partner: rsx_copy_on_device of the values into the scan's output buffer (2 * n * vb bytes), on the same buffers.  Call and partner are
measured alternately in one process, PAIR_REPEATS repeats of the pair, so that the partner's spread is known.
Bar (a): call <= copy x (model bytes of the call / (2 * n * vb)) x (1 + max(10 %, 2 x copy spread)); the byte model is DESIGN.md §4f's:
3 * n * vb (two reads and one write of the values) + 2 * n * kb with keys (two reads) + the per-tile partials.
Bar (b), the ragged int64 shape: call < torch.cumsum(v) - repeat_interleave(base, lengths), the composition callers write today.
torch.cumsum on the flat and row shapes is reported without a bar.
Times are HIP events on one stream around each call, median of --iters after --warmup.

    python tools/scan_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/scan_bench.jsonl]
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

SHAPES = [      # name, value dtype, n, key runs (None: no keys), lengths (None: NULL offsets), rows for torch.cumsum (None: flat)
    ("1x2^28_f32", torch.float32, 1 << 28, None, None, None),
    ("1x2^27_f64", torch.float64, 1 << 27, None, None, None),
    ("1x2^28_i32_u32keys_2^16runs", torch.int32, 1 << 28, 1 << 16, None, None),
    ("1x2^28_i32_u32keys_nruns", torch.int32, 1 << 28, "n", None, None),
    ("4096x2^16_f32", torch.float32, 1 << 28, None, lambda rng: np.full(4096, 1 << 16, dtype=np.int64), (4096, 1 << 16)),
    ("2^16x4096_f32", torch.float32, 1 << 28, None, lambda rng: np.full(1 << 16, 4096, dtype=np.int64), (1 << 16, 4096)),
    ("zipf_2^26_i64", torch.int64, 1 << 26, None, lambda rng: zipf_lengths(1 << 26, rng), None),
]
KIND = {torch.int32: rsx.VALUE_INT32, torch.int64: rsx.VALUE_INT64, torch.float32: rsx.VALUE_FLOAT32, torch.float64: rsx.VALUE_FLOAT64}


def scan_model_bytes(vb, kb, n):
    """the values read twice and written once, the keys read twice, per tile a tail, a carry (both read back) and a flag word"""
    tiles = (n + TILE - 1) // TILE
    return 3 * n * vb + 2 * n * kb + tiles * (4 * vb + 8)


def run_shape(name, vdt, n, runs, lens_fn, rows, iters, warmup, rng, gen):
    stream = torch.cuda.current_stream()
    vb = torch.empty(0, dtype=vdt).element_size()
    if vdt.is_floating_point:
        values = torch.randn(n, dtype=vdt, device="cuda", generator=gen)
    else:
        values = torch.randint(-1000, 1000, (n,), dtype=vdt, device="cuda", generator=gen)
    keys, kb = None, 0
    if runs is not None:
        kb = 4
        if runs == "n":                                         # about n runs: random keys, neighbours almost always differ
            keys = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device="cuda", generator=gen)
        else:                                                   # `runs` runs of equal length
            keys = torch.arange(n, dtype=torch.int32, device="cuda") // (n // runs)
    lens = None if lens_fn is None else lens_fn(rng)
    offs, nseg = None, 1
    if lens is not None:
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        nseg = len(lens)
    out = torch.empty_like(values)
    eng = rsx.Engine("uint32", 4096)
    eng.set_stream(stream.cuda_stream)
    kptr, optr = (None if keys is None else keys.data_ptr()), (None if offs is None else offs.data_ptr())

    def scan():
        eng.segmented_scan(kptr, values.data_ptr(), n, optr, nseg, rsx.REDUCE_SUM, KIND[vdt], out.data_ptr())

    def partner():
        rc = eng.lib.rsx_copy_on_device(eng._h, C.c_void_p(out.data_ptr()), C.c_void_p(values.data_ptr()), n * vb)
        assert rc == 0

    scan_ms, par = [], []
    for _ in range(PAIR_REPEATS):                               # alternate the two, so that drift hits both
        par.append(timed(partner, stream, iters, warmup))
        scan_ms.append(timed(scan, stream, iters, warmup))
    eng.sync()
    p_ms, s_ms = float(np.median(par)), float(np.median(scan_ms))
    spread = (max(par) - min(par)) / p_ms
    pb, sb = 2 * n * vb, scan_model_bytes(vb, kb, n)
    margin = max(0.10, 2 * spread)
    bound = p_ms * sb / pb * (1 + margin)
    row = {"shape": name, "op": "sum", "n": n, "segments": nseg, "values": str(vdt).replace("torch.", ""), "keys": None if keys is None else "uint32",
           "key_runs": None if runs is None else (n if runs == "n" else runs), "scan_ms": s_ms, "scan_repeats_ms": scan_ms,
           "partner": "rsx_copy_on_device of the values", "partner_ms": p_ms, "partner_repeats_ms": par, "partner_spread": spread,
           "partner_model_bytes": pb, "scan_model_bytes": sb, "byte_ratio": sb / pb, "time_ratio": s_ms / p_ms, "margin": margin,
           "bar_a_bound_ms": bound, "bar_a": "met" if s_ms <= bound else "missed", "scan_tb_per_s": sb / s_ms / 1e9, "copy_tb_per_s": pb / p_ms / 1e9}
    if keys is None and lens is not None and not vdt.is_floating_point:      # bar (b): the composition on the ragged integer shape
        tl = torch.from_numpy(lens).cuda()

        def composition():
            c = torch.cumsum(values, 0)
            base = torch.zeros(nseg, dtype=vdt, device="cuda")
            starts = offs[:-1]
            nz = starts > 0
            base[nz] = c[starts[nz] - 1]
            return c - torch.repeat_interleave(base, tl)

        want = composition()
        scan()
        eng.sync()
        row["composition_equal"] = bool(torch.equal(want, out))
        row["composition_ms"] = timed(composition, stream, max(iters // 2, 3), 1)
        row["bar_b"] = "met" if s_ms < row["composition_ms"] else "missed"
    if keys is None and (lens is None or rows is not None):                   # report only: torch.cumsum on the flat and row shapes
        x = values if rows is None else values.reshape(rows)
        row["torch_cumsum_ms"] = timed(lambda: torch.cumsum(x, -1), stream, max(iters // 2, 3), 1)
    eng.close()
    del values, out, keys
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
    for name, vdt, n, runs, lens_fn, rows in SHAPES:
        if only and name not in only:
            continue
        for row in run_shape(name, vdt, n, runs, lens_fn, rows, args.iters, args.warmup, rng, gen):
            row["device"] = rsx.device_name(0)
            print(json.dumps(row), flush=True)
            out.append(row)
        if args.out:                                            # rewritten after every shape: a cut-short run keeps what it measured
            with open(args.out, "w") as f:
                for r in out:
                    f.write(json.dumps(r) + "\n")
    for r in out:
        extra = "".join(f" | {k.replace('_ms', '')} {r[k]:.3f}" for k in ("composition_ms", "torch_cumsum_ms") if k in r)
        print(f"{r['shape']:>28}  scan {r['scan_ms']:.3f} ms ({r['scan_tb_per_s']:.2f} TB/s) | copy {r['partner_ms']:.3f} (spread {r['partner_spread']:.1%}) | "
              f"x{r['time_ratio']:.2f} measured, x{r['byte_ratio']:.2f} by bytes -> (a) {r['bar_a']}{extra}"
              + (f" -> (b) {r['bar_b']}" if "bar_b" in r else ""), file=sys.stderr)


if __name__ == "__main__":
    main()
