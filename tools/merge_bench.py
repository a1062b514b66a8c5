#!/usr/bin/env python3
"""rsx_segmented_merge against the composition it replaces and against a device-to-device copy of its keys, one JSON line per shape.

Bar (b), a requirement: call < composition / (1 + max(10 %, 2 x the composition's spread)).  The composition is what a user of this
library has without the call: the two inputs already concatenated per segment (A_s ++ B_s, formed outside the timed region) and sorted
with rsx_segmented_sort (rsx_sort_from for one segment), with an iota payload where the merge gives payload or index.  Only the sort is
timed.  Call and composition are measured alternately in one process, PAIR_REPEATS repeats of the pair, so that the partner's spread is
known.  The results must be equal entry for entry: keys by bits, and the sort's payload (a position in the concatenated buffer) with the
merge's index + the segment's start (and with the merge's payload output, whose inputs are that iota split in two).
Bar (a), reported as met or missed: call <= copy x (model bytes of the call / (2 n kb)) x (1 + max(10 %, 2 x the copy's spread)), the copy
being rsx_copy_on_device of the n = na + nb concatenated keys into the call's key output; the byte model is DESIGN.md §4i's:
n (2 kb [+ 8 with payload] [+ 4 with index]) + 8 per tile.
torch.sort(torch.cat([a, b], -1), stable=True) is reported beside the bars without a bar (shapes with equal rows only).
Times are HIP events on one stream around each call, median of --iters after --warmup.  Keys are non-negative, so that torch's signed
order is the unsigned engine's.

    python tools/merge_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/merge_bench.jsonl]
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


def zipf_pair(total, rng):
    """Zipf lengths, `total` in all, dealt to the two sides: a third of the segments keep A empty, a third B, the rest are split at random"""
    lens = zipf_lengths(total, rng)
    kind = rng.integers(0, 3, lens.size)
    la = np.where(kind == 0, 0, np.where(kind == 1, lens, (lens * rng.random(lens.size)).astype(np.int64)))
    return la.astype(np.int64), (lens - la).astype(np.int64)


SHAPES = [      # name, engine dtype, descending, (la, lb) per segment as a function of rng (None, (na, nb): NULL offsets), payload + index
    ("1x(2^27+2^27)_u32", "uint32", False, (None, (1 << 27, 1 << 27)), False),
    ("1x(2^28-2^20,2^20)_u32", "uint32", False, (None, ((1 << 28) - (1 << 20), 1 << 20)), False),
    ("1x(2^26+2^26)_u64", "uint64", False, (None, (1 << 26, 1 << 26)), False),
    ("1x(2^27+2^27)_u32_payload_index", "uint32", False, (None, (1 << 27, 1 << 27)), True),
    ("4096x(2^15+2^15)_u32", "uint32", False, (lambda rng: (np.full(4096, 1 << 15), np.full(4096, 1 << 15)), None), False),
    ("2^16x(2048+2048)_f32_desc", "float32", True, (lambda rng: (np.full(1 << 16, 2048), np.full(1 << 16, 2048)), None), False),
    ("2^20x(50+50)_f32_desc", "float32", True, (lambda rng: (np.full(1 << 20, 50), np.full(1 << 20, 50)), None), False),
    ("zipf_2^26_u32", "uint32", False, (lambda rng: zipf_pair(1 << 26, rng), None), False),
]
TORCH_DT = {"uint32": torch.int32, "uint64": torch.int64, "float32": torch.float32}


def model_bytes(n, kb, payload, index):
    """DESIGN.md §4i"""
    return n * (2 * kb + (8 if payload else 0) + (4 if index else 0)) + 8 * ((n + TILE - 1) // TILE)


def random_keys(n, tdt, gen):
    if tdt.is_floating_point:
        return torch.randn(n, dtype=tdt, device="cuda", generator=gen)
    return torch.randint(0, torch.iinfo(tdt).max, (n,), dtype=tdt, device="cuda", generator=gen)


def sorted_side(n, lens, tdt, dtype, descending, gen):
    """n random keys, every segment sorted in the engine's order"""
    keys = random_keys(n, tdt, gen)
    if lens is None:
        return torch.sort(keys, descending=descending)[0]
    if len(set(lens.tolist())) == 1 and lens[0] > 0:
        return torch.sort(keys.reshape(len(lens), int(lens[0])), dim=-1, descending=descending)[0].reshape(-1).contiguous()
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
    return rsx.segmented_sort(keys, offs, descending=descending)[0]         # (int32 / int64 engines: the unsigned order on non-negative keys)


def run_shape(name, dtype, descending, lengths, extras, iters, warmup, rng, gen):
    stream = torch.cuda.current_stream()
    tdt = TORCH_DT[dtype]
    kb = torch.empty(0, dtype=tdt).element_size()
    lens_fn, flat = lengths
    if lens_fn is None:
        la = lb = None
        na, nb = flat
        nseg = 1
    else:
        la, lb = (np.asarray(x, dtype=np.int64) for x in lens_fn(rng))
        na, nb, nseg = int(la.sum()), int(lb.sum()), len(la)
    n = na + nb
    a, b = sorted_side(na, la, tdt, dtype, descending, gen), sorted_side(nb, lb, tdt, dtype, descending, gen)
    aoff = boff = ooff_ref = None
    if la is not None:
        aoff = torch.from_numpy(np.concatenate([[0], np.cumsum(la)]).astype(np.int64)).cuda()
        boff = torch.from_numpy(np.concatenate([[0], np.cumsum(lb)]).astype(np.int64)).cuda()
        ooff_ref = aoff + boff
    # the concatenation A_s ++ B_s of every segment, formed outside the timed region: position of every element in it
    if la is None:
        cat = torch.cat([a, b])
    else:
        seg_a = torch.repeat_interleave(torch.arange(nseg, device="cuda"), torch.from_numpy(la).cuda())
        seg_b = torch.repeat_interleave(torch.arange(nseg, device="cuda"), torch.from_numpy(lb).cuda())
        pos_a = torch.arange(na, device="cuda") - aoff[seg_a] + ooff_ref[seg_a]
        pos_b = torch.arange(nb, device="cuda") - boff[seg_b] + ooff_ref[seg_b] + (aoff[seg_b + 1] - aoff[seg_b])
        cat = torch.empty(n, dtype=tdt, device="cuda")
        cat[pos_a] = a
        cat[pos_b] = b
        del seg_a, seg_b
    iota = torch.arange(n, dtype=torch.int32, device="cuda") if extras else None
    pa = pb = None
    if extras:
        pa, pb = (iota[:na].contiguous(), iota[na:].contiguous()) if la is None else (pos_a.to(torch.int32), pos_b.to(torch.int32))
    kout = torch.empty(n, dtype=tdt, device="cuda")
    pout = torch.empty(n, dtype=torch.int32, device="cuda") if extras else None
    iout = torch.empty(n, dtype=torch.int32, device="cuda") if extras else None
    ooff = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
    eng = rsx.Engine(dtype, 4096, descending=descending)
    eng.set_stream(stream.cuda_stream)
    ptr = lambda t: None if t is None else t.data_ptr()

    def call():
        eng.segmented_merge(a.data_ptr(), na, ptr(aoff), b.data_ptr(), nb, ptr(boff), nseg, kout.data_ptr(), ptr(iout), ooff.data_ptr(),
                            d_a_payload=ptr(pa), d_b_payload=ptr(pb), d_payload_out=ptr(pout))

    # the composition: the library's sort of the concatenation, on an engine of its own
    seng = rsx.Engine(dtype, n, payload=extras, descending=descending)
    seng.set_stream(stream.cuda_stream)
    skeys = torch.empty(n, dtype=tdt, device="cuda")
    sperm = torch.empty(n, dtype=torch.int32, device="cuda") if extras else None
    if la is None:
        def composition():
            seng.sort_from(cat.data_ptr(), n, ptr(iota))
    else:
        def composition():
            seng.segmented_sort(cat.data_ptr(), n, ooff_ref.data_ptr(), nseg, skeys.data_ptr(), ptr(iota), ptr(sperm))

    def copy():
        assert eng.lib.rsx_copy_on_device(eng._h, C.c_void_p(kout.data_ptr()), C.c_void_p(cat.data_ptr()), n * kb) == 0

    call_ms, comp_ms, copy_ms = [], [], []
    for _ in range(PAIR_REPEATS):                               # alternate, so that drift hits all
        comp_ms.append(timed(composition, stream, iters, warmup))
        copy_ms.append(timed(copy, stream, iters, warmup))
        call_ms.append(timed(call, stream, iters, warmup))
    # equality, entry for entry
    call()
    composition()
    eng.sync()
    seng.sync()
    if la is None:
        seng.copy_result(skeys.data_ptr(), ptr(sperm))
        seng.sync()
    bits = lambda t: t.view(torch.int32 if kb == 4 else torch.int64)
    equal = bool(torch.equal(bits(kout), bits(skeys)))
    if ooff_ref is not None:
        equal = equal and bool(torch.equal(ooff, ooff_ref))
    if extras:
        equal = equal and bool(torch.equal(pout, sperm)) and bool(torch.equal(iout, sperm))        # (one segment: index = position in the concatenation)
    c_ms, s_ms, p_ms = float(np.median(call_ms)), float(np.median(comp_ms)), float(np.median(copy_ms))
    s_spread, p_spread = (max(comp_ms) - min(comp_ms)) / s_ms, (max(copy_ms) - min(copy_ms)) / p_ms
    b_margin, a_margin = max(0.10, 2 * s_spread), max(0.10, 2 * p_spread)
    cb, pb_bytes = model_bytes(n, kb, extras, extras), 2 * n * kb
    limit = p_ms * cb / pb_bytes * (1 + a_margin)
    row = {"shape": name, "keys": dtype, "descending": descending, "segments": nseg, "na": na, "nb": nb, "payload": extras, "index": extras,
           "call_ms": c_ms, "call_repeats_ms": call_ms,
           "composition": ("rsx_sort_from" if la is None else "rsx_segmented_sort") + " of the concatenation" + (" with an iota payload" if extras else ""),
           "composition_ms": s_ms, "composition_repeats_ms": comp_ms, "composition_spread": s_spread, "bar_b_margin": b_margin,
           "speedup": s_ms / c_ms, "bar_b": "met" if c_ms * (1 + b_margin) < s_ms else "missed", "equal_to_composition": equal,
           "copy_ms": p_ms, "copy_repeats_ms": copy_ms, "copy_spread": p_spread, "copy_model_bytes": pb_bytes, "call_model_bytes": cb,
           "byte_ratio": cb / pb_bytes, "time_ratio": c_ms / p_ms, "bar_a_margin": a_margin, "bar_a_bound_ms": limit,
           "bar_a": "met" if c_ms <= limit else "missed", "call_tb_per_s": cb / c_ms / 1e9, "copy_tb_per_s": pb_bytes / p_ms / 1e9}
    if la is None or len(set(la.tolist())) == 1:
        rows_a, rows_b = (a, b) if la is None else (a.reshape(nseg, -1), b.reshape(nseg, -1))
        torch_sort = lambda: torch.sort(torch.cat([rows_a, rows_b], -1), dim=-1, stable=True, descending=descending)
        row["torch_sort_of_cat_ms"] = timed(torch_sort, stream, max(iters // 2, 3), 1)
        row["equal_to_torch_sort"] = bool(torch.equal(bits(torch_sort()[0].reshape(-1)), bits(kout)))
    eng.close()
    seng.close()
    torch.cuda.empty_cache()
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
    for name, dtype, descending, lengths, extras in SHAPES:
        if only and name not in only:
            continue
        row = run_shape(name, dtype, descending, lengths, extras, args.iters, args.warmup, rng, gen)
        row["device"] = rsx.device_name(0)
        print(json.dumps(row), flush=True)
        out.append(row)
        if args.out:                                            # rewritten after every shape: a cut-short run keeps what it measured
            with open(args.out, "w") as f:
                for r in out:
                    f.write(json.dumps(r) + "\n")
    for r in out:
        extra = f" | torch.sort(cat) {r['torch_sort_of_cat_ms']:.3f}" if "torch_sort_of_cat_ms" in r else ""
        print(f"{r['shape']:>32}  call {r['call_ms']:.3f} ms ({r['call_tb_per_s']:.2f} TB/s) | composition {r['composition_ms']:.3f} (spread "
              f"{r['composition_spread']:.1%}) x{r['speedup']:.1f} -> (b) {r['bar_b']} | copy {r['copy_ms']:.3f} (spread {r['copy_spread']:.1%}) x{r['time_ratio']:.2f} "
              f"measured, x{r['byte_ratio']:.2f} by bytes -> (a) {r['bar_a']} | equal {r['equal_to_composition']}{extra}", file=sys.stderr)


if __name__ == "__main__":
    main()
