#!/usr/bin/env python3
"""rsx_segmented_join against the composition a user has without it and against a device-to-device copy, one JSON line per shape.

Partners, each timed whole and alternated with the call in one process, PAIR_REPEATS repeats, so that every partner's spread is known:
  compose  Composition below, built on the calls the library had before the join: Engine.segmented_search twice (lower and upper bound of
           A's keys in B), a torch subtraction, rsx.cumsum (int64), Engine.segmented_expand with segment and rank over the row offsets,
           a second expand for the A positions inside their segments (ragged shapes), and torch gathers for the indices; all into
           preallocated buffers (tests/test_gpu_join.py checks this same class against the call entry for entry)
  copy     rsx_copy_on_device of na * kb bytes (2 * na * kb bytes of traffic)
Bar (b), the requirement: the call is faster than the composition by more than max(10 %, 2 x the composition's spread).
Bar (a), reported: call <= copy x byte ratio x (1 + max(10 %, 2 x copy spread)); byte ratio = DESIGN.md §4n's bytes / (2 na kb): A read
once, one 32-byte sector per probe of B, 12 bytes of scratch per A position written and read (16 with offsets), 8 or 8 + kb bytes per row.
torch.isin is reported beside the SEMI rows without a bar.  INNER shapes are compared with the composition entry for entry before they
are timed; LEFT and SEMI with torch expressions of their definition.  Times are HIP events on one stream around each call, median of
--iters after --warmup; outputs are preallocated.  Shapes and partners are not tuned to move a verdict: a missed bar is printed as missed.

    python tools/join_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/join_bench.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
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


class Composition:
    """The inner join without rsx_segmented_join.  a, b: sorted 1-D device tensors; a_off, b_off: int64 device offsets starting at 0 and
    ending at a.numel() / b.numel(), or both None.  rows: the number of rows (the buffers are preallocated, as the call's are).  run()
    fills ia, ib (int32, relative to the segments) and out_offsets."""

    def __init__(self, a, a_off, b, b_off, descending, rows, stream):
        name = str(a.dtype).replace("torch.", "")
        self.eng = rsx.Engine(name, 4096, descending=descending)
        self.eng.set_stream(stream)
        self.a, self.b, self.a_off, self.b_off, self.rows = a, b, a_off, b_off, rows
        na = a.numel()
        self.nseg = 1 if a_off is None else a_off.numel() - 1
        dev = a.device
        self.lo = torch.empty(na, dtype=torch.int32, device=dev)
        self.hi = torch.empty(na, dtype=torch.int32, device=dev)
        self.cnt = torch.empty(na, dtype=torch.int64, device=dev)
        self.off = torch.zeros(na + 1, dtype=torch.int64, device=dev)
        self.owner = torch.empty(rows, dtype=torch.int32, device=dev)
        self.rank = torch.empty(rows, dtype=torch.int32, device=dev)
        self.arel = torch.empty(na, dtype=torch.int32, device=dev) if a_off is not None else None
        self.ia = torch.empty(rows, dtype=torch.int32, device=dev) if a_off is not None else self.owner
        self.ib = torch.empty(rows, dtype=torch.int32, device=dev)
        self.out_offsets = torch.zeros(self.nseg + 1, dtype=torch.int64, device=dev)

    def run(self):
        e, na, nb = self.eng, self.a.numel(), self.b.numel()
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        if na == 0:
            return
        for right, out in ((False, self.lo), (True, self.hi)):
            e.segmented_search(ptr(self.b), nb, ptr(self.b_off), self.nseg, self.a.data_ptr(), na, ptr(self.a_off), out.data_ptr(), right=right)
        torch.sub(self.hi, self.lo, out=self.cnt)
        self.off[1:].copy_(rsx.cumsum(self.cnt))
        if self.rows:
            e.segmented_expand(None, 0, 4, self.off.data_ptr(), na, self.rows, None, None, self.owner.data_ptr(), self.rank.data_ptr())
            if self.a_off is not None:
                e.segmented_expand(None, 0, 4, self.a_off.data_ptr(), self.nseg, na, None, None, None, self.arel.data_ptr())
                torch.index_select(self.arel, 0, self.owner, out=self.ia)
            torch.index_select(self.lo, 0, self.owner, out=self.ib)
            self.ib.add_(self.rank)
        if self.a_off is not None:
            torch.index_select(self.off, 0, self.a_off, out=self.out_offsets)
        else:
            self.out_offsets[1:].copy_(self.off[-1:])

    def close(self):
        self.eng.sync()
        self.eng.close()


def sorted_draw(n, values, dtype, gen):
    return torch.sort(torch.randint(0, values, (n,), dtype=dtype, device="cuda", generator=gen)).values


def distinct(n, dtype, step=1):
    return torch.arange(0, n * step, step, dtype=dtype, device="cuda")


def foreign_key(gen):
    return sorted_draw(1 << 26, 1 << 20, torch.int32, gen), None, distinct(1 << 20, torch.int32), None


def many_to_many(gen):
    return sorted_draw(1 << 22, 1 << 18, torch.int32, gen), None, sorted_draw(1 << 22, 1 << 18, torch.int32, gen), None


def hot_key(gen):
    side = torch.sort(torch.cat([distinct(1 << 20, torch.int32, 2), torch.full((1 << 13,), 777, dtype=torch.int32, device="cuda")])).values
    return side, None, side.clone(), None


def sparse_walk(gen):
    n = 1 << 27
    a, b = distinct(n, torch.int32, 2), distinct(n, torch.int32, 2) + 1
    common = torch.arange(0, n, n >> 10, device="cuda")
    b[common] -= 1
    return a, None, b, None


def wide(gen):
    n = 1 << 26
    a, b = distinct(n, torch.int64, 2), distinct(n, torch.int64, 2)
    b[1::2] += 1
    return a, None, b, None


def rows_of(S, la, lb, dtype, values, gen, descending=False):
    def side(L):
        x = torch.randint(0, values, (S, L), device="cuda", generator=gen).to(dtype)
        return torch.sort(x, dim=1, descending=descending).values.reshape(-1).contiguous()
    steps = torch.arange(0, S + 1, dtype=torch.int64, device="cuda")
    return side(la), steps * la, side(lb), steps * lb


def ragged(gen):
    rng = np.random.default_rng(2026)
    la, lb = zipf_lengths(1 << 26, rng), zipf_lengths(1 << 26, rng)
    S = max(len(la), len(lb))
    la, lb = np.concatenate([la, np.zeros(S - len(la), dtype=np.int64)]), np.concatenate([lb, np.zeros(S - len(lb), dtype=np.int64)])
    out = []
    for lens in (la, lb):
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        seg = rsx.segment_ids(off, n=int(off[-1]))
        span = torch.from_numpy(np.maximum(la, lb) + 3).cuda()[seg]
        keys = (torch.rand(seg.numel(), device="cuda", generator=gen) * span).to(torch.int32)
        order = torch.argsort(seg * (1 << 31) + keys)               # by segment, then key
        out += [keys[order].contiguous(), off]
    return tuple(out)


SHAPES = [      # name, kind, keys out, descending, generator
    ("fk_2^26_over_2^20", "inner", False, False, foreign_key),
    ("m2m_2^22x2^22_over_2^18", "inner", False, False, many_to_many),
    ("hot_key_2^20+2^13", "inner", False, False, hot_key),
    ("sparse_2^27_2^10_common", "inner", False, False, sparse_walk),
    ("u64_2^26_half_common", "inner", False, False, wide),
    ("2^16x(512+512)", "inner", False, False, lambda gen: rows_of(1 << 16, 512, 512, torch.int32, 1024, gen)),
    ("2^20x(50+50)_f32_desc", "inner", False, True, lambda gen: rows_of(1 << 20, 50, 50, torch.float32, 100, gen, True)),
    ("zipf_2^26", "inner", False, False, ragged),
    ("fk_left_keys", "left", True, False, foreign_key),
    ("semi_2^27_in_2^20", "semi", False, False, lambda gen: (sorted_draw(1 << 27, 1 << 21, torch.int32, gen), None, distinct(1 << 20, torch.int32, 2), None)),
]


def model_bytes(kb, na, rows, probes, ragged_a, keys_out):
    """A once, a sector per probe, the scratch written and read, the rows"""
    return na * kb + 32 * probes + 2 * (16 if ragged_a else 12) * na + rows * (8 + (kb if keys_out else 0))


def run_shape(name, how, keys_out, descending, make, gen, iters, warmup):
    stream = torch.cuda.current_stream()
    a, a_off, b, b_off = make(gen)
    na, nb, kb = a.numel(), b.numel(), a.element_size()
    nseg = 1 if a_off is None else a_off.numel() - 1
    code = {"inner": rsx.JOIN_INNER, "left": rsx.JOIN_LEFT, "semi": rsx.JOIN_SEMI}[how]
    eng = rsx.Engine(str(a.dtype).replace("torch.", ""), 4096, descending=descending)
    eng.set_stream(stream.cuda_stream)
    ooff = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    eng.segmented_join(a.data_ptr(), na, ptr(a_off), b.data_ptr(), nb, ptr(b_off), nseg, code, 0, ooff.data_ptr())
    rows = int(ooff[-1].item())
    eng.sync()
    ia = torch.empty(rows, dtype=torch.int32, device="cuda")
    ib = torch.empty(rows, dtype=torch.int32, device="cuda")
    ko = torch.empty(rows, dtype=a.dtype, device="cuda") if keys_out else None

    def call():
        eng.segmented_join(a.data_ptr(), na, ptr(a_off), b.data_ptr(), nb, ptr(b_off), nseg, code, rows, ooff.data_ptr(), d_a_index_out=ia.data_ptr(),
                           d_b_index_out=ib.data_ptr(), d_keys_out=ptr(ko))

    call()
    eng.sync()
    partners, row = {}, {}
    comp = None
    if how == "inner":
        comp = Composition(a, a_off, b, b_off, descending, rows, stream.cuda_stream)
        comp.run()
        comp.eng.sync()
        row["compose_equal"] = bool(torch.equal(ia, comp.ia) and torch.equal(ib, comp.ib) and torch.equal(ooff, comp.out_offsets))
        partners["compose"] = comp.run
    elif how == "left":
        hit = ib != -1
        row["definition_equal"] = bool(rows >= na and torch.equal(ko, a[ia.long()]) and torch.equal(b[ib[hit].long()], ko[hit]))
    else:
        row["definition_equal"] = bool(torch.equal(ia.long(), torch.nonzero(torch.isin(a, b)).reshape(-1)))
        row["torch_isin_ms"] = timed(lambda: torch.isin(a, b, assume_unique=False), stream, max(iters // 2, 3), 1)
    scratch = torch.empty_like(a)

    def copy():
        assert eng.lib.rsx_copy_on_device(eng._h, C.c_void_p(scratch.data_ptr()), C.c_void_p(a.data_ptr()), na * kb) == 0

    partners["copy"] = copy
    times = {k: [] for k in ("call", *partners)}
    for _ in range(PAIR_REPEATS):
        for pname, fn in partners.items():
            times[pname].append(timed(fn, stream, iters, warmup))
        times["call"].append(timed(call, stream, iters, warmup))
    eng.sync()
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    row.update(shape=name, kind=how, keys_out=keys_out, na=na, nb=nb, segments=nseg, rows=rows, key_bytes=kb, call_ms=med["call"], call_repeats_ms=times["call"],
               call_spread=spread["call"])
    for p in partners:
        row[p + "_ms"], row[p + "_repeats_ms"], row[p + "_spread"] = med[p], times[p], spread[p]
    if comp is not None:
        margin = max(0.10, 2 * spread["compose"])
        row["compose_margin"] = margin
        row["bar_b"] = "met" if med["call"] < med["compose"] / (1 + margin) else "missed"
        comp.close()
    probes = na * (math.ceil(math.log2(max(nb / nseg, 2))) + 2)     # the bisection's levels and the gallop's two probes of a lone partner
    cb, pb = model_bytes(kb, na, rows, probes, a_off is not None, keys_out), 2 * na * kb
    margin = max(0.10, 2 * spread["copy"])
    row.update(byte_ratio=cb / pb, time_ratio=med["call"] / med["copy"], bar_a_bound_ms=med["copy"] * cb / pb * (1 + margin))
    row["bar_a"] = "met" if med["call"] <= row["bar_a_bound_ms"] else "missed"
    eng.close()
    return row


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
    for name, how, keys_out, descending, make in SHAPES:
        if only and name not in only:
            continue
        row = run_shape(name, how, keys_out, descending, make, gen, args.iters, args.warmup)
        row["device"] = rsx.device_name(0)
        print(json.dumps(row), flush=True)
        out.append(row)
        torch.cuda.empty_cache()
        if args.out:                                                # rewritten after every row: a cut-short run keeps what it measured
            with open(args.out, "w") as f:
                for r in out:
                    f.write(json.dumps(r) + "\n")
    for r in out:
        b = f" | compose {r['compose_ms']:.3f} (b) {r['bar_b']} equal {r['compose_equal']}" if "compose_ms" in r else f" | equal {r['definition_equal']}"
        print(f"{r['shape']:>26} {r['kind']:>5}  call {r['call_ms']:.3f} ms | copy {r['copy_ms']:.3f} x{r['time_ratio']:.2f} measured, x{r['byte_ratio']:.2f} by bytes "
              f"(a) {r['bar_a']}{b}" + (f" | torch.isin {r['torch_isin_ms']:.3f}" if "torch_isin_ms" in r else ""), file=sys.stderr)


if __name__ == "__main__":
    main()
