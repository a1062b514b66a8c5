#!/usr/bin/env python3
"""rsx_segmented_set_op against the composition it replaces and against rsx_segmented_merge of the same inputs, one JSON line per shape
and op (intersection, union).

Bar (b), a requirement: call < composition / (1 + max(10 %, 2 x the composition's spread)).  The composition is what a user of this
library has without the call.  Intersection: rsx_segmented_search of A's keys in B, lower and upper, and of A's keys in A, lower; the
torch arithmetic that makes the mask (rank among equals < count in B); rsx_segmented_compact in mask form.  Union: the same on B's side
(rank >= count in A), then rsx_segmented_merge of A with the compacted B.  All of it is timed, into preallocated buffers (the position of
every element relative to its segment, which depends on the offsets alone, is formed outside).  Call and partners are measured
alternately in one process, PAIR_REPEATS repeats, so that the partners' spreads are known.  The results must be equal entry for entry:
keys by bits and the kept offsets (with --extras rows also payload, index and match).
Bar (a), reported as met or missed without being a requirement: call <= merge x byte ratio x (1 + max(10 %, 2 x the merge's spread)),
the merge being rsx_segmented_merge of the same inputs, keys only; the byte ratio is DESIGN.md §4j's for keys only:
(2 (na + nb) + kept) / (2 (na + nb)).
Beside the bars, without one, on one-segment shapes: a[torch.isin(a, b)] for the intersection and torch.unique(torch.cat([a, b])) for
the union (set semantics: equal to the call on duplicate-free inputs only; the times are what is reported).
Times are HIP events on one stream around each call, median of --iters after --warmup.  Keys are non-negative, so that torch's signed
order is the unsigned engine's.

    python tools/setop_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/setop_bench.jsonl]
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
from merge_bench import TORCH_DT, random_keys, zipf_pair  # noqa: E402
from unique_bench import PAIR_REPEATS, timed  # noqa: E402

rsx = load_package()

SHAPES = [      # name, engine dtype, descending, (la, lb) per segment as a function of rng (None, (na, nb): NULL offsets), payload + index + match
    ("1x(2^27+2^27)_u32", "uint32", False, (None, (1 << 27, 1 << 27)), False),
    ("1x(2^28-2^20,2^20)_u32", "uint32", False, (None, ((1 << 28) - (1 << 20), 1 << 20)), False),
    ("1x(2^26+2^26)_u64", "uint64", False, (None, (1 << 26, 1 << 26)), False),
    ("4096x(2^15+2^15)_u32", "uint32", False, (lambda rng: (np.full(4096, 1 << 15), np.full(4096, 1 << 15)), None), False),
    ("2^20x(50+50)_f32_desc", "float32", True, (lambda rng: (np.full(1 << 20, 50), np.full(1 << 20, 50)), None), False),
    ("zipf_2^26_u32", "uint32", False, (lambda rng: zipf_pair(1 << 26, rng), None), False),
    ("1x(2^27+2^27)_u32_payload_index_match", "uint32", False, (None, (1 << 27, 1 << 27)), True),
]
OPS = [("intersection", rsx.SET_INTERSECTION), ("union", rsx.SET_UNION)]


def sort_side(keys, lens, descending):
    if lens is None:
        return torch.sort(keys, descending=descending)[0]
    if len(set(lens.tolist())) == 1 and lens[0] > 0:
        return torch.sort(keys.reshape(len(lens), int(lens[0])), dim=-1, descending=descending)[0].reshape(-1).contiguous()
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
    return rsx.segmented_sort(keys, offs, descending=descending)[0]         # (int32 / int64 engines: the unsigned order on non-negative keys)


def make_inputs(na, nb, la, lb, tdt, descending, gen):
    """two sorted sides; about half of B's keys are A's: every other key of A's segment where the segments have equal lengths (or there is
    one), keys of a range of 2^20 values where they are ragged"""
    if la is not None and not (len(set(la.tolist())) == 1 and len(set(lb.tolist())) == 1):
        a = torch.randint(0, 1 << 20, (na,), dtype=tdt, device="cuda", generator=gen)
        b = torch.randint(0, 1 << 20, (nb,), dtype=tdt, device="cuda", generator=gen)
        return sort_side(a, la, descending), sort_side(b, lb, descending)
    rows = 1 if la is None else len(la)
    a = sort_side(random_keys(na, tdt, gen), la, descending)
    wa, wb = na // rows, nb // rows
    stride = max(wa // max(wb // 2, 1), 2)                      # A's keys at an even stride: the shared keys span A's whole range
    take = min(wb // 2, (wa + stride - 1) // stride)
    shared = a.reshape(rows, wa)[:, ::stride][:, :take]
    b = torch.cat([shared, random_keys(rows * (wb - take), tdt, gen).reshape(rows, wb - take)], dim=1).reshape(-1).contiguous()
    return a, sort_side(b, lb, descending)


def run_shape(name, dtype, descending, lengths, extras, opname, op, iters, warmup, rng, gen):
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
    a, b = make_inputs(na, nb, la, lb, tdt, descending, gen)
    aoff = boff = None
    rel_a, rel_b = torch.arange(na, dtype=torch.int32, device="cuda"), torch.arange(nb, dtype=torch.int32, device="cuda")
    if la is not None:
        aoff = torch.from_numpy(np.concatenate([[0], np.cumsum(la)]).astype(np.int64)).cuda()
        boff = torch.from_numpy(np.concatenate([[0], np.cumsum(lb)]).astype(np.int64)).cuda()
        rel_a -= torch.repeat_interleave(aoff[:-1], torch.from_numpy(la).cuda()).to(torch.int32)
        rel_b -= torch.repeat_interleave(boff[:-1], torch.from_numpy(lb).cuda()).to(torch.int32)
    ptr = lambda t: None if t is None else t.data_ptr()
    i32 = lambda count: torch.empty(count, dtype=torch.int32, device="cuda")
    cap = na if op == rsx.SET_INTERSECTION else n
    pa = pb = pout = iout = mout = None
    if extras:
        pa, pb = torch.arange(na, dtype=torch.int32, device="cuda"), torch.arange(nb, dtype=torch.int32, device="cuda") + na
        pout, iout = i32(cap), i32(cap)
        mout = i32(cap) if op == rsx.SET_INTERSECTION else None
    kout = torch.empty(cap, dtype=tdt, device="cuda")
    koff = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
    eng = rsx.Engine(dtype, 4096, descending=descending)
    eng.set_stream(stream.cuda_stream)

    def call():
        eng.segmented_set_op(a.data_ptr(), na, ptr(aoff), b.data_ptr(), nb, ptr(boff), nseg, op, kout.data_ptr(), koff.data_ptr(), ptr(iout), ptr(mout),
                             d_a_payload=ptr(pa), d_b_payload=ptr(pb), d_payload_out=ptr(pout))

    # the composition, into preallocated buffers
    x, xoff, nx, relx, y, yoff, ny = (a, aoff, na, rel_a, b, boff, nb) if op == rsx.SET_INTERSECTION else (b, boff, nb, rel_b, a, aoff, na)
    lo_y, hi_y, lo_x, rank = i32(nx), i32(nx), i32(nx), i32(nx)
    mask = torch.empty(nx, dtype=torch.bool, device="cuda")
    ckeys = torch.empty(nx, dtype=tdt, device="cuda")
    cidx = torch.zeros(nx, dtype=torch.int32, device="cuda") if extras else None        # (zeros: what the compaction does not write is gathered from too)
    ckoff = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
    ukeys = torch.empty(n, dtype=tdt, device="cuda") if op == rsx.SET_UNION else None
    uoff = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
    upay, uidx = (i32(n), i32(n)) if extras and op == rsx.SET_UNION else (None, None)
    cpay, cmatch = (i32(nx), i32(nx)) if extras else (None, None)

    def composition():
        eng.segmented_search(y.data_ptr(), ny, ptr(yoff), nseg, x.data_ptr(), nx, ptr(xoff), lo_y.data_ptr())
        eng.segmented_search(y.data_ptr(), ny, ptr(yoff), nseg, x.data_ptr(), nx, ptr(xoff), hi_y.data_ptr(), right=True)
        eng.segmented_search(x.data_ptr(), nx, ptr(xoff), nseg, x.data_ptr(), nx, ptr(xoff), lo_x.data_ptr())
        torch.sub(relx, lo_x, out=rank)                         # the rank among equals on the element's own side
        torch.sub(hi_y, lo_y, out=hi_y)                         # the count on the other side
        if op == rsx.SET_INTERSECTION:
            torch.lt(rank, hi_y, out=mask)
        else:
            torch.ge(rank, hi_y, out=mask)
        eng.segmented_compact(x.data_ptr(), nx, ptr(xoff), nseg, mask.data_ptr(), None, ckeys.data_ptr(), ptr(cidx), ckoff.data_ptr())
        if extras and op == rsx.SET_INTERSECTION:               # (one segment: the compaction's index is a position in A)
            torch.index_select(pa, 0, cidx, out=cpay)
            torch.add(lo_y, rank, out=lo_y)
            torch.index_select(lo_y, 0, cidx, out=cmatch)
        if op == rsx.SET_UNION:
            eng.segmented_merge(a.data_ptr(), na, ptr(aoff), ckeys.data_ptr(), nb, ckoff.data_ptr() if aoff is not None else None, nseg, ukeys.data_ptr(),
                                None, uoff.data_ptr())

    union_one_segment = op == rsx.SET_UNION and aoff is None
    if union_one_segment:
        # one segment has no offsets array: the merge needs the compacted length as nb, a host value; the composition reads it back once
        def composition_union():
            eng.segmented_search(y.data_ptr(), ny, None, 1, x.data_ptr(), nx, None, lo_y.data_ptr())
            eng.segmented_search(y.data_ptr(), ny, None, 1, x.data_ptr(), nx, None, hi_y.data_ptr(), right=True)
            eng.segmented_search(x.data_ptr(), nx, None, 1, x.data_ptr(), nx, None, lo_x.data_ptr())
            torch.sub(relx, lo_x, out=rank)
            torch.sub(hi_y, lo_y, out=hi_y)
            torch.ge(rank, hi_y, out=mask)
            eng.segmented_compact(x.data_ptr(), nx, None, 1, mask.data_ptr(), None, ckeys.data_ptr(), None, ckoff.data_ptr())
            kept_b = int(ckoff[-1].item())
            eng.segmented_merge(a.data_ptr(), na, None, ckeys.data_ptr() if kept_b else None, kept_b, None, 1, ukeys.data_ptr(), None, uoff.data_ptr())
        comp = composition_union
    else:
        comp = composition

    mkeys = torch.empty(n, dtype=tdt, device="cuda")

    def merge():
        eng.segmented_merge(a.data_ptr(), na, ptr(aoff), b.data_ptr(), nb, ptr(boff), nseg, mkeys.data_ptr())

    call_ms, comp_ms, merge_ms = [], [], []
    for _ in range(PAIR_REPEATS):                               # alternate, so that drift hits all
        comp_ms.append(timed(comp, stream, iters, warmup))
        merge_ms.append(timed(merge, stream, iters, warmup))
        call_ms.append(timed(call, stream, iters, warmup))
    # equality, entry for entry
    call()
    comp()
    eng.sync()
    bits = lambda t: t.view(torch.int32 if kb == 4 else torch.int64)
    kept = int(koff[-1].item())
    if op == rsx.SET_INTERSECTION:
        equal = bool(torch.equal(koff, ckoff)) and bool(torch.equal(bits(kout[:kept]), bits(ckeys[:kept])))
        if extras:
            equal = equal and bool(torch.equal(iout[:kept], cidx[:kept])) and bool(torch.equal(pout[:kept], cpay[:kept])) and bool(torch.equal(mout[:kept], cmatch[:kept]))
    else:
        equal = bool(torch.equal(koff, uoff)) and bool(torch.equal(bits(kout[:kept]), bits(ukeys[:kept])))
    c_ms, s_ms, m_ms = float(np.median(call_ms)), float(np.median(comp_ms)), float(np.median(merge_ms))
    s_spread, m_spread = (max(comp_ms) - min(comp_ms)) / s_ms, (max(merge_ms) - min(merge_ms)) / m_ms
    b_margin, a_margin = max(0.10, 2 * s_spread), max(0.10, 2 * m_spread)
    ratio = (2 * n + kept) / (2 * n)
    limit = m_ms * ratio * (1 + a_margin)
    row = {"shape": name, "op": opname, "keys": dtype, "descending": descending, "segments": nseg, "na": na, "nb": nb, "kept": kept,
           "payload_index_match": extras, "call_ms": c_ms, "call_repeats_ms": call_ms,
           "composition": ("3 x rsx_segmented_search + torch mask + rsx_segmented_compact" + (" + rsx_segmented_merge" if op == rsx.SET_UNION else "")
                           + (" (one read-back of the compacted length)" if union_one_segment else "")),
           "composition_ms": s_ms, "composition_repeats_ms": comp_ms, "composition_spread": s_spread, "bar_b_margin": b_margin,
           "speedup": s_ms / c_ms, "bar_b": "met" if c_ms * (1 + b_margin) < s_ms else "missed", "equal_to_composition": equal,
           "merge_keys_only_ms": m_ms, "merge_repeats_ms": merge_ms, "merge_spread": m_spread, "byte_ratio_keys_only": ratio, "time_ratio": c_ms / m_ms,
           "bar_a_margin": a_margin, "bar_a_bound_ms": limit, "bar_a": ("met" if c_ms <= limit else "missed") if not extras else "not applicable (keys only)"}
    if aoff is None and not extras:
        if op == rsx.SET_INTERSECTION:
            partner = lambda: a[torch.isin(a, b)]
            row["torch_partner"] = "a[torch.isin(a, b)]"
        else:
            partner = lambda: torch.unique(torch.cat([a, b]))
            row["torch_partner"] = "torch.unique(torch.cat([a, b]))"
        try:
            row["torch_partner_ms"] = timed(partner, stream, 3, 1)
        except RuntimeError as e:                               # (out of memory at the largest shapes is a result too)
            row["torch_partner_ms"] = None
            row["torch_partner_error"] = str(e).splitlines()[0][:120]
    eng.close()
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
        for opname, op in OPS:
            if extras and op != rsx.SET_INTERSECTION:
                continue
            row = run_shape(name, dtype, descending, lengths, extras, opname, op, args.iters, args.warmup, rng, gen)
            row["device"] = rsx.device_name(0)
            print(json.dumps(row), flush=True)
            out.append(row)
            if args.out:                                        # rewritten after every row: a cut-short run keeps what it measured
                with open(args.out, "w") as f:
                    for r in out:
                        f.write(json.dumps(r) + "\n")
    for r in out:
        extra = f" | {r['torch_partner']} {r['torch_partner_ms']:.3f}" if r.get("torch_partner_ms") else ""
        print(f"{r['shape']:>38} {r['op']:>12}  call {r['call_ms']:.3f} ms | composition {r['composition_ms']:.3f} (spread {r['composition_spread']:.1%}) "
              f"x{r['speedup']:.1f} -> (b) {r['bar_b']} | merge {r['merge_keys_only_ms']:.3f} (spread {r['merge_spread']:.1%}) x{r['time_ratio']:.2f} measured, "
              f"x{r['byte_ratio_keys_only']:.2f} by bytes -> (a) {r['bar_a']} | equal {r['equal_to_composition']}{extra}", file=sys.stderr)


if __name__ == "__main__":
    main()
