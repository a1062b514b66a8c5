#!/usr/bin/env python3
"""rsx_segmented_search (lower bound) against the composition a user of this library has without it, one JSON line per shape.

Partner: the queries of every segment concatenated to its keys and the n + Q keys sorted with a payload (rsx_segmented_sort; rsx_sort_from
for one segment), from which the bounds could be read off.  Only that sort is timed — not the concatenation before it nor the pass after
it — which favours the partner.  Call and partner are measured alternately in one process, PAIR_REPEATS repeats of the pair, so that the
partner's spread is known.
Bar (b): call < partner x (1 - max(10 %, 2 x partner spread)).
Report only: torch.searchsorted on the flat and the ascending row shapes; on the flat shapes the same call on an engine created with
RSX_SEARCH_SAMPLED=0, i.e. the direct path where the default takes the sampled one.
Times are HIP events on one stream around each call, median of --iters after --warmup.

    python tools/search_bench.py [--iters 10] [--warmup 3] [--only NAME[,NAME...]] [--out profiles/search_bench.jsonl]
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
from unique_bench import PAIR_REPEATS, timed, zipf_lengths  # noqa: E402

rsx = load_package()

SHAPES = [      # name, dtype, descending, rows (None: one segment, "zipf": ragged), row length / n, queries per row / in all, sorted queries
    ("1x2^28_u32_2^24q", "uint32", False, None, 1 << 28, 1 << 24, False),
    ("1x2^28_u32_2^24q_sorted", "uint32", False, None, 1 << 28, 1 << 24, True),
    ("1x2^27_u64_2^24q", "uint64", False, None, 1 << 27, 1 << 24, False),
    ("1024x50257_f32_desc_1q", "float32", True, 1024, 50257, 1, False),
    ("4096x4096_f32_4096q", "float32", False, 4096, 4096, 4096, False),
    ("2^16x4096_u32_16q", "uint32", False, 1 << 16, 4096, 16, False),
    ("zipf_2^26_u32_2^22q", "uint32", False, "zipf", 1 << 26, 1 << 22, False),
]
TDT = {"uint32": torch.int32, "uint64": torch.int64, "float32": torch.float32}


def draw(dtype, count, gen):
    """non-negative integers (the same order as signed and as unsigned numbers), or uniform floats"""
    if dtype == "float32":
        return torch.rand(count, dtype=torch.float32, device="cuda", generator=gen)
    return torch.randint(0, torch.iinfo(TDT[dtype]).max, (count,), dtype=TDT[dtype], device="cuda", generator=gen)


def model_bytes(kb, nq):
    """DESIGN.md §4g, the part every path has: the queries read, the results written"""
    return nq * (kb + 4)


def run_shape(name, dtype, descending, rows, length, qcount, sorted_q, iters, warmup, rng, gen):
    stream = torch.cuda.current_stream()
    kb = torch.empty(0, dtype=TDT[dtype]).element_size()
    # ---- the haystack, sorted by segment (setup, not timed) ----
    if rows is None:
        n, nq, nseg = length, qcount, 1
        keys = torch.sort(draw(dtype, n, gen), descending=descending).values
        off = qoff = None
        lens = qlens = None
    elif rows == "zipf":
        n, nq = length, qcount
        lens = zipf_lengths(n, rng)
        nseg = len(lens)
        o = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        qo = o * nq // n                                        # queries in proportion to the keys
        qlens = np.diff(qo)
        off, qoff = torch.from_numpy(o).cuda(), torch.from_numpy(qo).cuda()
        keys, _ = rsx.segmented_sort(draw(dtype, n, gen), off, descending=descending)
    else:
        n, nq, nseg = rows * length, rows * qcount, rows
        keys = torch.sort(draw(dtype, n, gen).reshape(rows, length), dim=-1, descending=descending).values.reshape(-1)
        lens, qlens = np.full(rows, length, dtype=np.int64), np.full(rows, qcount, dtype=np.int64)
        off = torch.arange(rows + 1, dtype=torch.int64, device="cuda") * length
        qoff = None                                             # the even form
    queries = draw(dtype, nq, gen)
    if sorted_q:
        queries = torch.sort(queries).values
    out = torch.empty(nq, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def make_engine(sampled=True):
        if not sampled:
            os.environ["RSX_SEARCH_SAMPLED"] = "0"
        try:
            e = rsx.Engine(dtype, 4096, descending=descending)
        finally:
            os.environ.pop("RSX_SEARCH_SAMPLED", None)
        e.set_stream(stream.cuda_stream)
        return e

    def searcher(e):
        optr, qoptr = (None if off is None else off.data_ptr()), (None if qoff is None else qoff.data_ptr())
        return lambda: e.segmented_search(keys.data_ptr(), n, optr, nseg, queries.data_ptr(), nq, qoptr, out.data_ptr())

    eng = make_engine()
    search = searcher(eng)

    # ---- the partner: keys and queries of every segment in one array, sorted with a payload ----
    total = n + nq
    if rows is None:
        both = torch.cat([keys, queries])
        coff = None
    else:
        tl, tq = torch.from_numpy(lens).cuda(), torch.from_numpy(qlens).cuda()
        q_starts = (torch.arange(nseg + 1, dtype=torch.int64, device="cuda") * qcount) if qoff is None else qoff
        coff = (off + q_starts).contiguous()
        both = torch.empty(total, dtype=keys.dtype, device="cuda")
        both[torch.arange(n, device="cuda") + torch.repeat_interleave(q_starts[:-1], tl)] = keys
        both[torch.arange(nq, device="cuda") + torch.repeat_interleave(off[1:], tq)] = queries
        del tl, tq
    payload = torch.arange(total, dtype=torch.int32, device="cuda")
    peng = rsx.Engine(dtype, total, payload=True, descending=descending)
    peng.set_stream(stream.cuda_stream)
    if rows is None:
        partner = lambda: peng.sort_from(both.data_ptr(), total, payload.data_ptr())
    else:
        k_out, p_out = torch.empty_like(both), torch.empty_like(payload)
        partner = lambda: peng.segmented_sort(both.data_ptr(), total, coff.data_ptr(), nseg, k_out.data_ptr(), payload.data_ptr(), p_out.data_ptr())

    call_ms, par = [], []
    for _ in range(PAIR_REPEATS):                               # alternate the two, so that drift hits both
        par.append(timed(partner, stream, iters, warmup))
        call_ms.append(timed(search, stream, iters, warmup))
    eng.sync()
    peng.sync()
    peng.close()
    p_ms, s_ms = float(np.median(par)), float(np.median(call_ms))
    spread = (max(par) - min(par)) / p_ms
    margin = max(0.10, 2 * spread)
    bound = p_ms * (1 - margin)
    row = {"shape": name, "dtype": dtype, "descending": descending, "n": n, "segments": nseg, "queries": nq, "sorted_queries": sorted_q,
           "search_ms": s_ms, "search_repeats_ms": call_ms, "partner": "sort of the n + Q concatenated keys with payload", "partner_ms": p_ms,
           "partner_repeats_ms": par, "partner_spread": spread, "margin": margin, "bar_b_bound_ms": bound, "bar_b": "met" if s_ms < bound else "missed",
           "speedup": p_ms / s_ms, "queries_per_us": nq / s_ms / 1e3, "min_model_bytes": model_bytes(kb, nq)}
    # ---- report only ----
    if not descending and rows != "zipf":
        seq = keys if rows is None else keys.reshape(rows, length)
        vals = queries if rows is None else queries.reshape(rows, qcount)
        search()
        eng.sync()
        want = torch.searchsorted(seq, vals, out_int32=True)
        row["equal_torch"] = bool(torch.equal(want.reshape(-1), out))
        del want
        row["torch_searchsorted_ms"] = timed(lambda: torch.searchsorted(seq, vals, out_int32=True), stream, max(iters // 2, 3), 1)
    if rows is None:
        first = out.clone()
        deng = make_engine(sampled=False)
        direct = searcher(deng)
        row["direct_only_ms"] = float(np.median([timed(direct, stream, iters, warmup) for _ in range(3)]))
        deng.sync()
        row["direct_equal_sampled"] = bool(torch.equal(first, out))
        row["sampled_vs_direct"] = "sampled faster" if s_ms < row["direct_only_ms"] else "direct faster"
        deng.close()
    eng.close()
    del keys, queries, out, both, payload
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
    for name, dtype, descending, rows, length, qcount, sorted_q in SHAPES:
        if only and name not in only:
            continue
        for row in run_shape(name, dtype, descending, rows, length, qcount, sorted_q, args.iters, args.warmup, rng, gen):
            row["device"] = rsx.device_name(0)
            print(json.dumps(row), flush=True)
            out.append(row)
        if args.out:                                            # rewritten after every shape: a cut-short run keeps what it measured
            with open(args.out, "w") as f:
                for r in out:
                    f.write(json.dumps(r) + "\n")
    for r in out:
        extra = "".join(f" | {k.replace('_ms', '')} {r[k]:.3f}" for k in ("torch_searchsorted_ms", "direct_only_ms") if k in r)
        print(f"{r['shape']:>26}  search {r['search_ms']:.3f} ms | partner {r['partner_ms']:.3f} (spread {r['partner_spread']:.1%}) | "
              f"bound {r['bar_b_bound_ms']:.3f} -> (b) {r['bar_b']}, x{r['speedup']:.1f}{extra}", file=sys.stderr)


if __name__ == "__main__":
    main()
