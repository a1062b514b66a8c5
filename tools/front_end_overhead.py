#!/usr/bin/env python3
"""Host cost of a tiny call through the torch wrappers: what a caller with small tensors pays is the wrappers' Python, not the kernels.

For segmented_scan, segmented_searchsorted, segmented_merge and segmented_join(capacity=int) on 64 elements in 4 segments: the wall time
per call of --calls back-to-back calls with ONE stream synchronisation at the end, after a warm-up; --reps repetitions, and per wrapper
the median, the smallest and the largest of them in microseconds, as one JSON line.  None of the four synchronises with the host itself.

--package DIR measures another copy of the Python package (an older __init__.py next to planner.py and distributed.py) over the same
library: run the two alternately and compare the new median with the spread the old one shows against itself.  One process, no network;
--time-limit (seconds) ends it.

    python tools/front_end_overhead.py --calls 3000 --reps 9
    python tools/front_end_overhead.py --package /tmp/parent_package --label parent
"""
import argparse
import importlib.util
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(package_dir):
    spec = importlib.util.spec_from_file_location("radix_sort_amd", os.path.join(package_dir, "__init__.py"),
                                                  submodule_search_locations=[package_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["radix_sort_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=os.path.join(ROOT, "radix-sort_amd"))
    ap.add_argument("--label", default="")
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--time-limit", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    os.environ.setdefault("RSX_LIB", os.path.join(ROOT, "radix-sort_amd", "libradixsort_hip.so"))
    import torch
    rsx = load(args.package)
    dev = torch.device("cuda", 0)
    off = torch.arange(0, 5, dtype=torch.int64, device=dev) * 16                  # 4 segments of 16
    values = torch.arange(64, dtype=torch.float32, device=dev)
    a = (torch.arange(64, dtype=torch.int32, device=dev) % 16) * 2                 # every segment sorted: 0, 2, .. 30
    b = a + 1 - (torch.arange(64, dtype=torch.int32, device=dev) % 2)              # sorted too, half of it meets a
    cases = {
        "segmented_scan": lambda: rsx.segmented_scan(values, off),
        "segmented_searchsorted": lambda: rsx.segmented_searchsorted(a, off, b),
        "segmented_merge": lambda: rsx.segmented_merge(a, off, b, off),
        "segmented_join": lambda: rsx.segmented_join(a, off, b, off, capacity=256),
    }
    stream = torch.cuda.current_stream(dev)
    result = {"label": args.label, "package": os.path.abspath(args.package), "calls": args.calls, "reps": args.reps, "us_per_call": {}}
    for name, call in cases.items():
        for _ in range(args.warmup):
            call()
        stream.synchronize()
        per_call = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            stream.synchronize()
            per_call.append((time.perf_counter() - t0) / args.calls * 1e6)
        result["us_per_call"][name] = {"median": round(statistics.median(per_call), 2), "min": round(min(per_call), 2), "max": round(max(per_call), 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
