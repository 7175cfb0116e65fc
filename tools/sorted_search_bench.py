#!/usr/bin/env python3
"""Ladder of sorted search (glu_sorted_search_run_ptr): haystacks of 2^20, 2^24 and 2^28 uint32 keys and of 2^28 uint64 keys,
2^10 .. 2^28 needles (every second power of two; --every 1 for all of them), the needles uniform random and the same needles
sorted, lower bound only.

    python tools/sorted_search_bench.py [--reps 20] [--quick] [--only TEXT] [--every 2] > profiles/sorted_search/ladder.txt

Every row: a haystack made and sorted on the device once (values below 2^31, so that torch's signed order is the library's),
device events on the call's stream around the call, 3 warm-up repetitions, median of --reps.  Columns, all in ms:
  direct    PATH forced DIRECT: the binary search of the haystack, one kernel
  indexed   PATH forced INDEXED without reuse: the index kernel and the search kernel
  reuse     glu_sorted_search_index_ptr once, outside the timing; the call with reuse_index: the search kernel alone
  auto      PATH AUTO, and the path it took (D or I)
  torch     torch.searchsorted(hay, needles, out_int32=True) on the int32 / int64 view of the same arrays: what a PyTorch user has
            today; and torch / auto
  ns/needle auto over the needle count
The lower bounds of the auto call are compared with torch's for every row.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

HAYSTACKS = ((20, "uint32"), (24, "uint32"), (28, "uint32"), (28, "uint64"))


def rows(quick, every):
    out = []
    for lg, key_type in (((20, "uint32"), (22, "uint64")) if quick else HAYSTACKS):
        for lg_needles in range(10, (20 if quick else 28) + 1, every):
            for order in ("random", "sorted"):
                out.append({"name": "2^%d %s, 2^%d %s" % (lg, key_type, lg_needles, order), "hay": 1 << lg, "key_type": key_type,
                            "needles": 1 << lg_needles, "order": order})
    return out


def median_ms(torch, reps, call):
    times = []
    for rep in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        if rep >= 3:
            times.append(a.elapsed_time(b))
    return float(np.median(times))


def measure(torch, G, stream, row, reps, cache):
    n, m, key_type = row["hay"], row["needles"], row["key_type"]
    dtype = torch.int32 if key_type == "uint32" else torch.int64
    if cache.get("hay_key") != (n, key_type):  # (the rows of a haystack share it)
        cache.clear()
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n % 1000 + len(key_type))
        hay = torch.randint(0, 2 ** 31 - 1, (n,), generator=gen, device="cuda", dtype=dtype).sort().values
        cache.update(hay_key=(n, key_type), hay=hay, gen=gen)
    if cache.get("needle_key") != m:  # (the random and the sorted row of a count share the draws)
        cache["needles"] = None
        cache.update(needle_key=m, needles=torch.randint(0, 2 ** 31 - 1, (m,), generator=cache["gen"], device="cuda", dtype=dtype))
    hay = cache["hay"]
    needles = cache["needles"] if row["order"] == "random" else cache["needles"].sort().values
    out = torch.empty(m, dtype=torch.int32, device="cuda")
    ss = G.SortedSearch()
    ss.prepare(n, key_type)

    def call(reuse=False):
        ss.run_ptr(hay.data_ptr(), n, needles.data_ptr(), m, out.data_ptr(), None, key_type, reuse, stream)

    res = {}
    for name, path in (("direct", G.SearchPath_Direct), ("indexed", G.SearchPath_Indexed), ("auto", G.SearchPath_Auto)):
        ss.set_option("PATH", path)
        res[name] = median_ms(torch, reps, call)
        if name == "auto":
            res["auto_path"] = "I" if ss.last()[0] == G.SearchPath_Indexed else "D"
    auto_out = out.clone()
    ss.index_ptr(hay.data_ptr(), n, key_type, stream)
    res["reuse"] = median_ms(torch, reps, lambda: call(True))
    res["torch"] = median_ms(torch, reps, lambda: torch.searchsorted(hay, needles, out_int32=True))
    want = torch.searchsorted(hay, needles, out_int32=True)
    assert torch.equal(auto_out, want) and torch.equal(out, want), "sorted search differs from torch.searchsorted"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="small haystacks and up to 2^20 needles only")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only (e.g. '2^28 uint32' under a profiler)")
    ap.add_argument("--every", type=int, default=2, help="step of the needle count's exponent")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    table = [row for row in rows(args.quick, args.every) if args.only is None or args.only in row["name"]]
    print("# %s" % G.device_info())
    print("# device events, 3 warm-up + %d repetitions, median; lower bound only; ms" % args.reps)
    print("%-30s %10s %10s %10s %10s %2s | %10s %9s | %9s" % ("row", "direct", "indexed", "reuse", "auto", "", "torch", "torch/auto", "ns/needle"))
    # a stream of our own, made current: the events go where the calls go (the handle of torch's default stream is 0, which the
    # library reads as "the library queue")
    side = torch.cuda.Stream()
    cache = {}
    with torch.cuda.stream(side):
        for row in table:
            r = measure(torch, G, side.cuda_stream, row, args.reps, cache)
            print("%-30s %10.4f %10.4f %10.4f %10.4f %2s | %10.4f %9.2f | %9.3f" % (
                row["name"], r["direct"], r["indexed"], r["reuse"], r["auto"], r["auto_path"], r["torch"], r["torch"] / r["auto"],
                1e6 * r["auto"] / row["needles"]))
            sys.stdout.flush()
        side.synchronize()
    print("# indexed: the index is built inside the timed call; reuse: it was built before")


if __name__ == "__main__":
    main()
