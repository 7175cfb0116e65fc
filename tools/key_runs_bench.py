#!/usr/bin/env python3
"""Ladder of key runs (glu_key_runs_run_ptr): sorted uint32 keys of 2^20 .. 2^28 elements at mean run lengths 1, 4, 256 and
65536, 2^28 keys as one run, 2^26 uint64 keys at mean run length 256 -- and a sort-by-key pipeline of 2^26 pairs.

    python tools/key_runs_bench.py [--reps 20] [--quick] [--only TEXT] > profiles/key_runs/ladder.txt

Every row: keys made on the device once (ascending, a new run wherever a random draw says so; mean run length 1: all distinct),
device events on the call's stream around the call, 3 warm-up repetitions, median of --reps, max_runs = the number of runs.
Columns:
  ms        the whole call (its three kernels)
  B/key     bytes moved per key: two reads of the keys, 4 B + the key size per run, max_runs + 1 offsets
  of peak   bytes moved / ms over 8 TB/s
  stream    glu_reduce_run_batch_ptr over the same array as one partition: a read-only stream of the same bytes, read once
  unique    torch.unique_consecutive(keys, return_counts=True) on the same array (what a PyTorch user has today), and
            unique / ms
The three kernels of a call cannot be told apart by events around the call: their times come from a run of their own under
`rocprofv3 --kernel-trace --stats -- python tools/key_runs_bench.py --only 2^28 --reps 5` (profiles/key_runs/README.md).
The pipeline row: sort_typed_ptr on 2^26 (key, value) pairs with 2^16 distinct keys, then key runs, then the batched reduce of
the values over the runs' offsets with max_runs = 2^16, all on one stream with no host synchronisation between them, beside the
sort alone (every repetition sorts a fresh copy of the same pairs; the copies are outside the events).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

PEAK_BYTES_PER_MS = 8e12 / 1e3
UINT, SUM = 3, 0  # glu::DataType_Uint, glu::ReduceOperator_Sum


def rows(quick):
    out = []
    for lg in ((20, 22) if quick else (20, 24, 26, 28)):
        for mean in (1, 4, 256, 65536):
            out.append({"name": "2^%d uint32, mean run %d" % (lg, mean), "n": 1 << lg, "mean": mean, "bits": 32})
    if not quick:
        out.append({"name": "2^28 uint32, one run", "n": 1 << 28, "mean": 0, "bits": 32})
    out.append({"name": "2^%d uint64, mean run 256" % (22 if quick else 26), "n": 1 << (22 if quick else 26), "mean": 256, "bits": 64})
    return out


def median_ms(torch, reps, call, before=None):
    times = []
    for rep in range(reps + 3):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        if rep >= 3:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def make_keys(torch, row):
    """Ascending keys: key[i] = the number of heads in front of i (times a stride that spreads 8-byte keys over both words)."""
    n, mean = row["n"], row["mean"]
    gen = torch.Generator(device="cuda").manual_seed(n % 1000 + mean)
    if mean == 0:
        heads = torch.zeros(n, dtype=torch.int64, device="cuda")
    elif mean == 1:
        heads = torch.ones(n, dtype=torch.int64, device="cuda")
    else:
        heads = (torch.rand(n, generator=gen, device="cuda") < 1.0 / mean).to(torch.int64)
    heads[0] = 1
    ident = torch.cumsum(heads, 0) - 1
    runs = int(ident[-1].item()) + 1
    if row["bits"] == 64:
        return (ident * 0x100000001), runs
    return ident.to(torch.int32), runs


def measure(torch, G, stream, row, reps):
    keys, runs_n = make_keys(torch, row)
    n, kb = row["n"], row["bits"] // 8
    offsets = torch.empty(runs_n + 1, dtype=torch.int32, device="cuda")
    unique = torch.empty(runs_n * (kb // 4), dtype=torch.int32, device="cuda")
    num = torch.zeros(1, dtype=torch.int32, device="cuda")
    runs = G.KeyRuns()
    runs.prepare(n, row["bits"])
    torch.cuda.synchronize()
    res = {"runs": runs_n}
    res["call"] = median_ms(torch, reps, lambda: runs.run_ptr(keys.data_ptr(), n, offsets.data_ptr(), runs_n, num.data_ptr(), unique.data_ptr(),
                                                               key_bits=row["bits"], stream=stream))
    torch.cuda.synchronize()
    assert int(num.item()) == runs_n and int(offsets[-1].item()) == n, "key runs gave a wrong number of runs"
    # the read-only stream: the batched reduce over the same bytes as one partition of 4-byte elements
    red = G.Reduce(UINT, SUM)
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    words = n * (kb // 4)
    red.run_batch_ptr(keys.data_ptr(), out.data_ptr(), words, 1, stream)
    torch.cuda.synchronize()
    res["stream"] = median_ms(torch, reps, lambda: red.run_batch_ptr(keys.data_ptr(), out.data_ptr(), words, 1, stream))
    res["unique"] = median_ms(torch, reps, lambda: torch.unique_consecutive(keys, return_counts=True))
    res["bytes"] = 2.0 * n * kb + runs_n * (4.0 + kb) + 4.0 * (runs_n + 1)
    return res


def pipeline(torch, G, stream, reps, lg):
    n, distinct = 1 << lg, 1 << 16
    gen = torch.Generator(device="cuda").manual_seed(5)
    keys0 = (torch.randint(0, distinct, (n,), generator=gen, device="cuda", dtype=torch.int32) * 40503)
    vals0 = torch.randint(0, 1000, (n,), generator=gen, device="cuda", dtype=torch.int32)
    keys, vals = keys0.clone(), vals0.clone()
    offsets = torch.empty(distinct + 1, dtype=torch.int32, device="cuda")
    unique = torch.empty(distinct, dtype=torch.int32, device="cuda")
    sums = torch.empty(distinct, dtype=torch.int32, device="cuda")
    num = torch.zeros(1, dtype=torch.int32, device="cuda")
    sort, runs, red = G.RadixSort(), G.KeyRuns(), G.Reduce(UINT, SUM)
    sort.prepare_internal_buffers(n, 4, True)
    runs.prepare(n)
    red.prepare_batch(n, distinct)

    def fresh():
        keys.copy_(keys0)
        vals.copy_(vals0)

    def sort_only():
        sort.sort_typed_ptr(keys.data_ptr(), vals.data_ptr(), n, "uint32", stream)

    def group_by():
        sort_only()
        red.run_by_key_ptr(runs, keys.data_ptr(), vals.data_ptr(), sums.data_ptr(), n, offsets.data_ptr(), distinct, num.data_ptr(),
                           unique.data_ptr(), stream=stream)

    a = median_ms(torch, reps, sort_only, fresh)
    b = median_ms(torch, reps, group_by, fresh)
    torch.cuda.synchronize()
    assert int(num.item()) == distinct and int(sums.to(torch.int64).sum().item()) == int(vals0.to(torch.int64).sum().item())
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="2^20 and 2^22 rows only, a pipeline of 2^22 pairs")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only (e.g. '2^28' under a profiler); no pipeline")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    table = [row for row in rows(args.quick) if args.only is None or args.only in row["name"]]
    print("# %s" % G.device_info())
    print("# device events, 3 warm-up + %d repetitions, median (min .. max); max_runs = runs" % args.reps)
    print("%-28s %10s %9s %21s %7s %8s | %9s %7s | %9s %7s" % ("row", "runs", "ms", "(min .. max)", "B/key", "of peak", "stream ms", "2x/ms",
                                                             "unique ms", "uniq/ms"))
    # a stream of our own, made current: the events go where the calls go (the handle of torch's default stream is 0, which the
    # library reads as "the library queue")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for row in table:
            r = measure(torch, G, side.cuda_stream, row, args.reps)
            ms, lo, hi = r["call"]
            print("%-28s %10d %9.4f %21s %7.2f %7.1f%% | %9.4f %7.3f | %9.4f %7.2f" % (
                row["name"], r["runs"], ms, "(%.4f .. %.4f)" % (lo, hi), r["bytes"] / row["n"], 100.0 * r["bytes"] / ms / PEAK_BYTES_PER_MS,
                r["stream"][0], 2.0 * r["stream"][0] / ms, r["unique"][0], r["unique"][0] / ms))
            sys.stdout.flush()
            torch.cuda.empty_cache()
        if args.only is None:
            lg = 22 if args.quick else 26
            a, b = pipeline(torch, G, side.cuda_stream, args.reps, lg)
            print("# sort by key of 2^%d (uint32, uint32) pairs with 2^16 distinct keys: %.4f ms (%.4f .. %.4f)" % ((lg,) + a))
            print("# the same, then key runs and the batched reduce (Sum) of the values, max_runs = 2^16: %.4f ms (%.4f .. %.4f): "
                  "group-by costs %.4f ms (%.1f%%) on top of the sort" % (b + (b[0] - a[0], 100.0 * (b[0] - a[0]) / a[0])))
        side.synchronize()
    print("# column 2x/ms: twice the read-only stream (the call reads the keys twice) over the call")


if __name__ == "__main__":
    main()
