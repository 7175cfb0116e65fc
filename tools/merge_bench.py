#!/usr/bin/env python3
"""Ladder of merge (glu_merge_run_ptr): two sorted arrays of uint32 keys with uint32 values into one, against the two ways there
were to get the same array: this library's sort of the concatenation, and torch's.

    python tools/merge_bench.py [--reps 20] [--quick] [--only TEXT] [--timeout 600] > profiles/merge/ladder.txt

Rows (a_count, b_count), uniform random keys on both sides unless the row says otherwise: (2^27, 2^27), (2^28 - 2^20, 2^20),
(2^24, 2^24), (2^20, 2^20); (2^27, 2^27) with all of A below all of B; (2^27, 2^27) keys only; (2^27, 2^27) with uint64 keys.
Every row runs in a child process of its own under its own timeout, and the ladder stops at the first row that fails.  In a row:
both sides made and sorted on the device once (keys below 2^31, so that torch's signed order is the library's), device events on
the call's stream around the call, 3 warm-up repetitions, median of --reps.  Columns:
  merge     glu_merge_run_ptr after glu_merge_prepare: the partition kernel and the tile kernel; ms
  GB/s      the bytes a merge has to move (every key and every value read once and written once: 16 B a pair for uint32 keys with
            values, 8 keys only, 24 with uint64 keys) over that time, and that rate over the 8 TB/s peak of HBM
  sort      glu_radix_sort_run_typed_ptr on a pristine concatenation A || B (copied in before every repetition, outside the timed
            region) in the same process on the same data; ms; and sort / merge
  torch     torch.sort(torch.cat((a, b)), stable=True) on the int32 / int64 view, the concatenation inside the timed region: keys and
            the permutation, the values would take a gather more; ms; and torch / merge
The merged keys and values of every row are compared with the sort's.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

PEAK_GBS = 8000.0  # HBM3E of one MI355X

ROWS = [
    {"name": "2^27 + 2^27 uint32 pairs", "na": 1 << 27, "nb": 1 << 27, "key_type": "uint32", "vals": True, "data": "uniform"},
    {"name": "2^28-2^20 + 2^20 uint32 pairs", "na": (1 << 28) - (1 << 20), "nb": 1 << 20, "key_type": "uint32", "vals": True, "data": "uniform"},
    {"name": "2^24 + 2^24 uint32 pairs", "na": 1 << 24, "nb": 1 << 24, "key_type": "uint32", "vals": True, "data": "uniform"},
    {"name": "2^20 + 2^20 uint32 pairs", "na": 1 << 20, "nb": 1 << 20, "key_type": "uint32", "vals": True, "data": "uniform"},
    {"name": "2^27 + 2^27 uint32 pairs, disjoint", "na": 1 << 27, "nb": 1 << 27, "key_type": "uint32", "vals": True, "data": "disjoint"},
    {"name": "2^27 + 2^27 uint32 keys only", "na": 1 << 27, "nb": 1 << 27, "key_type": "uint32", "vals": False, "data": "uniform"},
    {"name": "2^27 + 2^27 uint64 pairs", "na": 1 << 27, "nb": 1 << 27, "key_type": "uint64", "vals": True, "data": "uniform"},
]
QUICK_ROWS = [
    {"name": "2^18 + 2^18 uint32 pairs", "na": 1 << 18, "nb": 1 << 18, "key_type": "uint32", "vals": True, "data": "uniform"},
    {"name": "2^18 + 2^10 uint64 keys only, disjoint", "na": 1 << 18, "nb": 1 << 10, "key_type": "uint64", "vals": False, "data": "disjoint"},
]
HEADER = "%-36s %9s %8s %6s | %9s %10s | %9s %11s" % ("row", "merge", "GB/s", "peak", "sort", "sort/merge", "torch", "torch/merge")


def bytes_per_pair(row):
    """What a merge has to move for one output: the key and the value read once and written once."""
    return 2 * ((8 if row["key_type"] == "uint64" else 4) + (4 if row["vals"] else 0))


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
    return float(np.median(times))


def measure(torch, G, stream, row, reps):
    na, nb, key_type, with_vals = row["na"], row["nb"], row["key_type"], row["vals"]
    total = na + nb
    dtype = torch.int32 if key_type == "uint32" else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(total % 1000 + len(key_type))
    if row["data"] == "disjoint":  # all of A below all of B
        a = torch.randint(0, 2 ** 30, (na,), generator=gen, device="cuda", dtype=dtype).sort().values
        b = torch.randint(2 ** 30, 2 ** 31 - 1, (nb,), generator=gen, device="cuda", dtype=dtype).sort().values
    else:
        a = torch.randint(0, 2 ** 31 - 1, (na,), generator=gen, device="cuda", dtype=dtype).sort().values
        b = torch.randint(0, 2 ** 31 - 1, (nb,), generator=gen, device="cuda", dtype=dtype).sort().values
    av = torch.arange(na, dtype=torch.int32, device="cuda") if with_vals else None
    bv = torch.arange(nb, dtype=torch.int32, device="cuda") + (-2 ** 31) if with_vals else None  # (the bits of iota + 2^31)
    out_k = torch.empty(total, dtype=dtype, device="cuda")
    out_v = torch.empty(total, dtype=torch.int32, device="cuda") if with_vals else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    torch.cuda.empty_cache()

    merge = G.Merge()
    merge.prepare(total, key_type)
    res = {"merge": median_ms(torch, reps, lambda: merge.run_ptr(ptr(a), ptr(av), na, ptr(b), ptr(bv), nb, ptr(out_k), ptr(out_v), key_type, stream))}
    assert merge.last() == G.plan_merge(na, nb, key_type, with_vals)[1:3]

    # this library's sort of the concatenation; the copy that makes it pristine again is outside the timed region
    cat_k = torch.cat((a, b))
    cat_v = torch.cat((av, bv)) if with_vals else None
    work_k = torch.empty_like(cat_k)
    work_v = torch.empty_like(cat_v) if with_vals else None
    sort = G.RadixSort()

    def pristine():
        work_k.copy_(cat_k)
        if with_vals:
            work_v.copy_(cat_v)

    res["sort"] = median_ms(torch, reps, lambda: sort.sort_typed_ptr(ptr(work_k), ptr(work_v), total, key_type, stream), pristine)
    assert torch.equal(out_k, work_k), "the merged keys differ from the sort of the concatenation"
    if with_vals:
        assert torch.equal(out_v, work_v), "the merged values differ from the sort of the concatenation"
    del cat_k, cat_v, work_k, work_v, sort
    torch.cuda.empty_cache()
    res["torch"] = median_ms(torch, reps, lambda: torch.sort(torch.cat((a, b)), stable=True))
    return res


def run_row(name, reps):
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    row = next(r for r in ROWS + QUICK_ROWS if r["name"] == name)
    # a stream of our own, made current: the events go where the calls go (the handle of torch's default stream is 0, which the
    # library reads as "the library queue")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r = measure(torch, G, side.cuda_stream, row, reps)
        side.synchronize()
    gbs = bytes_per_pair(row) * (row["na"] + row["nb"]) / (r["merge"] * 1e-3) / 1e9
    print("%-36s %9.4f %8.0f %5.1f%% | %9.4f %10.2f | %9.4f %11.2f" % (
        name, r["merge"], gbs, 100.0 * gbs / PEAK_GBS, r["sort"], r["sort"] / r["merge"], r["torch"], r["torch"] / r["merge"]))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="two small rows only")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only")
    ap.add_argument("--timeout", type=int, default=600, help="seconds a row's process may take")
    ap.add_argument("--row", default=None, help="(internal) measure this row in this process")
    args = ap.parse_args()
    if args.row is not None:
        run_row(args.row, args.reps)
        return 0
    table = [row for row in (QUICK_ROWS if args.quick else ROWS) if args.only is None or args.only in row["name"]]
    print("# device events, 3 warm-up + %d repetitions, median; ms; GB/s = the bytes a merge has to move over the merge's time; "
          "peak = that over %d GB/s" % (args.reps, PEAK_GBS))
    print(HEADER)
    sys.stdout.flush()
    for row in table:
        # a fresh child per row, under its own time limit; a row that fails, dies or runs out of time ends the ladder
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", row["name"], "--reps", str(args.reps)], timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("# %s: no result within %d s; the ladder stops here" % (row["name"], args.timeout))
            return 124
        if p.returncode != 0:
            print("# %s: exit status %d; the ladder stops here" % (row["name"], p.returncode))
            return p.returncode if p.returncode > 0 else 1
    print("# sort: this library's sort of A || B, the copy outside the timed region; torch: torch.sort(torch.cat((a, b)), stable=True)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
