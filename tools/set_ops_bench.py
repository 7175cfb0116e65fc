#!/usr/bin/env python3
"""Ladder of the set operations (glu_set_ops_run_ptr): union, intersection, difference and symmetric difference of two sorted arrays,
against this library's merge of the same inputs, and for the intersection against torch.

    python tools/set_ops_bench.py [--reps 20] [--quick] [--only TEXT] [--timeout 600] > profiles/set_ops/ladder.txt

Rows: 2^27 + 2^27 uint32 pairs with about half of the keys shared (B = every second key of A and as many fresh ones), all four
operations and a call that only counts; the same with keys alone; the same with uint64 pairs; 2^24 + 2^24 and 2^20 + 2^20 union and
intersection; 2^27 + 2^27 with all of A below all of B; 2^27 + 2^27 identical arrays.  Every row runs in a child process of its own
under its own timeout, and the ladder stops at the first row that fails.  In a row: both sides made and sorted on the device once
(keys below 2^31, so that torch's signed order is the library's), device events on the call's stream around the call, 3 warm-up
repetitions, median of --reps.  Columns:
  set op    glu_set_ops_run_ptr after glu_set_ops_prepare: bounds, count, scan and write (no write for "count"); ms
  S/total   the kept elements over a_count + b_count
  merge     glu_merge_run_ptr after glu_merge_prepare on the same inputs in the same process (with values where the row has them): the
            yardstick -- a union writes at most what merge writes and reads the keys once more; ms; and set op / merge
  torch     intersection rows only: torch.isin(a, b, assume_unique=False) followed by torch.masked_select(a, mask), keys alone; ms;
            and torch / set op
The kept keys of every row are checked to be in order, and their number where the row's data give it in closed form.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

OPS = ("union", "intersection", "difference", "symmetric_difference", "count")  # count: a union that only counts


def rows_of(n, key_type, vals, data, ops):
    shape = "2^%d + 2^%d %s %s" % (n.bit_length() - 1, n.bit_length() - 1, key_type, "pairs" if vals else "keys")
    return [{"name": "%s, %s: %s" % (shape, data, op), "na": n, "nb": n, "key_type": key_type, "vals": vals, "data": data, "op": op} for op in ops]


ROWS = (rows_of(1 << 27, "uint32", True, "half shared", OPS) + rows_of(1 << 27, "uint32", False, "half shared", OPS[:4]) +
        rows_of(1 << 27, "uint64", True, "half shared", OPS) + rows_of(1 << 24, "uint32", True, "half shared", OPS[:2]) +
        rows_of(1 << 20, "uint32", True, "half shared", OPS[:2]) + rows_of(1 << 27, "uint32", True, "disjoint", OPS[:2]) +
        rows_of(1 << 27, "uint32", True, "identical", OPS[:3]))
QUICK_ROWS = rows_of(1 << 18, "uint32", True, "half shared", OPS) + rows_of(1 << 18, "uint64", False, "identical", OPS[:2])
HEADER = "%-58s %9s %8s | %9s %12s | %9s %12s" % ("row", "set op", "S/total", "merge", "set op/merge", "torch", "torch/set op")


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


def measure(torch, G, stream, row, reps):
    na, nb, key_type, with_vals, op = row["na"], row["nb"], row["key_type"], row["vals"], row["op"]
    total = na + nb
    dtype = torch.int32 if key_type == "uint32" else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(total % 1000 + len(key_type))
    draw = lambda lo, hi, n: torch.randint(lo, hi, (n,), generator=gen, device="cuda", dtype=dtype)
    if row["data"] == "disjoint":  # all of A below all of B
        a, b = draw(0, 2 ** 30, na).sort().values, draw(2 ** 30, 2 ** 31 - 1, nb).sort().values
    elif row["data"] == "identical":
        a = draw(0, 2 ** 31 - 1, na).sort().values
        b = a.clone()
    else:  # about half of the keys shared: every second key of A, and as many fresh ones
        a = draw(0, 2 ** 31 - 1, na).sort().values
        b = torch.cat((a[::2], draw(0, 2 ** 31 - 1, nb - (na + 1) // 2))).sort().values
    count_only = op == "count"
    with_vals = with_vals and not count_only
    av = torch.arange(na, dtype=torch.int32, device="cuda") if with_vals else None
    bv = torch.arange(nb, dtype=torch.int32, device="cuda") + (-2 ** 31) if with_vals else None  # (the bits of iota + 2^31)
    out_k = torch.empty(total, dtype=dtype, device="cuda")
    out_v = torch.empty(total, dtype=torch.int32, device="cuda") if with_vals else None
    num = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else None
    torch.cuda.empty_cache()

    set_ops = G.SetOps()
    set_ops.prepare(total, key_type)
    name = "union" if count_only else op
    b_vals = ptr(bv) if name in ("union", "symmetric_difference") else None
    call = lambda: set_ops.run_ptr(name, ptr(a), ptr(av), na, ptr(b), b_vals, nb, None if count_only else ptr(out_k), ptr(out_v),
                                   0 if count_only else total, ptr(num), key_type, stream)
    res = {"set": median_ms(torch, reps, call)}
    assert set_ops.last() == G.plan_set_ops(na, nb, key_type, not count_only)[1:3]
    S = int(num.cpu().numpy().view(np.uint32)[0])
    res["S"] = S
    if not count_only and S > 1:
        assert bool((out_k[1:S] >= out_k[:S - 1]).all()), "the kept keys are not in order"
    closed = {("disjoint", "union"): total, ("disjoint", "intersection"): 0, ("identical", "union"): na, ("identical", "intersection"): na,
              ("identical", "difference"): 0}
    assert closed.get((row["data"], name), S) == S, (S, closed[(row["data"], name)])

    merge = G.Merge()
    merge.prepare(total, key_type)
    mv = row["vals"]
    if mv and av is None:
        av = torch.arange(na, dtype=torch.int32, device="cuda")
        bv = torch.arange(nb, dtype=torch.int32, device="cuda") + (-2 ** 31)
        out_v = torch.empty(total, dtype=torch.int32, device="cuda")
    res["merge"] = median_ms(torch, reps, lambda: merge.run_ptr(ptr(a), ptr(av) if mv else None, na, ptr(b), ptr(bv) if mv else None, nb, ptr(out_k),
                                                                ptr(out_v) if mv else None, key_type, stream))
    res["torch"] = None
    if op == "intersection":
        del out_k, out_v
        torch.cuda.empty_cache()
        res["torch"] = median_ms(torch, reps, lambda: torch.masked_select(a, torch.isin(a, b, assume_unique=False)))
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
    torch_cols = "%9.4f %12.2f" % (r["torch"], r["torch"] / r["set"]) if r["torch"] is not None else "%9s %12s" % ("-", "-")
    print("%-58s %9.4f %8.3f | %9.4f %12.2f | %s" % (name, r["set"], r["S"] / (row["na"] + row["nb"]), r["merge"], r["set"] / r["merge"], torch_cols))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="a few small rows only")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only")
    ap.add_argument("--timeout", type=int, default=600, help="seconds a row's process may take")
    ap.add_argument("--row", default=None, help="(internal) measure this row in this process")
    args = ap.parse_args()
    if args.row is not None:
        run_row(args.row, args.reps)
        return 0
    table = [row for row in (QUICK_ROWS if args.quick else ROWS) if args.only is None or args.only in row["name"]]
    print("# device events, 3 warm-up + %d repetitions, median; ms; merge: this library's merge of the same inputs in the same process" % args.reps)
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
    print("# torch: torch.masked_select(a, torch.isin(a, b, assume_unique=False)), keys alone")
    return 0


if __name__ == "__main__":
    sys.exit(main())
