#!/usr/bin/env python3
"""Ladder of gather and scatter (glu_gather_run_ptr, glu_gather_scatter_ptr, glu_gather_run_batch_ptr): items fetched or placed by
device indices, against torch in the same process on the same data, and on the identity row against this library's select with
everything selected.

    python tools/gather_bench.py [--reps 20] [--quick] [--only TEXT] [--timeout 600] > profiles/gather/ladder.txt

Every row runs in a child process of its own under its own timeout, and the ladder stops at the first row that fails.  In a row the
data are made on the device once; device events on the call's stream around the call, 3 warm-up repetitions, median of --reps.
Columns:
  glu       the library's call; ms
  MB        the bytes per output that the call must move: 4 for the index, item_bytes written, item_bytes of useful read
  GB/s      that over the time, and that rate over the 8 TB/s peak of HBM
  (a)       gather: torch.index_select(items, 0, indices) with the int32 indices; scatter: out.index_copy_(0, indices, items);
            batched: torch.gather(items as rows, 1, indices as int64, made outside the timed region); ms, and (a) / glu
  (b)       gather: items[indices as int64], the int64 indices made outside the timed region; ms, and (b) / glu
            `refused` under (a) or (b): torch does not launch that call at this size ("invalid configuration argument")
  select    the identity row only: glu_select_run_ptr with every element selected (stencil != 0) and 4-byte items, out_items
            alone: it streams 4 bytes of stencil and 4 of item in and 4 out, the same 12 bytes per element; GB/s, ms, and the
            gather's time per byte over the select's (the bar is 1.10)
The library's output of every row is compared with torch's.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

PEAK_GBS = 8000.0  # HBM3E of one MI355X
N = 1 << 28


def rows():
    out = []
    for order in ("random", "sorted random"):
        for e in (20, 24, 28):
            out.append({"name": "gather 4 B, table 2^%d, %s" % (e, order), "op": "gather", "bytes": 4, "count": N, "table": 1 << e,
                        "index": order})
    out.append({"name": "gather 4 B, identity", "op": "gather", "bytes": 4, "count": N, "table": N, "index": "identity"})
    out.append({"name": "gather 4 B, the sort's permutation", "op": "gather", "bytes": 4, "count": N, "table": N, "index": "sort"})
    for b in (8, 16, 32):
        out.append({"name": "gather %d B, table 2^28, random" % b, "op": "gather", "bytes": b, "count": N, "table": N, "index": "random"})
    for b in (4, 16):
        out.append({"name": "scatter %d B, random permutation" % b, "op": "scatter", "bytes": b, "count": N, "table": N, "index": "permutation"})
    for e in (24, 20):
        out.append({"name": "gather 4 B, 2^%d outputs, random" % e, "op": "gather", "bytes": 4, "count": 1 << e, "table": 1 << e,
                    "index": "random"})
    out.append({"name": "batched 4 B, 65536 rows of 1024, k 32", "op": "batch", "bytes": 4, "rows": 65536, "len": 1024, "k": 32})
    out.append({"name": "batched 4 B, 1024 rows of 32768, k 50", "op": "batch", "bytes": 4, "rows": 1024, "len": 32768, "k": 50})
    return out


QUICK_ROWS = [{"name": "gather 4 B, 2^18 outputs, random", "op": "gather", "bytes": 4, "count": 1 << 18, "table": 1 << 18, "index": "random"},
              {"name": "scatter 16 B, 2^18, random permutation", "op": "scatter", "bytes": 16, "count": 1 << 18, "table": 1 << 18,
               "index": "permutation"},
              {"name": "batched 4 B, 256 rows of 1024, k 32", "op": "batch", "bytes": 4, "rows": 256, "len": 1024, "k": 32}]
HEADER = "%-40s %9s %8s %7s %6s | %9s %8s | %9s %8s | %s" % ("row", "glu", "MB", "GB/s", "peak", "(a)", "(a)/glu", "(b)", "(b)/glu", "select")


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


def refusable(torch, reps, call):
    """median_ms, or NaN where torch refuses the launch ("invalid configuration argument": 2^28 rows of 16 bytes and more)"""
    try:
        return median_ms(torch, reps, call)
    except RuntimeError as e:
        if "invalid configuration" not in str(e):
            raise
        return float("nan")


def make_indices(torch, G, stream, row):
    """int32 indices on the device"""
    count, table, kind = row["count"], row["table"], row["index"]
    gen = torch.Generator(device="cuda").manual_seed(table % 1000 + len(kind))
    if kind == "identity":
        return torch.arange(count, dtype=torch.int32, device="cuda")
    if kind == "permutation":
        return torch.randperm(count, generator=gen, device="cuda").to(torch.int32)
    if kind == "sort":  # what this library's sort of uniform keys leaves in its values
        keys = torch.randint(-2 ** 31, 2 ** 31 - 1, (count,), generator=gen, dtype=torch.int32, device="cuda")
        vals = torch.arange(count, dtype=torch.int32, device="cuda")
        torch.cuda.current_stream().synchronize()
        G.RadixSort().sort_typed_ptr(keys.data_ptr(), vals.data_ptr(), count, "uint32", stream)
        torch.cuda.current_stream().synchronize()
        return vals
    idx = torch.randint(0, table, (count,), generator=gen, dtype=torch.int32, device="cuda")
    if kind == "sorted random":
        idx = torch.sort(idx).values
    return idx


def measure_flat(torch, G, stream, row, reps):
    count, table, b = row["count"], row["table"], row["bytes"]
    words = b // 4
    idx = make_indices(torch, G, stream, row)
    gather = G.Gather()
    extra = ""
    if row["op"] == "gather":
        items = torch.randint(0, 2 ** 31 - 1, (table, words), dtype=torch.int32, device="cuda")
        out = torch.empty((count, words), dtype=torch.int32, device="cuda")
        torch.cuda.current_stream().synchronize()
        ms = median_ms(torch, reps, lambda: gather.run_ptr(items.data_ptr(), table, b, idx.data_ptr(), count, out.data_ptr(), stream))
        assert gather.last() == G.plan_gather(count, b)[1:3]
        a_ms = refusable(torch, reps, lambda: torch.index_select(items, 0, idx))
        for a in range(0, count, 1 << 24):  # (in pieces: torch refuses some of these launches whole)
            assert torch.equal(out[a:a + (1 << 24)], torch.index_select(items, 0, idx[a:a + (1 << 24)])), "the gather differs from torch.index_select"
        idx64 = idx.long()
        b_ms = refusable(torch, reps, lambda: items[idx64])
        del idx64
        if row["index"] == "identity":  # this library's select with everything selected, the same 12 bytes per element
            stencil = torch.ones(count, dtype=torch.int32, device="cuda")
            num = torch.zeros(1, dtype=torch.int32, device="cuda")
            out.fill_(0)
            select = G.Select()
            select.prepare(count, G.SelectStencil_Uint)
            torch.cuda.current_stream().synchronize()
            s_ms = median_ms(torch, reps, lambda: select.run_ptr(stencil.data_ptr(), count, count, num.data_ptr(), items_ptr=items.data_ptr(),
                                                                 out_items_ptr=out.data_ptr(), item_bytes=4,
                                                                 stencil_type=G.SelectStencil_Uint, op=G.SelectOperator_NE, threshold=0,
                                                                 stream=stream))
            assert int(num.item()) == count and torch.equal(out, items)
            moved = 12.0 * count
            extra = "%5.0f GB/s, %6.4f ms, gather / select per byte %.2f" % (moved / (s_ms * 1e-3) / 1e9, s_ms, ms / s_ms)
    else:
        items = torch.randint(0, 2 ** 31 - 1, (count, words), dtype=torch.int32, device="cuda")
        out = torch.zeros((table, words), dtype=torch.int32, device="cuda")
        torch.cuda.current_stream().synchronize()
        ms = median_ms(torch, reps, lambda: gather.scatter_ptr(items.data_ptr(), b, idx.data_ptr(), count, out.data_ptr(), table, stream))
        want = torch.zeros((table, words), dtype=torch.int32, device="cuda")
        try:
            a_ms = median_ms(torch, reps, lambda: want.index_copy_(0, idx, items))
        except (RuntimeError, IndexError):  # (a torch that takes int64 indices alone: made outside the timed region)
            idx64 = idx.long()
            a_ms = median_ms(torch, reps, lambda: want.index_copy_(0, idx64, items))
            del idx64
        assert torch.equal(out, want), "the scatter differs from torch's index_copy_"
        b_ms = None
    return ms, (4.0 + 2 * b) * count, a_ms, b_ms, extra


def measure_batch(torch, G, stream, row, reps):
    n, length, k, b = row["rows"], row["len"], row["k"], row["bytes"]
    gen = torch.Generator(device="cuda").manual_seed(n % 1000 + k)
    keys = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, length), generator=gen, dtype=torch.int32, device="cuda")
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    out = torch.empty((n, k), dtype=torch.int32, device="cuda")
    topk, gather = G.TopK(), G.Gather()
    torch.cuda.current_stream().synchronize()
    topk.run_batch_ptr(keys.data_ptr(), length, n, k, None, idx.data_ptr(), None, "uint32", True, True, stream)  # the real producer
    torch.cuda.current_stream().synchronize()
    ms = median_ms(torch, reps, lambda: gather.run_batch_ptr(keys.data_ptr(), b, length, n, idx.data_ptr(), k, out.data_ptr(), stream))
    assert gather.last() == G.plan_gather(n * k, b)[1:3]
    idx64 = idx.long()
    a_ms = median_ms(torch, reps, lambda: torch.gather(keys, 1, idx64))
    assert torch.equal(out, torch.gather(keys, 1, idx64)), "the batched gather differs from torch.gather"
    return ms, (4.0 + 2 * b) * n * k, a_ms, None, ""


def run_row(name, reps):
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    row = next(r for r in rows() + QUICK_ROWS if r["name"] == name)
    # a stream of our own, made current: the events go where the calls go (the handle of torch's default stream is 0, which the
    # library reads as "the library queue")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ms, moved, a_ms, b_ms, extra = (measure_batch if row["op"] == "batch" else measure_flat)(torch, G, side.cuda_stream, row, reps)
        side.synchronize()
    gbs = moved / (ms * 1e-3) / 1e9
    cell = lambda v: "%9s %8s" % ("-", "-") if v is None else "%9s %8s" % ("refused", "-") if v != v else "%9.4f %8.2f" % (v, v / ms)
    print("%-40s %9.4f %8.1f %7.0f %5.1f%% | %s | %s | %s" % (name, ms, moved / 1e6, gbs, 100.0 * gbs / PEAK_GBS, cell(a_ms), cell(b_ms), extra or "-"))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="three small rows only")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only")
    ap.add_argument("--timeout", type=int, default=600, help="seconds a row's process may take")
    ap.add_argument("--row", default=None, help="(internal) measure this row in this process")
    args = ap.parse_args()
    if args.row is not None:
        run_row(args.row, args.reps)
        return 0
    table = [row for row in (QUICK_ROWS if args.quick else rows()) if args.only is None or args.only in row["name"]]
    print("# device events, 3 warm-up + %d repetitions, median; ms; MB = per output 4 bytes of index, the item written and the item read; "
          "peak = GB/s over %d GB/s" % (args.reps, PEAK_GBS))
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
    print("# (a): torch.index_select / index_copy_ / torch.gather; (b): items[indices as int64]; select: glu_select_run_ptr with every "
          "element selected, on the identity row")
    return 0


if __name__ == "__main__":
    sys.exit(main())
