#!/usr/bin/env python3
"""Ladder of top-k (glu_top_k_run_ptr) against what a caller did before it existed (this library's typed sort of a copy), against
torch.topk, and against the floor of its reads (this library's Reduce of the same array, times the reads the row's path makes).

    python tools/top_k_bench.py [--reps 10] [--quick] [--only TEXT] [--timeout 600] [--out profiles/top_k/ladder.txt]

Rows: uint32 and float32 at 2^20, 2^24 and 2^28 keys, uint64 at 2^28 x k in {1, 1024, 2^20 (where it is at most the count), count / 8}
x {sorted, unsorted} x {uniform, equal, zipf}, the k largest with keys and indices.  Every block of rows of one size and type runs in
a child process of its own under its own timeout, and the ladder stops at the first block that fails.  The keys are made on the
device once per block and data:
  uniform  every value of the lower half of the type's unsigned range (uint32 below 2^31 and uint64 below 2^63, so that torch's signed
           order is the library's), floats uniform in [0, 1)
  equal    one value: the FULL path, every round reads the input again
  zipf     floor(R^u) for uniform u and R the range above: P(value = v) ~ 1 / v, the continuous form of Zipf(1.0)
Device events on the call's stream around the call, 3 warm-up repetitions, median of --reps (a call that takes more than 50 ms: 1 and
3).  Columns, ms:
  topk     the call after glu_top_k_prepare, all its kernels; the path as read_last() states it
  sort     (a) glu_radix_sort_run_typed_ptr of a copy of the keys with iota values, the copies outside the timed region; and sort / topk
  torch    (b) torch.topk(largest=True, sorted=the row's) of the same tensor; and torch / topk
  floor    (c) glu_reduce_run_batch_ptr (sum, one partition) of the same array, times the full reads of the row's path: 4 on
           CANDIDATES (count, collect, and the two of the compaction), the digit rounds + 2 on FULL; and topk / floor
The keys of every row are compared with torch's (as sorted multisets where the row is unsorted).
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

BLOCKS = [("uint32", 20), ("float32", 20), ("uint32", 24), ("float32", 24), ("uint32", 28), ("float32", 28), ("uint64", 28)]
INPUTS = ["uniform", "equal", "zipf"]
HEADER = "%-44s %9s %5s | %9s %9s | %9s %10s | %9s %10s" % ("row", "topk", "path", "sort", "sort/topk", "torch", "torch/topk", "floor",
                                                          "topk/floor")


def median_ms(torch, reps, call, setup=None):
    """3 warm-up + `reps` repetitions, median; a call that takes more than 50 ms gets 1 warm-up + 3 repetitions."""
    times = []
    warm, rep = 3, 0
    while rep < warm + reps:
        if setup:
            setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        if rep == 0 and a.elapsed_time(b) > 50.0:
            warm, reps = 1, min(reps, 3)
        if rep >= warm:
            times.append(a.elapsed_time(b))
        rep += 1
    return float(np.median(times))


def make_keys(torch, gen, kind, n, data):
    if kind == "float32":
        if data == "equal":
            return torch.full((n,), 0.625, device="cuda", dtype=torch.float32)
        u = torch.rand(n, generator=gen, device="cuda", dtype=torch.float32)
        return u if data == "uniform" else torch.pow(torch.tensor(2.0 ** 31, device="cuda"), u).floor()
    bits, dt = (31, torch.int32) if kind == "uint32" else (63, torch.int64)
    if data == "equal":
        return torch.full((n,), 123456789, device="cuda", dtype=dt)
    if data == "uniform":
        return torch.randint(0, 2 ** bits - 1, (n,), generator=gen, device="cuda", dtype=torch.int64).to(dt)
    u = torch.rand(n, generator=gen, device="cuda", dtype=torch.float64)
    return torch.pow(torch.tensor(2.0 ** bits, device="cuda", dtype=torch.float64), u).floor().clamp_(0, 2.0 ** bits - 2 ** 11).to(dt)


def run_block(kind, log2n, reps, only):
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    n = 1 << log2n
    kb = 8 if kind == "uint64" else 4
    rounds = G.plan_top_k(n, 1, kind)["rounds"]
    ks = sorted({1, 1024, n // 8} | ({1 << 20} if (1 << 20) <= n else set()))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s = side.cuda_stream
        gen = torch.Generator(device="cuda").manual_seed(log2n + kb)
        top = G.TopK()
        top.prepare(n, max(ks), kind)
        sorter = G.RadixSort()
        sorter.prepare_internal_buffers(n, kb, True)
        red = G.Reduce(G.DataType_Double if kb == 8 else G.DataType_Uint, G.ReduceOperator_Sum)
        red_out = torch.empty(4, dtype=torch.int64, device="cuda")
        iota = torch.arange(n, device="cuda", dtype=torch.int32)
        for data in INPUTS:
            if only is not None and data not in only and any(d in only for d in INPUTS):
                continue
            x = make_keys(torch, gen, kind, n, data)
            copy, vals = torch.empty_like(x), torch.empty_like(iota)
            sort_ms = median_ms(torch, reps, lambda: sorter.sort_typed_ptr(copy.data_ptr(), vals.data_ptr(), n, kind, s),
                                setup=lambda: (copy.copy_(x), vals.copy_(iota)))
            del copy, vals
            read_ms = median_ms(torch, reps, lambda: red.run_batch_ptr(x.data_ptr(), red_out.data_ptr(), n, 1, s))
            for k in ks:
                for sorted_ in (True, False):
                    name = "2^%d %s, k %d, %s, %s" % (log2n, kind, k, "sorted" if sorted_ else "unsorted", data)
                    if only is not None and not all(part in name for part in only.split(",")):
                        continue
                    ok, oi = torch.empty(k, dtype=x.dtype, device="cuda"), torch.empty(k, dtype=torch.int32, device="cuda")
                    call = lambda: top.run_ptr(x.data_ptr(), n, k, ok.data_ptr(), oi.data_ptr(), None, kind, True, sorted_, s)
                    topk_ms = median_ms(torch, reps, call)
                    side.synchronize()
                    last = top.read_last()
                    theirs = lambda: torch.topk(x, k, largest=True, sorted=sorted_)
                    want = theirs().values
                    if sorted_:
                        assert torch.equal(ok, want), "the keys differ from torch.topk's"
                    else:
                        assert torch.equal(ok.sort().values, want.sort().values), "the keys differ from torch.topk's"
                    assert torch.equal(x[oi.to(torch.int64)], ok), "the indices do not point at the keys"
                    del want
                    torch_ms = median_ms(torch, reps, theirs)
                    floor_ms = read_ms * (4 if last["path"] == G.TopKPath_Candidates else rounds + 2)
                    print("%-44s %9.4f %5s | %9.4f %9.2f | %9.4f %10.2f | %9.4f %10.2f" % (
                        name, topk_ms, "CAND" if last["path"] == G.TopKPath_Candidates else "FULL", sort_ms, sort_ms / topk_ms, torch_ms,
                        torch_ms / topk_ms, floor_ms, topk_ms / floor_ms))
                    sys.stdout.flush()
                    del ok, oi
            del x
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="2^20 keys only")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only (several texts, separated by commas: all of them)")
    ap.add_argument("--timeout", type=int, default=600, help="seconds a block's process may take")
    ap.add_argument("--out", default=None, help="write the ladder to this file as well as to stdout")
    ap.add_argument("--block", default=None, help="(internal) KIND:LOG2N, measured in this process")
    args = ap.parse_args()
    if args.block is not None:
        kind, log2n = args.block.split(":")
        run_block(kind, int(log2n), args.reps, args.only)
        return 0
    lines = []

    def say(text):
        print(text)
        sys.stdout.flush()
        lines.append(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("# device events, 3 warm-up + %d repetitions, median; ms; the k largest with keys and indices" % args.reps)
    say(HEADER)
    for kind, log2n in BLOCKS:
        if args.quick and log2n != 20:
            continue
        if args.only is not None and any(p.startswith("2^") and p != "2^%d %s" % (log2n, kind) for p in args.only.split(",")):
            continue
        # a fresh child per block, under its own time limit; a block that fails, dies or runs out of time ends the ladder
        cmd = [sys.executable, os.path.abspath(__file__), "--block", "%s:%d" % (kind, log2n), "--reps", str(args.reps)]
        if args.only is not None:
            cmd += ["--only", args.only]
        try:
            p = subprocess.run(cmd, timeout=args.timeout, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            say("# 2^%d %s: no result within %d s; the ladder stops here" % (log2n, kind, args.timeout))
            return 124
        for line in p.stdout.splitlines():
            say(line)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            say("# 2^%d %s: exit status %d; the ladder stops here" % (log2n, kind, p.returncode))
            return p.returncode if p.returncode > 0 else 1
    say("# sort: the typed sort of a copy of the keys with iota values; torch: torch.topk; floor: Reduce of the same array x the full "
        "reads of the path (4 on CAND, the digit rounds + 2 on FULL)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
