#!/usr/bin/env python3
"""Ladder of histogram (glu_histogram_run_even_ptr, glu_histogram_run_edges_ptr) against torch and against this library's Reduce of
the same array, the floor of one read.

    python tools/histogram_bench.py [--reps 20] [--quick] [--only TEXT] [--timeout 600] [--out profiles/histogram/ladder.txt]

Rows: 2^20, 2^24 and 2^28 samples x {uint32 even bins, float32 even bins, uint64 edges} x {256, 8192, 2^20 bins; edges: 256 and
8192} x {uniform, constant, zipf}.  Every block of rows of one size and type runs in a child process of its own under its own
timeout, and the ladder stops at the first block that fails.  In a row the samples are made on the device once:
  uint32   x = 16 * id + 4 random low bits, lo = 0, hi = 16 * bins (W = 16: the exact division is part of what is timed)
  float32  x = (id + a random fraction) / bins, lo = 0, hi = 1
  uint64   x = id * step + a random offset below step, edges[k] = k * step, step = 2^62 / bins (below 2^63: torch's signed order is
           the library's)
with id the bin the sample is meant for: uniform over the bins; constant = bins / 3; zipf = floor(bins^u) - 1 for uniform u, that is
P(id = k) ~ log((k + 2) / (k + 1)), the continuous form of Zipf(1.0) over the bins.  Device events on the call's stream around the
call, 3 warm-up repetitions, median of --reps.  Columns, ms:
  hist     the call after glu_histogram_prepare, all its kernels; path and workgroups as last() states them
  GB/s     the bytes the call has to read (4 or 8 a sample) over that time, and that rate over the 8 TB/s peak of HBM
  reduce   glu_reduce_run_batch_ptr (sum, one partition) over the same array in the same process: one read, no bins
  torch    uint32: torch.bincount of the ids (x >> 4, made outside the timed region), minlength = bins; float32: torch.histc;
           uint64: torch.searchsorted(edges, x, right=True) followed by torch.bincount; and torch / hist
The counts of every integer row are compared with torch's; histc works and counts in float32 (its bins differ beside the edges,
and a count stops at 2^24), so the float32 rows only check that no sample was lost (tests/test_gpu_histogram.py holds the counts
against numpy).  A call that takes more than 50 ms is repeated 3 times after 1 warm-up.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

PEAK_GBS = 8000.0  # HBM3E of one MI355X
SIZES = [20, 24, 28]
KINDS = ["uint32", "float32", "uint64"]
BINS = {"uint32": [256, 8192, 1 << 20], "float32": [256, 8192, 1 << 20], "uint64": [256, 8192]}
INPUTS = ["uniform", "constant", "zipf"]
HEADER = "%-40s %9s %7s %6s %6s %6s | %9s %9s | %9s %10s" % ("row", "hist", "GB/s", "peak", "path", "groups", "reduce", "hist/red", "torch", "torch/hist")


def median_ms(torch, reps, call):
    """3 warm-up + `reps` repetitions, median; a call that takes more than 50 ms gets 1 warm-up + 3 repetitions."""
    times = []
    warm, rep = 3, 0
    while rep < warm + reps:
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


def make_ids(torch, gen, n, bins, data):
    if data == "uniform":
        return torch.randint(0, bins, (n,), generator=gen, device="cuda", dtype=torch.int64)
    if data == "constant":
        return torch.full((n,), bins // 3, device="cuda", dtype=torch.int64)
    u = torch.rand(n, generator=gen, device="cuda", dtype=torch.float64)
    return (torch.pow(torch.tensor(float(bins), device="cuda", dtype=torch.float64), u).floor().to(torch.int64) - 1).clamp_(0, bins - 1)


def measure(torch, G, stream, kind, n, bins, data, reps):
    gen = torch.Generator(device="cuda").manual_seed(n % 1000 + bins % 1000 + len(data))
    ids = make_ids(torch, gen, n, bins, data)
    out = torch.empty(bins, dtype=torch.int32, device="cuda")
    hist = G.Histogram()
    hist.prepare(n, bins)
    if kind == "uint32":
        x = (ids * 16 + torch.randint(0, 16, (n,), generator=gen, device="cuda", dtype=torch.int64)).to(torch.int32)  # (below 2^31)
        ids32 = ids.to(torch.int32)
        call = lambda: hist.run_even_ptr(x.data_ptr(), n, 0, 16 * bins, bins, out.data_ptr(), "uint32", False, stream)
        theirs = lambda: torch.bincount(ids32, minlength=bins)
        reduce_type, elem = G.DataType_Uint, 4
    elif kind == "float32":
        x = ((ids.to(torch.float64) + torch.rand(n, generator=gen, device="cuda", dtype=torch.float64)) / bins).to(torch.float32)
        x = x.clamp_(0.0, float(np.nextafter(np.float32(1), np.float32(0))))
        call = lambda: hist.run_even_ptr(x.data_ptr(), n, 0.0, 1.0, bins, out.data_ptr(), "float32", False, stream)
        theirs = lambda: torch.histc(x, bins=bins, min=0.0, max=1.0)
        reduce_type, elem = G.DataType_Float, 4
    else:
        step = (1 << 62) // bins
        x = ids * step + torch.randint(0, step, (n,), generator=gen, device="cuda", dtype=torch.int64)
        edges = torch.arange(bins + 1, device="cuda", dtype=torch.int64) * step
        call = lambda: hist.run_edges_ptr(x.data_ptr(), n, edges.data_ptr(), bins, out.data_ptr(), "uint64", False, stream)
        theirs = lambda: torch.bincount(torch.searchsorted(edges, x, right=True) - 1, minlength=bins)
        reduce_type, elem = G.DataType_Double, 8  # (8 bytes an element: the same read)
    del ids
    torch.cuda.empty_cache()
    res = {"hist": median_ms(torch, reps, call), "last": hist.last()}
    want = theirs()
    if kind != "float32":
        assert torch.equal(out.to(torch.int64), want.to(torch.int64)), "the counts differ from torch's"
    else:  # (histc counts in float32: its bins differ beside the edges, and a count stops at 2^24)
        assert int(out.sum().item()) == n, "samples were lost"
    res["torch"] = median_ms(torch, reps, theirs)
    del want
    red = G.Reduce(reduce_type, G.ReduceOperator_Sum)
    red_out = torch.empty(4, dtype=torch.int64, device="cuda")
    res["reduce"] = median_ms(torch, reps, lambda: red.run_batch_ptr(x.data_ptr(), red_out.data_ptr(), n, 1, stream))
    res["bytes"] = elem * n
    return res


def run_block(kind, log2n, reps, only):
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    n = 1 << log2n
    # a stream of our own, made current: the events go where the calls go
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for bins in BINS[kind]:
            for data in INPUTS:
                name = "2^%d %s %s, %d bins, %s" % (log2n, kind, "edges" if kind == "uint64" else "even", bins, data)
                if only is not None and not all(part in name for part in only.split(",")):
                    continue
                r = measure(torch, G, side.cuda_stream, kind, n, bins, data, reps)
                side.synchronize()
                gbs = r["bytes"] / (r["hist"] * 1e-3) / 1e9
                print("%-40s %9.4f %7.0f %5.1f%% %6s %6d | %9.4f %9.2f | %9.4f %10.2f" % (
                    name, r["hist"], gbs, 100.0 * gbs / PEAK_GBS, "LDS" if r["last"][0] == 0 else "GLOBAL", r["last"][1], r["reduce"],
                    r["hist"] / r["reduce"], r["torch"], r["torch"] / r["hist"]))
                sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="2^20 samples only")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only (several texts, separated by commas: all of them)")
    ap.add_argument("--timeout", type=int, default=600, help="seconds a block's process may take")
    ap.add_argument("--kinds", default=",".join(KINDS), help="of uint32, float32, uint64: these blocks only")
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

    import glu_hip as G  # (host only: the plan)

    say("# device events, 3 warm-up + %d repetitions, median; ms; GB/s = the bytes of the samples over the call's time; peak = that "
        "over %d GB/s" % (args.reps, PEAK_GBS))
    for kind in KINDS:
        mode = "edges" if kind == "uint64" else "even"
        _, threads, tile, groups_max, _, _ = G.plan_histogram(2 ** 32 - 1, 1, kind, mode)
        say("# %s %s: %d threads a workgroup, %d samples a tile, at most %d workgroups" % (kind, mode, threads, tile, groups_max))
    say(HEADER)
    for log2n in ([20] if args.quick else SIZES):
        for kind in [k for k in KINDS if k in args.kinds.split(",")]:
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
    say("# reduce: glu_reduce_run_batch_ptr (sum, one partition) of the same array; torch: bincount of ready ids (uint32), histc "
        "(float32), searchsorted + bincount (uint64 edges)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
