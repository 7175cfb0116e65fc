#!/usr/bin/env python3
"""Ladder of the batched histogram (glu_histogram_run_batch_even_ptr / _batch_offsets_even_ptr / _batch_offsets_edges_ptr) against
the ways round it and against the floor of one read.

    python tools/histogram_batch_bench.py [--reps 10] [--quick] [--only TEXT] [--timeout 600] [--out profiles/histogram_batch/ladder.txt]

Rows, 2^28 uint32 samples unless the row says otherwise (--quick: 2^22), uniform ids over the bins unless it says zipf:
  equal partitions   2^20 x 256 (64 bins: wave class), 65536 x 4096 (256 bins), 4096 x 65536 (256 and 8192 bins), 64 x 2^22 (256 and
                     8192 bins: long class), 1 x 2^28 (256 bins)
  ragged             the 2^16 groups key runs finds in 2^26 sorted keys (256 bins over the values beside them), device offsets
  types              float32 even bins and uint64 over 256 edges, 4096 x 65536 (block class)
  skew               4096 x 65536, 256 bins, zipf ids
Every row runs in a child process of its own under its own timeout, and the ladder stops at the first row that fails.  Device events
on the call's stream around the call, 3 warm-up repetitions, median of --reps.  Columns, ms, measured in the same process on the same
data:
  batch    the batched call after glu_histogram_prepare_batch, all its kernels; segments per class as read_batch() states them
  single   ONE glu_histogram_run_even_ptr / _edges_ptr over the whole array into one table: the same read, the floor
  reduce   the batched Reduce (sum) over the same segments: one read with segments
  loop     glu_histogram_run_*_ptr once per segment, where there are at most 4096 segments
  torch    torch.bincount of ready combined ids segment * bins + bin (int64, made outside the timed region), minlength = S * bins
The counts of every row are compared with torch's."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

# name: (kind, log2 of the samples, segments (None: key runs), bins, data)
ROWS = [
    ("2^20 x 256, 64 bins", "uint32", 28, 1 << 20, 64, "uniform"),
    ("65536 x 4096, 256 bins", "uint32", 28, 65536, 256, "uniform"),
    ("4096 x 65536, 256 bins", "uint32", 28, 4096, 256, "uniform"),
    ("4096 x 65536, 8192 bins", "uint32", 28, 4096, 8192, "uniform"),
    ("64 x 2^22, 256 bins", "uint32", 28, 64, 256, "uniform"),
    ("64 x 2^22, 8192 bins", "uint32", 28, 64, 8192, "uniform"),
    ("1 x 2^28, 256 bins", "uint32", 28, 1, 256, "uniform"),
    ("key runs: 2^16 groups in 2^26, 256 bins", "uint32", 26, None, 256, "uniform"),
    ("float32 even, 4096 x 65536, 256 bins", "float32", 28, 4096, 256, "uniform"),
    ("uint64 edges, 4096 x 65536, 256 bins", "uint64", 28, 4096, 256, "uniform"),
    ("zipf ids, 4096 x 65536, 256 bins", "uint32", 28, 4096, 256, "zipf"),
    ("zipf ids, 64 x 2^22, 8192 bins", "uint32", 28, 64, 8192, "zipf"),
]
# --constants: the rows that hold a class limit against half and twice its value (a tuning build of glu_histogram.hip with
# -DGLU_HIST_BATCH_WAVE_BYTES / _BLOCK_BYTES / _CHUNK_BYTES, loaded through GLU_HIP_LIB_PATH); only the batched call is timed
CONSTANT_ROWS = [
    ("2^18 x 1024, 64 bins", "uint32", 28, 1 << 18, 64, "uniform"),     # at wave_limit: the wave class, or the block class at half
    ("2^17 x 2048, 64 bins", "uint32", 28, 1 << 17, 64, "uniform"),     # at twice wave_limit
    ("4096 x 65536, 256 bins", "uint32", 28, 4096, 256, "uniform"),     # at block_limit: the block class, or the long class at half
    ("2048 x 131072, 256 bins", "uint32", 28, 2048, 256, "uniform"),    # at twice block_limit
    ("64 x 2^22, 256 bins", "uint32", 28, 64, 256, "uniform"),          # long: the chunk
    ("1 x 2^28, 256 bins", "uint32", 28, 1, 256, "uniform"),
    ("64 x 2^22, 8192 bins", "uint32", 28, 64, 8192, "uniform"),
]
HEADER ="%-42s %9s %7s %-18s | %9s %7s | %9s %7s | %9s %7s | %9s %7s" % (
    "row", "batch", "GB/s", "wave/block/long", "single", "b/single", "reduce", "b/reduce", "loop", "loop/b", "torch", "torch/b")
LOOP_MOST = 4096


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
    u = torch.rand(n, generator=gen, device="cuda", dtype=torch.float64)  # P(id = k) ~ log((k + 2) / (k + 1)): Zipf(1.0) over the bins
    return (torch.pow(torch.tensor(float(bins), device="cuda", dtype=torch.float64), u).floor().to(torch.int64) - 1).clamp_(0, bins - 1)


def measure(torch, G, stream, kind, n, segments, bins, data, reps, batch_only=False):
    gen = torch.Generator(device="cuda").manual_seed(n % 1000 + bins % 1000 + len(data))
    ids = make_ids(torch, gen, n, bins, data)
    hist, single = G.Histogram(), G.Histogram()
    if segments is None:  # the groups key runs finds in sorted keys: nothing about them is read on the host in between
        segments = 1 << 16
        keys = torch.sort(torch.randint(0, segments, (n,), generator=gen, device="cuda", dtype=torch.int32))[0]
        offsets = torch.zeros(segments + 1, dtype=torch.int32, device="cuda")
        runs = torch.zeros(1, dtype=torch.int32, device="cuda")
        G.KeyRuns().run_ptr(keys.data_ptr(), n, offsets.data_ptr(), segments, runs.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        seg_of = torch.searchsorted(offsets[1:].to(torch.int64), torch.arange(n, device="cuda"), right=True)
        del keys
        count = None
    else:
        count = n // segments
        offsets = (torch.arange(segments + 1, device="cuda", dtype=torch.int64) * count).to(torch.int32)
        seg_of = torch.arange(n, device="cuda", dtype=torch.int64) // count
    combined = seg_of * bins + ids
    del seg_of
    out = torch.empty(segments * bins, dtype=torch.int32, device="cuda")
    one = torch.empty(bins, dtype=torch.int32, device="cuda")
    hist.prepare_batch(n, segments, bins)
    single.prepare(n, bins)
    if kind == "uint32":
        x = (ids * 16 + torch.randint(0, 16, (n,), generator=gen, device="cuda", dtype=torch.int64)).to(torch.int32)  # (below 2^31)
        rule, reduce_type, elem = (0, 16 * bins), G.DataType_Uint, 4
    elif kind == "float32":
        x = ((ids.to(torch.float64) + torch.rand(n, generator=gen, device="cuda", dtype=torch.float64)) / bins).to(torch.float32)
        x = x.clamp_(0.0, float(np.nextafter(np.float32(1), np.float32(0))))
        ids = (x.to(torch.float64) * bins).to(torch.int64).clamp_(max=bins - 1)  # (the bin of the ROUNDED sample, by the contract)
        combined = (combined // bins) * bins + ids
        rule, reduce_type, elem = (0.0, 1.0), G.DataType_Float, 4
    else:
        step = (1 << 62) // bins
        x = ids * step + torch.randint(0, step, (n,), generator=gen, device="cuda", dtype=torch.int64)
        edges = torch.arange(bins + 1, device="cuda", dtype=torch.int64) * step
        rule, reduce_type, elem = None, G.DataType_Double, 8  # (8 bytes an element: the same read)
    del ids
    torch.cuda.empty_cache()
    xp, op, fp = x.data_ptr(), out.data_ptr(), offsets.data_ptr()
    if rule is not None:
        if count is not None:
            call = lambda: hist.run_batch_even_ptr(xp, count, segments, rule[0], rule[1], bins, op, kind, False, stream)
        else:
            call = lambda: hist.run_batch_offsets_even_ptr(xp, n, fp, segments, rule[0], rule[1], bins, op, kind, False, stream)
        whole = lambda: single.run_even_ptr(xp, n, rule[0], rule[1], bins, one.data_ptr(), kind, False, stream)
        part = lambda s, b, m: single.run_even_ptr(xp + elem * b, m, rule[0], rule[1], bins, op + 4 * bins * s, kind, False, stream)
    else:
        call = lambda: hist.run_batch_offsets_edges_ptr(xp, n, fp, segments, edges.data_ptr(), bins, op, kind, False, stream)
        whole = lambda: single.run_edges_ptr(xp, n, edges.data_ptr(), bins, one.data_ptr(), kind, False, stream)
        part = lambda s, b, m: single.run_edges_ptr(xp + elem * b, m, edges.data_ptr(), bins, op + 4 * bins * s, kind, False, stream)
    res = {"batch": median_ms(torch, reps, call), "classes": hist.read_batch(), "last": hist.last(), "bytes": elem * n, "segments": segments}
    theirs = lambda: torch.bincount(combined, minlength=segments * bins)
    want = theirs()
    assert torch.equal(out.to(torch.int64), want), "the counts differ from torch's"
    del want
    if batch_only:
        return res
    res["torch"] = median_ms(torch, reps, theirs)
    del combined
    torch.cuda.empty_cache()
    res["single"] = median_ms(torch, reps, whole)
    red = G.Reduce(reduce_type, G.ReduceOperator_Sum)
    red_out = torch.empty(segments + 4, dtype=torch.int64, device="cuda")
    red.prepare_batch(n, segments)
    res["reduce"] = median_ms(torch, reps, lambda: red.run_batch_offsets_ptr(xp, red_out.data_ptr(), n, fp, segments, stream))
    res["loop"] = None
    if segments <= LOOP_MOST:
        host = offsets.cpu().numpy().astype(np.int64)

        def loop():
            for s in range(segments):
                part(s, int(host[s]), int(host[s + 1] - host[s]))

        res["loop"] = median_ms(torch, reps, loop)
    return res


def run_row(index, quick, reps, constants):
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    name, kind, log2n, segments, bins, data = (CONSTANT_ROWS if constants else ROWS)[index]
    n = 1 << (log2n - 6 if quick else log2n)
    if quick and segments is not None:
        segments = max(1, segments >> 6)
    side = torch.cuda.Stream()  # a stream of our own, made current: the events go where the calls go
    with torch.cuda.stream(side):
        r = measure(torch, G, side.cuda_stream, kind, n, segments, bins, data, reps, batch_only=constants)
        side.synchronize()
    gbs = r["bytes"] / (r["batch"] * 1e-3) / 1e9
    c = r["classes"]
    if constants:
        print("%-42s %9.4f %7.0f %-18s" % (name, r["batch"], gbs, "%d/%d/%d" % (c["wave"], c["block"], c["long"])))
        return
    loop = ("%9.3f %7.1f" % (r["loop"], r["loop"] / r["batch"])) if r["loop"] is not None else "%9s %7s" % ("-", "-")
    print("%-42s %9.4f %7.0f %-18s | %9.4f %7.2f | %9.4f %7.2f | %s | %9.4f %7.2f" % (
        name, r["batch"], gbs, "%d/%d/%d" % (c["wave"], c["block"], c["long"]), r["single"], r["batch"] / r["single"], r["reduce"],
        r["batch"] / r["reduce"], loop, r["torch"], r["torch"] / r["batch"]))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="a 64th of the samples and of the segments")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only")
    ap.add_argument("--timeout", type=int, default=600, help="seconds a row's process may take")
    ap.add_argument("--out", default=None, help="write the ladder to this file as well as to stdout")
    ap.add_argument("--row", type=int, default=None, help="(internal) the row measured in this process")
    ap.add_argument("--constants", action="store_true", help="the rows around the class limits, the batched call only")
    args = ap.parse_args()
    if args.row is not None:
        run_row(args.row, args.quick, args.reps, args.constants)
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

    say("# device events, 3 warm-up + %d repetitions, median; ms; GB/s = the bytes of the samples over the batched call's time%s"
        % (args.reps, "; --quick: a 64th of every row" if args.quick else ""))
    for kind, mode in (("uint32", "even"), ("uint64", "edges")):
        for bins in (256, 8192):
            _, _, (wave_limit, block_limit), chunk, _ = G.plan_histogram_batch(1, bins, kind, mode)
            say("# %s %s, %d bins: wave_limit %d, block_limit %d, chunk %d samples" % (kind, mode, bins, wave_limit, block_limit, chunk))
    say("# library: %s" % os.path.relpath(G.LIB_PATH, ROOT))
    say(HEADER[:HEADER.index(" |")] if args.constants else HEADER)
    for index, row in enumerate(CONSTANT_ROWS if args.constants else ROWS):
        if args.only is not None and args.only not in row[0]:
            continue
        # a fresh child per row, under its own time limit; a row that fails, dies or runs out of time ends the ladder
        cmd = [sys.executable, os.path.abspath(__file__), "--row", str(index), "--reps", str(args.reps)] + (["--quick"] if args.quick else []) \
            + (["--constants"] if args.constants else [])
        try:
            p = subprocess.run(cmd, timeout=args.timeout, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            say("# %s: no result within %d s; the ladder stops here" % (row[0], args.timeout))
            return 124
        for line in p.stdout.splitlines():
            say(line)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            say("# %s: exit status %d; the ladder stops here" % (row[0], p.returncode))
            return p.returncode if p.returncode > 0 else 1
    say("# single: one glu_histogram_run_*_ptr over the whole array; reduce: glu_reduce_run_batch_offsets_ptr (sum) over the same "
        "segments; loop: a single call per segment (at most %d segments); torch: bincount of ready combined ids" % LOOP_MOST)
    return 0


if __name__ == "__main__":
    sys.exit(main())
