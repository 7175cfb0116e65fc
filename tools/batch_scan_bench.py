#!/usr/bin/env python3
"""Ladder of the batched scan (glu_scan_run_batch_offsets_ptr): 2^26 elements cut into equal segments of several lengths, the
rows just below and above every class limit, one mixed batch, one row against the same work done as a loop of single scans --
the only way to do it without the batched entry point -- and one long segment beside glu_scan_run_ptr on the same array.

    python tools/batch_scan_bench.py [--baseline-lib PATH] [--reps 20] [--quick] > profiles/batched_scan/ladder.txt

Every row: random uint32 made on the device once (the scan works in place: every repetition scans what the one before left,
which costs the same), device events on the call's stream around the call, 3 warm-up repetitions, median of --reps.  Columns:
  ms        the batched call
  B/elem    bytes moved per element: read + write (8), a second read for segments of the long class (12), plus the offsets
            (4 bytes per segment)
  of peak   bytes moved / ms over 8 TB/s
  path      the class glu_scan_plan_batch gives the row's segments (mixed: segments per class from glu_scan_read_batch)
Rows marked `partitions` also run glu_scan_run_ptr(count, num_partitions) on the same array (its packed-partition kernel for
power-of-two counts up to 1024).  The loop row: 4096 calls of glu_scan_run_ptr, one per segment, on one object.  With
--baseline-lib the loop runs in a child process on THAT library (GLU_HIP_LIB_PATH; the library built from the parent commit), else
on the library under test.  The 2^28 row: the batched call, glu_scan_run_ptr with GLU_HIP_SCAN_CHAINED=0 (reduce-then-scan, 12
B/element like the long class) and glu_scan_run_ptr as it is by default (chained, 8 B/element), same array, same process.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

PEAK_BYTES_PER_MS = 8e12 / 1e3
UINT = 3  # glu::DataType_Uint


def mixed_lengths(rng, scale):
    """Zeros, ones, geometric around 40, uniform up to 3000, workgroup-sized and long segments, shuffled."""
    lens = np.concatenate([np.zeros(3000 * scale, np.int64), np.ones(3000 * scale, np.int64), rng.geometric(1 / 40.0, 20000 * scale),
                           rng.integers(0, 3001, 800 * scale),
                           np.asarray(([8192] * 2 + [16384] * 2 + [16385] * 2 + [100001]) * scale + [1500000], dtype=np.int64)])
    rng.shuffle(lens)
    return lens


def rows(quick):
    lg = 22 if quick else 26
    out = []
    for length in (4, 32, 256, 4096, 65536, 1 << 20):
        out.append({"name": "%7d x %-8d (2^%d)" % (length, (1 << lg) // length, lg), "count": length, "parts": (1 << lg) // length,
                    "partitions": length == 256})
    for length in (33, 128, 129, 512, 513, 1024, 16384, 16385):  # last length of a class / group size beside the first of the next
        out.append({"name": "%7d x %-8d (boundary)" % (length, (1 << lg) // length), "count": length, "parts": (1 << lg) // length})
    out.append({"name": "mixed offsets (about 2^%d)" % lg, "lens": mixed_lengths(np.random.default_rng(1), 1 if quick else 27)})
    out.append({"name": "   4096 x 4096     (2^24)", "count": 4096, "parts": 4096, "loop": True})
    if not quick:
        out.append({"name": "   2^28 x 1", "count": 1 << 28, "parts": 1, "single": True})
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


def measure(row, reps, mode):
    import torch

    # a stream of our own, made current: the events go where the calls go (the handle of torch's default stream is 0, which the
    # library reads as "the library queue")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = measure_on(torch, side.cuda_stream, row, reps, mode)
        side.synchronize()
    return out


def scan_with_env(G, value):
    """A BlellochScan made while GLU_HIP_SCAN_CHAINED is `value` (None: unset): the object reads it when it is created."""
    old = os.environ.pop("GLU_HIP_SCAN_CHAINED", None)
    if value is not None:
        os.environ["GLU_HIP_SCAN_CHAINED"] = value
    try:
        return G.BlellochScan(UINT)
    finally:
        os.environ.pop("GLU_HIP_SCAN_CHAINED", None)
        if old is not None:
            os.environ["GLU_HIP_SCAN_CHAINED"] = old


def measure_on(torch, stream, row, reps, mode):
    import glu_hip as G

    lens = row["lens"] if "lens" in row else np.full(row["parts"], row["count"], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    total, nseg = int(offsets[-1]), lens.size
    data = torch.randint(-(1 << 31), 1 << 31, (total,), dtype=torch.int32, device="cuda")
    scan = G.BlellochScan(UINT)
    res = {}
    if mode == "loop":
        spans = [(int(offsets[s]) * 4, int(lens[s])) for s in range(nseg) if lens[s] > 0]
        base = data.data_ptr()

        def call():
            for byte, n in spans:
                scan.run_ptr(base + byte, n, 1, stream)

        return {"loop_ms": median_ms(torch, reps, call), "calls": len(spans)}
    ot = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    scan.prepare_batch(total, nseg)
    torch.cuda.synchronize()
    res["offsets_ms"] = median_ms(torch, reps, lambda: scan.run_batch_offsets_ptr(data.data_ptr(), total, ot.data_ptr(), nseg, stream))
    torch.cuda.synchronize()
    res["classes"] = scan.read_batch()
    if row.get("partitions"):
        scan.prepare(row["count"], nseg)
        res["partitions_ms"] = median_ms(torch, reps, lambda: scan.run_ptr(data.data_ptr(), row["count"], nseg, stream))
    if row.get("single"):
        for key, value in (("single_rts_ms", "0"), ("single_chained_ms", None)):
            single = scan_with_env(G, value)
            single.prepare(total, 1)
            torch.cuda.synchronize()
            res[key] = median_ms(torch, reps, lambda: single.run_ptr(data.data_ptr(), total, 1, stream))
    res["total"], res["nseg"] = total, nseg
    res["path"] = G.plan_scan_batch(row["count"], 4) if "count" in row else None
    lengths, how_many = np.unique(lens, return_counts=True)
    res["bytes"] = 4.0 * (nseg + 1) + float(sum(int(n) * int(m) * (12 if G.plan_scan_batch(int(n), 4)[0] == 3 else 8)
                                                for n, m in zip(lengths, how_many)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None, help="libglu_hip.so built from the parent commit: the loop runs on it, in a child process")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="2^22 rows only, no 2^28 segment")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only (e.g. '2^28' under a profiler)")
    ap.add_argument("--loop-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    table = [row for row in rows(args.quick) if args.only is None or args.only in row["name"]]
    if args.loop_child:
        import ctypes

        import torch

        torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
        import glu_hip as G

        # the baseline library predates the batched entry points of this tree's binding: bind what it exports (the loop needs run_ptr only)
        exported = ctypes.CDLL(G.LIB_PATH)
        G.SYMBOLS[:] = [s for s in G.SYMBOLS if hasattr(exported, s[0])]
        print(json.dumps([measure(row, args.reps, "loop") for row in table if row.get("loop")]))
        return
    import torch

    import glu_hip as G

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    batch = [measure(row, args.reps, "batch") for row in table]
    torch.cuda.synchronize()
    if args.baseline_lib:
        env = dict(os.environ, GLU_HIP_LIB_PATH=os.path.abspath(args.baseline_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--loop-child", "--reps", str(args.reps)] + (["--quick"] if args.quick else [])
        cmd += ["--only", args.only] if args.only is not None else []
        child = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
        if child.returncode != 0:
            sys.exit("the loop on the baseline library failed:\n" + child.stderr[-2000:])
        loop = json.loads(child.stdout.strip().splitlines()[-1])
        where = "library " + args.baseline_lib
    else:
        loop = [measure(row, args.reps, "loop") for row in table if row.get("loop")]
        where = "the library under test"
    print("# %s" % G.device_info())
    print("# device events, 3 warm-up + %d repetitions, median; the loop ran on %s" % (args.reps, where))
    print("%-34s %10s %7s %8s  %s" % ("row", "ms", "B/elem", "of peak", "path"))
    loops = iter(loop)
    for row, b in zip(table, batch):
        n = b["total"]
        path = "path %d, %d workgroup(s) per segment" % tuple(b["path"]) if b["path"] else "wave %(wave)d block %(block)d long %(long)d" % b["classes"]
        print("%-34s %10.4f %7.2f %7.1f%%  %s" % (row["name"], b["offsets_ms"], b["bytes"] / n, 100.0 * b["bytes"] / b["offsets_ms"] / PEAK_BYTES_PER_MS, path))
        if "partitions_ms" in b:
            print("%-34s %10.4f ms, %.1f%% of peak at 8 B/elem; batched / partitions: %.3f" % (
                "    glu_scan_run_ptr, %d partitions" % b["nseg"], b["partitions_ms"], 100.0 * 8 * n / b["partitions_ms"] / PEAK_BYTES_PER_MS,
                b["offsets_ms"] / b["partitions_ms"]))
        if row.get("loop"):
            l = next(loops)
            print("%-34s %10.3f ms for %d calls of glu_scan_run_ptr: %.1f x the batched call" % (
                "    the loop of single scans", l["loop_ms"], l["calls"], l["loop_ms"] / b["offsets_ms"]))
        if row.get("single"):
            print("%-34s %10.4f ms, %.1f%% of peak at 12 B/elem; batched / single: %.3f" % (
                "    glu_scan_run_ptr, CHAINED=0", b["single_rts_ms"], 100.0 * 12 * n / b["single_rts_ms"] / PEAK_BYTES_PER_MS,
                b["offsets_ms"] / b["single_rts_ms"]))
            print("%-34s %10.4f ms, %.1f%% of peak at 8 B/elem; batched / chained: %.3f" % (
                "    glu_scan_run_ptr, chained", b["single_chained_ms"], 100.0 * 8 * n / b["single_chained_ms"] / PEAK_BYTES_PER_MS,
                b["offsets_ms"] / b["single_chained_ms"]))


if __name__ == "__main__":
    main()
