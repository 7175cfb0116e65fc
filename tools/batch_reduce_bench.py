#!/usr/bin/env python3
"""Ladder of the batched reduce (glu_reduce_run_batch_ptr / _batch_offsets_ptr): every row through both entry points, one row
against the same work done as a loop of single reduces -- the only way to do it without the batched entry points -- and one long
segment beside glu_reduce_run_ptr on the same array.

    python tools/batch_reduce_bench.py [--baseline-lib PATH] [--reps 20] [--quick] > profiles/batched_reduce/ladder.txt

Every row: random data made on the device once (the batched reduce only reads it), device events on the call's stream around
the call, 3 warm-up repetitions, median of --reps; uint32 Sum unless the row says otherwise.  Columns:
  ms        the batched call with equal partitions (`-` for rows that have no such form) and with device offsets
  B/elem    bytes read per element: the element itself, plus the offsets (4 bytes per segment) in the offsets form
  of peak   bytes read / ms over 8 TB/s
  path      the class glu_reduce_plan_batch gives the row's segments (mixed: segments per class from glu_reduce_read_batch)
The loop row: 4096 calls of glu_reduce_run_ptr, one per segment, on one object.  With --baseline-lib the loop runs in a child
process on THAT library (GLU_HIP_LIB_PATH; the library built from the parent commit), else on the library under test.
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
UINT, FLOAT, DVEC4 = 3, 0, 7  # glu::DataType values
SUM, MIN = 0, 2
ELEM_BYTES = {UINT: 4, FLOAT: 4, DVEC4: 32}


def mixed_lengths(rng, scale):
    """Zeros, ones, geometric around 40, uniform up to 3000, workgroup-sized and long segments, shuffled."""
    lens = np.concatenate([np.zeros(3000 * scale, np.int64), np.ones(3000 * scale, np.int64), rng.geometric(1 / 40.0, 20000 * scale),
                           rng.integers(0, 3001, 800 * scale),
                           np.asarray(([16384] * 2 + [65536] * 2 + [65537] * 2 + [100001]) * scale + [1500000], dtype=np.int64)])
    rng.shuffle(lens)
    return lens


def rows(quick):
    lg = 22 if quick else 26
    out = []
    for length in (4, 32, 256, 4096, 65536, 1 << 20):
        out.append({"name": "%7d x %-8d (2^%d)" % (length, (1 << lg) // length, lg), "count": length, "parts": (1 << lg) // length})
    for length in (16, 17, 64, 65, 1024, 1025, 65537):  # last length of a class / group size beside the first of the next
        out.append({"name": "%7d x %-8d (boundary)" % (length, (1 << lg) // length), "count": length, "parts": (1 << lg) // length})
    out.append({"name": "mixed offsets (about 2^%d)" % lg, "lens": mixed_lengths(np.random.default_rng(1), 1 if quick else 27)})
    out.append({"name": "   4096 x 4096     dvec4 Sum", "count": 4096, "parts": 4096, "dt": DVEC4})
    out.append({"name": "   4096 x 4096     float Min", "count": 4096, "parts": 4096, "dt": FLOAT, "op": MIN})
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


def make_data(torch, total, dt):
    if dt == DVEC4:
        return torch.randn(total * 4, dtype=torch.float64, device="cuda")
    if dt == FLOAT:
        return torch.randn(total, dtype=torch.float32, device="cuda")
    return torch.randint(-(1 << 31), 1 << 31, (total,), dtype=torch.int32, device="cuda")


def measure(row, reps, mode):
    import torch

    # a stream of our own, made current: the events go where the calls go (the handle of torch's default stream is 0, which the
    # library reads as "the library queue")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = measure_on(torch, side.cuda_stream, row, reps, mode)
        side.synchronize()
    return out


def measure_on(torch, stream, row, reps, mode):
    import glu_hip as G

    dt, op = row.get("dt", UINT), row.get("op", SUM)
    es = ELEM_BYTES[dt]
    lens = row["lens"] if "lens" in row else np.full(row["parts"], row["count"], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    total, nseg = int(offsets[-1]), lens.size
    data = make_data(torch, total, dt)
    red = G.Reduce(dt, op)
    res = {}
    if mode == "loop":
        spans = [(int(offsets[s]) * es, int(lens[s])) for s in range(nseg) if lens[s] > 0]
        base = data.data_ptr()

        def call():
            for byte, n in spans:
                red.run_ptr(base + byte, n, stream)

        return {"loop_ms": median_ms(torch, reps, call), "calls": len(spans)}
    out = torch.empty(nseg * es // 4, dtype=torch.int32, device="cuda")
    ot = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    red.prepare_batch(total, nseg)
    torch.cuda.synchronize()
    if "count" in row:
        res["equal_ms"] = median_ms(torch, reps, lambda: red.run_batch_ptr(data.data_ptr(), out.data_ptr(), row["count"], nseg, stream))
    res["offsets_ms"] = median_ms(torch, reps, lambda: red.run_batch_offsets_ptr(data.data_ptr(), out.data_ptr(), total, ot.data_ptr(), nseg, stream))
    torch.cuda.synchronize()
    res["classes"] = red.read_batch()
    if row.get("single"):  # last: the single reduce writes its result into the array
        res["single_ms"] = median_ms(torch, reps, lambda: red.run_ptr(data.data_ptr(), total, stream))
    res["total"], res["nseg"], res["es"] = total, nseg, es
    res["path"] = G.plan_reduce_batch(row["count"], es) if "count" in row else None
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
    print("%-34s %10s %7s %8s %11s %7s %8s  %s" % ("row", "equal ms", "B/elem", "of peak", "offsets ms", "B/elem", "of peak", "path"))
    loops = iter(loop)
    for row, b in zip(table, batch):
        n, es = b["total"], b["es"]
        ob = es + 4.0 * (b["nseg"] + 1) / n
        eq = "%10.4f %7.2f %7.1f%%" % (b["equal_ms"], es, 100.0 * es * n / b["equal_ms"] / PEAK_BYTES_PER_MS) if "equal_ms" in b else "%10s %7s %8s" % ("-", "-", "-")
        path = "path %d, %d workgroup(s) per segment" % tuple(b["path"]) if b["path"] else "wave %(wave)d block %(block)d long %(long)d" % b["classes"]
        print("%-34s %s %11.4f %7.2f %7.1f%%  %s" % (row["name"], eq, b["offsets_ms"], ob, 100.0 * ob * n / b["offsets_ms"] / PEAK_BYTES_PER_MS, path))
        if row.get("loop"):
            l = next(loops)
            print("%-34s %10.3f ms for %d calls of glu_reduce_run_ptr: %.1f x the equal-partition call, %.1f x the offsets call" % (
                "    the loop of single reduces", l["loop_ms"], l["calls"], l["loop_ms"] / b["equal_ms"], l["loop_ms"] / b["offsets_ms"]))
        if row.get("single"):
            print("%-34s %10.4f ms, %.1f%% of peak; batched / single: equal partitions %.3f, offsets %.3f" % (
                "    glu_reduce_run_ptr, same array", b["single_ms"], 100.0 * es * n / b["single_ms"] / PEAK_BYTES_PER_MS,
                b["equal_ms"] / b["single_ms"], b["offsets_ms"] / b["single_ms"]))


if __name__ == "__main__":
    main()
