#!/usr/bin/env python3
"""Ladder of the batched scan with an operator and a kind (glu_scan_run_batch_offsets_op_ptr), in three parts.

    python tools/scan_ops_bench.py --baseline-lib PATH [--reps 20] [--quick] > profiles/batched_scan/ops_ladder.txt

Shapes: 2^26 elements as equal segments of 4, 32, 256, 4096, 65536 and 2^20 elements, 4096 x 4096, and one segment of 2^28.
Every figure: data made on the device once (calls in place scan what the one before left, which costs the same; Mul scans
factors of +-1 so that this holds for it too), device events on the call's stream around the call, 3 warm-up repetitions, median
of --reps.

1. The old call, glu_scan_run_batch_offsets_ptr on uint32, in three child processes one after the other: the library built from
   the parent commit (--baseline-lib), the library under test, the parent's library again.  The spread between the parent's two
   runs is the margin a row of the library under test has around them.
2. The new forms beside the exclusive Sum in place of the same process: inclusive Sum, inclusive Max and exclusive Mul on uint32
   and float32, in place and out of place, as ratios.  They move the same bytes.
3. Beside torch (recorded, not gated): torch.cumsum / cummax / cumprod on one segment of 2^28 and along the rows of 4096 x 4096,
   and the one-segment form (offsets == NULL, 12 B/element) beside the chained glu_scan_run_ptr (8 B/element) on the same array.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

FLOAT, UINT = 0, 3  # glu::DataType_Float, DataType_Uint
FORMS = [("incl sum", "sum", True), ("incl max", "max", True), ("excl mul", "mul", False)]


def shapes(quick):
    lg = 22 if quick else 26
    out = [("%7d x %-8d" % (n, (1 << lg) // n), n, (1 << lg) // n) for n in (4, 32, 256, 4096, 65536, 1 << 20)]
    out.append(("   4096 x 4096    ", 4096, 4096))
    if not quick:
        out.append(("   2^28 x 1       ", 1 << 28, 1))
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


def make(torch, dt, total, op="sum"):
    """Random words / floats in [0.999, 1.001]; for Mul +1 and -1 at random (as words: 1 and 0xFFFFFFFF), which stay +-1 however
    often a call in place scans its own results (random factors collapse to 0, inf and NaN within a few repetitions)."""
    if op == "mul":
        signs = torch.randint(0, 2, (total,), dtype=torch.int32, device="cuda").mul_(2).sub_(1)
        return signs if dt == UINT else signs.to(torch.float32)
    if dt == UINT:
        return torch.randint(-(1 << 31), 1 << 31, (total,), dtype=torch.int32, device="cuda")
    return torch.empty(total, dtype=torch.float32, device="cuda").uniform_(0.999, 1.001)


def offsets_of(torch, count, parts):
    return torch.arange(parts + 1, dtype=torch.int64, device="cuda").mul_(count).to(torch.int32)  # (wraps to the uint32 bits)


def old_call(torch, G, stream, reps, quick):
    """Part 1, in whatever library this process loaded."""
    out = []
    for name, count, parts in shapes(quick):
        total = count * parts
        data, ot = make(torch, UINT, total), offsets_of(torch, count, parts)
        scan = G.BlellochScan(UINT)
        scan.prepare_batch(total, parts)
        torch.cuda.synchronize()
        out.append(median_ms(torch, reps, lambda: scan.run_batch_offsets_ptr(data.data_ptr(), total, ot.data_ptr(), parts, stream)))
        del data, ot, scan
    return out


def new_forms(torch, G, stream, reps, quick):
    """Part 2: {shape: {dtype: [exclusive sum in place, then in place / out of place for every form]}}."""
    out = []
    for name, count, parts in shapes(quick):
        total = count * parts
        ot = offsets_of(torch, count, parts)
        row = {}
        for dt in (UINT, FLOAT):
            data, apart = make(torch, dt, total), make(torch, dt, total)
            scan = G.BlellochScan(dt)
            scan.prepare_batch(total, parts)
            torch.cuda.synchronize()
            ms = [median_ms(torch, reps, lambda: scan.run_batch_offsets_ptr(data.data_ptr(), total, ot.data_ptr(), parts, stream))]
            for _, op, inclusive in FORMS:
                if op == "mul":
                    data = make(torch, dt, total, op)
                for out_ptr in (None, apart.data_ptr()):
                    ms.append(median_ms(torch, reps, lambda: scan.run_batch_offsets_ptr(data.data_ptr(), total, ot.data_ptr(), parts, stream,
                                                                                        out_ptr=out_ptr, op=op, inclusive=inclusive)))
            row[dt] = ms
            del data, apart, scan
        out.append(row)
    return out


def beside_torch(torch, G, stream, reps):
    """Part 3."""
    lines = []
    n = 1 << 28
    for label, dt, shape, dim in (("2^28 x 1", UINT, (n,), 0), ("2^28 x 1", FLOAT, (n,), 0), ("4096 x 4096 rows", UINT, (4096, 4096), 1),
                                  ("4096 x 4096 rows", FLOAT, (4096, 4096), 1)):
        total = int(np.prod(shape))
        data, apart = make(torch, dt, total), make(torch, dt, total)
        view = data.view(shape)
        parts = 1 if len(shape) == 1 else shape[0]
        ot = offsets_of(torch, total // parts, parts)
        scan = G.BlellochScan(dt)
        scan.prepare_batch(total, parts)
        kind = "uint32 " if dt == UINT else "float32"
        for what, op, fn in (("cumsum", "sum", lambda: torch.cumsum(view, dim, dtype=view.dtype)), ("cummax", "max", lambda: torch.cummax(view, dim)),
                             ("cumprod", "mul", lambda: torch.cumprod(view, dim, dtype=view.dtype))):
            t_ms = median_ms(torch, reps, fn)
            g_ms = median_ms(torch, reps, lambda: scan.run_batch_offsets_ptr(data.data_ptr(), total, ot.data_ptr(), parts, stream, out_ptr=apart.data_ptr(),
                                                                             op=op, inclusive=True))
            lines.append("%-18s %s torch.%-8s %9.4f ms   this library, inclusive, out of place %9.4f ms   library / torch %.3f" % (
                label, kind, what, t_ms, g_ms, g_ms / t_ms))
        if len(shape) == 1 and dt == UINT:
            w_ms = median_ms(torch, reps, lambda: scan.run_whole_ptr(data.data_ptr(), total, stream))
            single = G.BlellochScan(dt)
            single.prepare(total, 1)
            torch.cuda.synchronize()
            c_ms = median_ms(torch, reps, lambda: single.run_ptr(data.data_ptr(), total, 1, stream))
            lines.append("%-18s %s one-segment form (offsets NULL, exclusive sum in place, 12 B/elem) %9.4f ms   glu_scan_run_ptr chained (8 B/elem) "
                         "%9.4f ms   ratio %.3f" % (label, kind, w_ms, c_ms, w_ms / c_ms))
        del data, apart, view, scan
    return lines


def on_side_stream(torch, fn):
    # a stream of our own, made current: the events go where the calls go
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = fn(side.cuda_stream)
        side.synchronize()
    return out


def child(args):
    import ctypes

    import torch

    torch.cuda.init()
    import glu_hip as G

    exported = ctypes.CDLL(G.LIB_PATH)  # the parent's library lacks the newest symbol: bind what it exports
    G.SYMBOLS[:] = [s for s in G.SYMBOLS if hasattr(exported, s[0])]
    print(json.dumps(on_side_stream(torch, lambda s: old_call(torch, G, s, args.reps, args.quick))))


def run_child(args, lib):
    env = dict(os.environ)
    if lib:
        env["GLU_HIP_LIB_PATH"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--old-call-child", "--reps", str(args.reps)] + (["--quick"] if args.quick else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.exit("the old call on %s failed:\n%s" % (lib or "the library under test", p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=False, help="libglu_hip.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="2^22 rows only, no 2^28 segment, no torch")
    ap.add_argument("--old-call-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.old_call_child:
        return child(args)
    names = [s[0] for s in shapes(args.quick)]
    if args.baseline_lib:
        first, new, second = run_child(args, args.baseline_lib), run_child(args, None), run_child(args, args.baseline_lib)
    import torch

    import glu_hip as G

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    print("# %s" % G.device_info())
    print("# device events, 3 warm-up + %d repetitions, median, milliseconds" % args.reps)
    if args.baseline_lib:
        print("\n# 1. glu_scan_run_batch_offsets_ptr, uint32: parent's library, library under test, parent's library again (three processes)")
        print("%-20s %10s %10s %10s %9s %9s  %s" % ("shape", "parent", "new", "parent", "spread", "new/best", "verdict"))
        for name, a, n, b in zip(names, first, new, second):
            spread = abs(a - b)
            inside = n <= max(a, b) + spread
            print("%-20s %10.4f %10.4f %10.4f %8.2f%% %9.3f  %s" % (name, a, n, b, 100 * spread / min(a, b), n / min(a, b),
                                                                  "inside the margin" if inside else "OUTSIDE the margin"))
    forms = on_side_stream(torch, lambda s: new_forms(torch, G, s, args.reps, args.quick))
    print("\n# 2. the new forms over the exclusive Sum in place of the same process (ms), as ratios: in place / out of place")
    print("%-20s %-8s %10s  %s" % ("shape", "type", "excl sum", "   ".join("%-13s" % f[0] for f in FORMS)))
    for name, row in zip(names, forms):
        for dt in (UINT, FLOAT):
            ms = row[dt]
            ratios = ["%5.3f / %5.3f" % (ms[1 + 2 * i] / ms[0], ms[2 + 2 * i] / ms[0]) for i in range(len(FORMS))]
            print("%-20s %-8s %10.4f  %s" % (name, "uint32" if dt == UINT else "float32", ms[0], "   ".join(ratios)))
    if not args.quick:
        print("\n# 3. beside torch (cummax also writes int64 indices: 12 more bytes per element), and the one-segment form beside the chained scan")
        for line in on_side_stream(torch, lambda s: beside_torch(torch, G, s, args.reps)):
            print(line)


if __name__ == "__main__":
    main()
