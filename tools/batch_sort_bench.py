#!/usr/bin/env python3
"""Ladder of the batched radix sort (glu_radix_sort_run_batch_ptr / _batch_offsets_ptr) against the same work done as a loop of
single sorts -- the only way to do it without the batched entry points.

    python tools/batch_sort_bench.py [--baseline-lib PATH] [--reps 20] [--quick] > profiles/batched_sort/ladder.txt

Every row: uint32 keys with uint32 values, fresh random keys copied in before every repetition (outside the timed window), device
events around the call, 3 warm-up repetitions, median of --reps.  Columns:
  ms        the batched call
  Gkeys/s   elements / ms
  B/pair    bytes the path really moves per pair: 16 where a wave or a workgroup sorts the segment inside LDS (one read, one
            write of key and value); 80 where a workgroup streams four counting passes (per pass: keys read for the histogram,
            pair read, pair written); 80 for the four passes of the ordinary sort that equal partitions beyond a tile loop over
  of peak   B/pair x elements / ms over 8 TB/s
  loop ms   the same segments as a loop of glu_radix_sort_run_typed_ptr calls, one per segment of >= 2 elements, on one object.  At most
            4096 calls are timed (the first 4096 such segments) and the time is scaled by elements in all segments / elements in
            the timed ones; `calls` says how many were timed.  With --baseline-lib the loop runs in a child process on THAT
            library (GLU_HIP_LIB_PATH; the library built from the parent commit), else on the library under test.
  ratio     loop ms / ms
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
LOOP_MAX_CALLS = 4096


def mixed_lengths(rng, scale):
    """The mix of tests/test_gpu_batched_sort.py::test_every_class_in_one_call, `scale` times as many segments of every kind."""
    lens = np.concatenate([np.zeros(3000 * scale, np.int64), np.ones(3000 * scale, np.int64), rng.geometric(1 / 40.0, 20000 * scale),
                           rng.integers(0, 3001, 800 * scale),
                           np.asarray(([16384] * 2 + [16385] * 2 + [100000] * 2 + [100001]) * scale + [1500000], dtype=np.int64)])
    rng.shuffle(lens)
    return lens


def rows(quick):
    rng = np.random.default_rng(1)
    out = []
    for lg in ((22,) if quick else (22, 26)):
        for length in (32, 256, 1024, 4096, 16384):
            out.append({"name": "equal %5d x %-7d (2^%d)" % (length, (1 << lg) // length, lg), "count": length,
                        "lens": np.full((1 << lg) // length, length, np.int64)})
    if not quick:  # the row the 16 x condition of the batched sort's issue names
        out.append({"name": "equal  4096 x 4096    (2^24)", "count": 4096, "lens": np.full(4096, 4096, np.int64)})
    for length in (512, 513, 1025, 4097):  # the first / last length of a class beside the ladder's 1024 and 4096 rows
        out.append({"name": "equal %5d x %-7d (class boundary)" % (length, (1 << 22) // length), "count": length,
                    "lens": np.full((1 << 22) // length, length, np.int64)})
    out.append({"name": "mixed offsets (about 2^%d)" % (22 if quick else 26), "count": 0, "lens": mixed_lengths(rng, 1 if quick else 27)})
    if not quick:
        out.append({"name": "equal 2^20 x 64 (looped ordinary sort)", "count": 1 << 20, "lens": np.full(64, 1 << 20, np.int64)})
        out.append({"name": "offsets 2^20 x 64 (a workgroup per segment)", "count": 0, "lens": np.full(64, 1 << 20, np.int64)})
    return out


def bytes_moved(G, row):
    lens = row["lens"]
    lens = lens[lens >= 2]
    if row["count"]:
        per = 16 if G.plan_batch(row["count"])[0] in (1, 2) else 80
        return per * int(lens.sum())
    return 16 * int(lens[lens <= 16384].sum()) + 80 * int(lens[lens > 16384].sum())


def median_ms(torch, reps, fill, call):
    times = []
    for rep in range(reps + 3):
        fill()
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

    # a stream of our own, made current: the events and the copies go where the sorts go (the handle of torch's default stream is
    # 0, which the library reads as "the library queue")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = measure_on(torch, side.cuda_stream, row, reps, mode)
        side.synchronize()
    return out


def measure_on(torch, stream, row, reps, mode):
    import glu_hip as G

    lens = row["lens"]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    total, nseg = int(offsets[-1]), lens.size
    rng = np.random.default_rng(2)
    master_k = torch.from_numpy(rng.integers(0, 2**32, total, dtype=np.uint32).view(np.int32)).cuda()
    master_v = torch.arange(total, dtype=torch.int32, device="cuda")
    kt, vt = torch.empty_like(master_k), torch.empty_like(master_v)
    sorter = G.RadixSort()

    def fill():
        kt.copy_(master_k)
        vt.copy_(master_v)

    if mode == "batch":
        sorter.prepare_batch(total, nseg, 4, True)
        if row["count"]:
            call = lambda: sorter.sort_batch_ptr(kt.data_ptr(), vt.data_ptr(), row["count"], nseg, "uint32", stream)
        else:
            ot = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
            call = lambda: sorter.sort_batch_offsets_ptr(kt.data_ptr(), vt.data_ptr(), total, ot.data_ptr(), nseg, "uint32", stream)
        ms = median_ms(torch, reps, fill, call)
        torch.cuda.synchronize()
        return {"ms": ms, "classes": sorter.read_batch()}
    # the loop of single sorts
    which = np.flatnonzero(lens >= 2)[:LOOP_MAX_CALLS]
    sorter.prepare_internal_buffers(int(lens.max()))
    spans = [(int(offsets[s]) * 4, int(lens[s])) for s in which]
    kp, vp = kt.data_ptr(), vt.data_ptr()

    def call():
        for byte, n in spans:
            sorter.sort_typed_ptr(kp + byte, vp + byte, n, "uint32", stream)

    ms = median_ms(torch, reps, fill, call)
    scale = float(lens[lens >= 2].sum()) / float(lens[which].sum())
    return {"ms": ms * scale, "calls": len(spans), "scale": scale}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None, help="libglu_hip.so built from the parent commit: the loop runs on it, in a child process")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="2^22 rows only")
    ap.add_argument("--loop-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    table = rows(args.quick)
    if args.loop_child:
        import ctypes

        import torch

        torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
        import glu_hip as G

        # the baseline library predates some entry points of this tree's binding: bind what it exports (the loop needs run_typed_ptr only)
        exported = ctypes.CDLL(G.LIB_PATH)
        G.SYMBOLS[:] = [s for s in G.SYMBOLS if hasattr(exported, s[0])]
        print(json.dumps([measure(row, args.reps, "loop") for row in table]))
        return
    import torch

    import glu_hip as G

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    batch = [measure(row, args.reps, "batch") for row in table]
    torch.cuda.synchronize()
    if args.baseline_lib:
        env = dict(os.environ, GLU_HIP_LIB_PATH=os.path.abspath(args.baseline_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--loop-child", "--reps", str(args.reps)] + (["--quick"] if args.quick else [])
        child = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
        if child.returncode != 0:
            sys.exit("the loop on the baseline library failed:\n" + child.stderr[-2000:])
        loop = json.loads(child.stdout.strip().splitlines()[-1])
        where = "library " + args.baseline_lib
    else:
        loop = [measure(row, args.reps, "loop") for row in table]
        where = "the library under test"
    print("# %s" % G.device_info())
    print("# uint32 pairs; device events, 3 warm-up + %d repetitions, median; the loop ran on %s" % (args.reps, where))
    print("%-46s %9s %8s %7s %8s %10s %6s %8s  %s" % ("row", "ms", "Gkeys/s", "B/pair", "of peak", "loop ms", "calls", "ratio", "segments per class"))
    for row, b, l in zip(table, batch, loop):
        n = int(row["lens"][row["lens"] >= 2].sum())
        moved = bytes_moved(G, row)
        print("%-46s %9.4f %8.2f %7.1f %7.1f%% %10.3f %6d %8.1f  %s" % (
            row["name"], b["ms"], n / b["ms"] / 1e6, moved / n, 100.0 * moved / b["ms"] / PEAK_BYTES_PER_MS, l["ms"], l["calls"],
            l["ms"] / b["ms"], "wave %(wave)d block %(block)d long %(long)d" % b["classes"]))


if __name__ == "__main__":
    main()
