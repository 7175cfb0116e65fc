#!/usr/bin/env python3
"""The ladder of batched top-k (glu_top_k_run_batch_ptr / _batch_offsets_ptr): device events, 3 warm-ups, the median of 10, the
candidates alternating in one process on the same inputs.  Per row (segments x length, k), sorted and unsorted, the k smallest:

  batch   the batched call
  (a)     what a caller did before: the batched sort of a copy with local iota values plus the gather of the heads (the copy is
          outside the timed region)
  (b)     the loop of glu_top_k_run_ptr, one call per row (rows beyond --loop-max segments: not run, it takes minutes)
  (c)     torch.topk along the dimension
  (d)     the floor: one Reduce pass over the array

Writes the table to --out (default profiles/top_k_batch/ladder.txt)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

ROWS = [(1 << 20, 64, 8), (1 << 16, 1024, 32), (4096, 4096, 64), (1024, 32768, 50), (256, 131072, 50), (64, 1 << 20, 1024), (8, 1 << 24, 1024)]
FLOAT_ONLY = {(1024, 32768, 50), (256, 131072, 50)}
WARMUPS, REPEATS = 3, 10


def main():
    import torch

    import glu_hip as G

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_k_batch", "ladder.txt"))
    ap.add_argument("--loop-max", type=int, default=4096, help="the loop of single calls is run for rows of at most this many segments")
    ap.add_argument("--rows", default="", help="comma-separated indices into the rows (default: all)")
    ap.add_argument("--loop-crossover", action="store_true", help="only: the long kernel against the loop of single calls, rows of 2^20 .. 2^24")
    args = ap.parse_args()
    side = torch.cuda.Stream()  # (the library takes a NULL stream for its own queue: the events and the work share this one)
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    tdt = {"uint32": torch.int32, "float32": torch.float32, "uint64": torch.int64}
    lines = ["# %s" % G.device_info(), "# milliseconds, median of %d after %d warm-ups; k smallest; n/a: not run" % (REPEATS, WARMUPS),
             "%-10s %-22s %6s %-8s %9s %9s %9s %9s %9s  %s" % ("type", "segments x length", "k", "order", "batch", "(a) sort", "(b) loop", "(c) torch",
                                                                "(d) floor", "path")]

    def timed(fn, before=None):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def measure(candidates):
        """{name: (fn, before)} -> {name: median ms}, alternating the candidates"""
        times = {name: [] for name in candidates}
        for it in range(WARMUPS + REPEATS):
            for name, (fn, before) in candidates.items():
                t = timed(fn, before)
                if it >= WARMUPS:
                    times[name].append(t)
        return {name: statistics.median(v) for name, v in times.items()}

    def fmt(v):
        return "%9.3f" % v if v is not None else "%9s" % "n/a"

    if args.loop_crossover:
        # the long kernel (BATCH_LOOP_MIN out of reach) against the loop of single calls (BATCH_LOOP_MIN = 1) on the same rows
        forced = {"long": G.TopK({"BATCH_LOOP_MIN": (1 << 32) - 1}), "loop": G.TopK({"BATCH_LOOP_MIN": 1})}
        lines[2] = "%-10s %-22s %6s %-8s %9s %9s" % ("type", "segments x length", "k", "order", "long", "loop")
        for nseg in (8, 64, 512):
            for log2 in (20, 21, 22, 23, 24):
                length, k = 1 << log2, 1024
                if nseg * length >= 1 << 31:
                    continue
                keys = torch.randint(0, 1 << 31, (nseg * length,), generator=torch.Generator(device="cuda").manual_seed(13), device="cuda",
                                     dtype=torch.int32)
                ok, oi = torch.empty(nseg * k, dtype=torch.int32, device="cuda"), torch.empty(nseg * k, dtype=torch.int32, device="cuda")
                for t in forced.values():
                    t.prepare_batch(nseg * length, nseg, k)
                t = measure({name: ((lambda t=t: t.run_batch_ptr(keys.data_ptr(), length, nseg, k, ok.data_ptr(), oi.data_ptr(), stream=stream)), None)
                             for name, t in forced.items()})
                lines.append("%-10s %-22s %6d %-8s %s %s" % ("uint32", "%d x 2^%d" % (nseg, log2), k, "sorted", fmt(t["long"]), fmt(t["loop"])))
                print(lines[-1], flush=True)
                del keys
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    picked = [int(i) for i in args.rows.split(",")] if args.rows else range(len(ROWS))
    configs = [(dtype, ROWS[i]) for dtype in ("uint32", "float32") for i in picked if dtype == "float32" or ROWS[i] not in FLOAT_ONLY]
    configs.append(("uint64", ROWS[2]))
    top, single, sorter, red = G.TopK(), G.TopK(), G.RadixSort(), G.Reduce(G.DataType_Uint, G.ReduceOperator_Max)
    gen = torch.Generator(device="cuda").manual_seed(11)
    for dtype, (nseg, length, k) in configs:
        total, kb = nseg * length, 8 if dtype == "uint64" else 4
        if dtype == "float32":
            keys = torch.randn(total, generator=gen, device="cuda", dtype=torch.float32)
        else:
            keys = torch.randint(0, 1 << 31 if kb == 4 else 1 << 62, (total,), generator=gen, device="cuda", dtype=tdt[dtype])
        work = torch.empty_like(keys)
        iota = (torch.arange(total, device="cuda", dtype=torch.int32) % length).contiguous()
        vals = torch.empty_like(iota)
        ok = torch.empty(nseg * k, dtype=tdt[dtype], device="cuda")
        oi = torch.empty(nseg * k, dtype=torch.int32, device="cuda")
        top.prepare_batch(total, nseg, k, dtype)
        sorter.prepare_batch(total, nseg, kb, True)
        path = G.plan_top_k_batch(length, nseg, k, dtype)["path"]
        for sorted_ in (True, False):
            def batch():
                top.run_batch_ptr(keys.data_ptr(), length, nseg, k, ok.data_ptr(), oi.data_ptr(), key_type=dtype, sorted=sorted_, stream=stream)

            def copy():
                work.copy_(keys)
                vals.copy_(iota)

            def sort_heads():
                sorter.sort_batch_ptr(work.data_ptr(), vals.data_ptr(), length, nseg, dtype, stream)
                ok.view(nseg, k).copy_(work.view(nseg, length)[:, :k])
                oi.view(nseg, k).copy_(vals.view(nseg, length)[:, :k])

            def loop():
                for s in range(nseg):
                    single.run_ptr(keys.data_ptr() + s * length * kb, length, k, ok.data_ptr() + s * k * kb, oi.data_ptr() + s * k * 4, key_type=dtype,
                                   sorted=sorted_, stream=stream)

            def torch_topk():
                torch.topk(keys.view(nseg, length), k, dim=1, largest=False, sorted=sorted_)

            def floor():
                red.run_ptr(work.data_ptr(), total * kb // 4, stream)

            candidates = {"batch": (batch, None), "a": (sort_heads, copy), "c": (torch_topk, None), "d": (floor, None)}
            if nseg <= args.loop_max:
                candidates["b"] = (loop, None)
            t = measure(candidates)
            lines.append("%-10s %-22s %6d %-8s %s %s %s %s %s  %d" % (dtype, "%d x %d" % (nseg, length), k, "sorted" if sorted_ else "unsorted",
                                                                      fmt(t["batch"]), fmt(t["a"]), fmt(t.get("b")), fmt(t["c"]), fmt(t["d"]), path))
            print(lines[-1], flush=True)
        del keys, work, iota, vals, ok, oi
        torch.cuda.empty_cache()
    # one mixed batch with device offsets: lengths 1 .. 2^17, most of them short
    rng = np.random.default_rng(12)
    pick = rng.integers(0, 100, 20000)
    lengths = np.where(pick < 60, rng.integers(1, 513, 20000), np.where(pick < 90, rng.integers(513, 8193, 20000),
                       np.where(pick < 99, rng.integers(8193, 32769, 20000), rng.integers(32769, 1 << 17, 20000))))
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    total, nseg, k = int(offsets[-1]), lengths.size, 32
    d_off = torch.from_numpy(offsets.view(np.int32)).cuda()
    for dtype in ("uint32", "float32"):
        keys = torch.randn(total, generator=gen, device="cuda") if dtype == "float32" else torch.randint(0, 1 << 31, (total,), generator=gen,
                                                                                                        device="cuda", dtype=torch.int32)
        work, vals = torch.empty_like(keys), torch.empty(total, dtype=torch.int32, device="cuda")
        ok, oi = torch.empty(nseg * k, dtype=tdt[dtype], device="cuda"), torch.empty(nseg * k, dtype=torch.int32, device="cuda")
        top.prepare_batch(total, nseg, k, dtype)
        sorter.prepare_batch(total, nseg, 4, True)
        for sorted_ in (True, False):
            t = measure({
                "batch": (lambda: top.run_batch_offsets_ptr(keys.data_ptr(), total, d_off.data_ptr(), nseg, k, ok.data_ptr(), oi.data_ptr(),
                                                            key_type=dtype, sorted=sorted_, stream=stream), None),
                "a": (lambda: sorter.sort_batch_offsets_ptr(work.data_ptr(), vals.data_ptr(), total, d_off.data_ptr(), nseg, dtype, stream),
                      lambda: work.copy_(keys)),  # (the sort alone: the gather of ragged heads is not timed)
                "d": (lambda: red.run_ptr(work.data_ptr(), total, stream), None)})
            lines.append("%-10s %-22s %6d %-8s %s %s %s %s %s  %d" % (dtype, "mixed %d segments" % nseg, k, "sorted" if sorted_ else "unsorted",
                                                                      fmt(t["batch"]), fmt(t["a"]), fmt(None), fmt(None), fmt(t["d"]), G.TopKBatch_Binned))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
