#!/usr/bin/env python3
"""Ladder of select (glu_select_run_ptr): byte and uint32 stencils of 2^20 .. 2^28 elements with 0.1 %, 10 %, 50 % and 100 %
selected, writing indices only, 4-byte items or 16-byte items.

    python tools/select_bench.py [--reps 20] [--quick] [--only TEXT] > profiles/select/ladder.txt

Every row: a stencil made on the device once (nonzero where a random draw says so; the call is NE against a NULL threshold),
device events on the call's stream around the call, 3 warm-up repetitions, median of --reps, max_out = the number selected.
Columns:
  ms        the whole call (its three kernels)
  B/elem    bytes moved per element: two reads of the stencil, the selected items read and written, 4 B per stored index
  of peak   bytes moved / ms over 8 TB/s
  stream    glu_reduce_run_batch_ptr over the stencil's bytes as one partition of 4-byte elements: a read-only stream of the same
            bytes, read once
  torch     what a PyTorch user has today on the same arrays: torch.masked_select(items, mask) for the byte stencil with items,
            torch.nonzero(mask) for the byte stencil with indices only (which synchronises with the host to size its result and
            returns int64 indices: recorded as it is), nothing for uint32 stencils; and torch / ms
The three kernels of a call cannot be told apart by events around the call: their times come from a run of their own under
`rocprofv3 --kernel-trace --stats -- python tools/select_bench.py --only 2^28 --reps 5` (profiles/select/README.md).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

PEAK_BYTES_PER_MS = 8e12 / 1e3
UINT, SUM = 3, 0  # glu::DataType_Uint, glu::ReduceOperator_Sum
SHARES = ((0.001, "0.1%"), (0.1, "10%"), (0.5, "50%"), (1.0, "100%"))
OUTPUTS = ((0, "indices"), (4, "4 B items"), (16, "16 B items"))


def rows(quick):
    out = []
    for lg in ((20, 22) if quick else (20, 24, 26, 28)):
        for stencil in ("byte", "uint32"):
            for share, share_name in SHARES:
                for item_bytes, out_name in OUTPUTS:
                    out.append({"name": "2^%d %s, %s, %s" % (lg, stencil, share_name, out_name), "n": 1 << lg, "stencil": stencil,
                                "share": share, "item_bytes": item_bytes})
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
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def measure(torch, G, stream, row, reps, cache):
    n, share, item_bytes = row["n"], row["share"], row["item_bytes"]
    key = (n, row["stencil"], share)
    if cache.get("key") != key:  # (the three output forms of a row share their stencil)
        cache.clear()
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(n % 1000 + int(1000 * share))
        flags = torch.ones(n, dtype=torch.bool, device="cuda") if share >= 1.0 else torch.rand(n, generator=gen, device="cuda") < share
        cache.update(key=key, selected=int(flags.sum().item()), mask=flags,
                     stencil=flags.to(torch.uint8) if row["stencil"] == "byte" else flags.to(torch.int32) * 0x01010101)
    stencil, selected = cache["stencil"], cache["selected"]
    sb = stencil.element_size()
    byte = row["stencil"] == "byte"
    max_out = max(selected, 1)
    items = torch.arange(n * (item_bytes // 4), dtype=torch.int32, device="cuda") if item_bytes else None
    out_items = torch.empty(max_out * (item_bytes // 4), dtype=torch.int32, device="cuda") if item_bytes else None
    out_indices = None if item_bytes else torch.empty(max_out, dtype=torch.int32, device="cuda")
    num = torch.zeros(1, dtype=torch.int32, device="cuda")
    sel = G.Select()
    stencil_type = G.SelectStencil_Byte if byte else G.SelectStencil_Uint
    sel.prepare(n, stencil_type)

    def call():
        sel.run_ptr(stencil.data_ptr(), n, max_out, num.data_ptr(), out_indices_ptr=out_indices.data_ptr() if out_indices is not None else None,
                    items_ptr=items.data_ptr() if item_bytes else None, out_items_ptr=out_items.data_ptr() if item_bytes else None,
                    item_bytes=item_bytes or 4, stencil_type=stencil_type, stream=stream)

    torch.cuda.synchronize()
    res = {"selected": selected, "call": median_ms(torch, reps, call)}
    torch.cuda.synchronize()
    assert int(num.item()) == selected, "select gave a wrong number"
    # the read-only stream: the batched reduce over the stencil's bytes as one partition of 4-byte elements
    red = G.Reduce(UINT, SUM)
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    words = n * sb // 4
    red.run_batch_ptr(stencil.data_ptr(), out.data_ptr(), words, 1, stream)
    torch.cuda.synchronize()
    res["stream"] = median_ms(torch, reps, lambda: red.run_batch_ptr(stencil.data_ptr(), out.data_ptr(), words, 1, stream))
    other = None
    if byte and item_bytes == 4:
        other = lambda: torch.masked_select(items, cache["mask"])
    elif byte and item_bytes == 16:
        wide = items.view(n, 4)
        other = lambda: wide[cache["mask"]]  # (masked_select takes a mask per scalar: rows go by index)
    elif byte:
        other = lambda: torch.nonzero(cache["mask"])
    res["torch"] = None
    if other:
        try:
            res["torch"] = median_ms(torch, reps, other)
        except RuntimeError as err:
            # torch refuses the launch of its own kernel for some of these shapes; nothing ran and the row says so.  Every other
            # error, a fault of the device among them, ends the ladder.
            if "invalid configuration argument" not in str(err):
                raise
            res["torch"] = "refused"
    res["bytes"] = 2.0 * n * sb + selected * (2.0 * item_bytes if item_bytes else 4.0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="2^20 and 2^22 rows only")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only (e.g. '2^28' under a profiler)")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    table = [row for row in rows(args.quick) if args.only is None or args.only in row["name"]]
    print("# %s" % G.device_info())
    print("# device events, 3 warm-up + %d repetitions, median (min .. max); max_out = selected; NE against a NULL threshold" % args.reps)
    print("%-34s %10s %9s %21s %7s %8s | %9s %7s | %9s %8s" % ("row", "selected", "ms", "(min .. max)", "B/elem", "of peak", "stream ms", "2x/ms",
                                                             "torch ms", "torch/ms"))
    # a stream of our own, made current: the events go where the calls go (the handle of torch's default stream is 0, which the
    # library reads as "the library queue")
    side = torch.cuda.Stream()
    cache = {}
    with torch.cuda.stream(side):
        for row in table:
            r = measure(torch, G, side.cuda_stream, row, args.reps, cache)
            ms, lo, hi = r["call"]
            if r["torch"] == "refused":
                other = "%9s %8s" % ("refused", "-")
            else:
                other = "%9.4f %8.2f" % (r["torch"][0], r["torch"][0] / ms) if r["torch"] else "%9s %8s" % ("-", "-")
            print("%-34s %10d %9.4f %21s %7.2f %7.1f%% | %9.4f %7.3f | %s" % (
                row["name"], r["selected"], ms, "(%.4f .. %.4f)" % (lo, hi), r["bytes"] / row["n"], 100.0 * r["bytes"] / ms / PEAK_BYTES_PER_MS,
                r["stream"][0], 2.0 * r["stream"][0] / ms, other))
            sys.stdout.flush()
        side.synchronize()
    print("# column 2x/ms: twice the read-only stream (the call reads the stencil twice) over the call")
    print("# torch: masked_select(items, mask) for 4 B items, items.view(n, 4)[mask] for 16 B items, nonzero(mask) (int64, host sync) for indices;")
    print("# refused: torch raised at the launch of its own kernel (HIP: invalid configuration argument) and has no figure for the row")


if __name__ == "__main__":
    main()
