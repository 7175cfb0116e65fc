#!/usr/bin/env python3
"""Ladder of the batched select (glu_select_run_batch_ptr, glu_select_run_batch_offsets_ptr): uint32 and byte stencils with 10 % and
50 % selected, writing indices alone or indices and 4-byte items, in GLOBAL and LOCAL form, always with out_offsets, over six segment shapes.

    python tools/select_batch_bench.py [--reps 20] [--quick] [--only TEXT] > profiles/select_batch/ladder.txt

Every row: a stencil made on the device once (nonzero where a random draw says so; the call is NE against a NULL threshold), device
events on the call's stream around the call, 3 warm-up repetitions, median of --reps with min and max, max_out = the number
selected, the object prepared.  Beside every row, in the same process and on the same arrays:
  floor     the single glu_select_run_ptr over the whole array with the same outputs: it moves the same bytes and writes no offsets,
            so it is what the batched call can at best equal
  today     what a caller does without the batched call: that single select, a second select of a key per element with the same
            stencil, and key runs on the compacted keys (which loses the emptied segments)
  torch     torch.masked_select(items, mask) on a ready bool mask, for the rows with items
The kernels of a call cannot be told apart by events around the call: their times come from a run of their own under
`rocprofv3 --kernel-trace --stats -- python tools/select_batch_bench.py --only "one segment" --reps 5` (profiles/select_batch/README.md).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

SHARES = ((0.1, "10%"), (0.5, "50%"))


def shapes(quick):
    """(name, total, how): equal partitions (count, partitions) or a recipe for device offsets."""
    if quick:
        return [("2^20 as one segment", 1 << 20, ("offsets", "one")), ("256 x 4096", 1 << 20, ("equal", 4096, 256)),
                ("2^12 runs of 2^20 sorted keys", 1 << 20, ("offsets", "runs", 1 << 12)), ("2^16 empty around one", 1 << 20, ("offsets", "empties", 1 << 16)),
                ("2^18 at 4096 segments", 1 << 18, ("offsets", "ragged", 4096))]
    return [("2^28 as one segment", 1 << 28, ("offsets", "one")),
            ("4096 x 65536", 1 << 28, ("equal", 65536, 4096)),
            ("2^20 x 256", 1 << 28, ("equal", 256, 1 << 20)),
            ("2^16 runs of 2^26 sorted keys", 1 << 26, ("offsets", "runs", 1 << 16)),
            ("2^24 empty around one of 2^26", 1 << 26, ("offsets", "empties", 1 << 24)),
            ("2^24 at 4096 segments", 1 << 24, ("offsets", "ragged", 4096)),
            ("2^20 at 4096 segments", 1 << 20, ("offsets", "ragged", 4096))]


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


def make_segments(torch, G, stream, total, how):
    """(offsets tensor or None, count, num_segments, a uint32 key per element that is its segment)."""
    if how[0] == "equal":
        _, count, parts = how
        return None, count, parts, (torch.arange(total, dtype=torch.int32, device="cuda") // count)
    kind = how[1]
    gen = torch.Generator(device="cuda").manual_seed(total % 1000 + 7)
    if kind == "one":
        offsets = torch.tensor([0, total], dtype=torch.int64)
    elif kind == "empties":  # half of the empty segments in front of the full one, half behind it
        offsets = torch.cat([torch.zeros(how[2] // 2, dtype=torch.int64), torch.full((how[2] // 2 + 1,), total, dtype=torch.int64)])
    elif kind == "ragged":
        cuts = torch.sort(torch.randint(0, total + 1, (how[2] - 1,), generator=gen, device="cuda"))[0].cpu()
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.full((1,), total, dtype=torch.int64)])
    else:  # "runs": what key runs finds in sorted keys drawn from how[2] values
        keys = torch.sort(torch.randint(0, how[2], (total,), generator=gen, device="cuda", dtype=torch.int32))[0]
        off = torch.empty(how[2] + 1, dtype=torch.int32, device="cuda")
        num = torch.zeros(1, dtype=torch.int32, device="cuda")
        G.KeyRuns().run_ptr(keys.data_ptr(), total, off.data_ptr(), how[2], num.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        return off, 0, how[2], keys
    offsets = offsets.to(torch.int32).cuda()
    n = offsets.numel() - 1
    keys = torch.searchsorted(offsets[1:].contiguous(), torch.arange(total, dtype=torch.int32, device="cuda"), right=True).to(torch.int32)
    return offsets, 0, n, keys


def measure(torch, G, stream, reps, total, seg, stencil_name, share):
    """The eight rows (outputs x forms) of one shape, stencil and share: [(outputs, form, results)]."""
    offsets, count, parts, keys = seg
    gen = torch.Generator(device="cuda").manual_seed(total % 1000 + int(1000 * share))
    mask = torch.rand(total, generator=gen, device="cuda") < share
    selected = int(mask.sum().item())
    byte = stencil_name == "byte"
    stencil = mask.to(torch.uint8) if byte else mask.to(torch.int32) * 0x01010101
    stencil_type = G.SelectStencil_Byte if byte else G.SelectStencil_Uint
    max_out = max(selected, 1)
    items = torch.arange(total, dtype=torch.int32, device="cuda")
    out_items = torch.empty(max_out, dtype=torch.int32, device="cuda")
    out_keys = torch.empty(max_out, dtype=torch.int32, device="cuda")
    out_indices = torch.empty(max_out, dtype=torch.int32, device="cuda")
    out_offsets = torch.empty(parts + 1, dtype=torch.int32, device="cuda")
    run_offsets = torch.empty(min(parts, 1 << 24) + 1, dtype=torch.int32, device="cuda")
    num, num2, num_runs = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(3))
    sel, single, runs = G.Select(), G.Select(), G.KeyRuns()
    sel.prepare_batch(total, parts, stencil_type)
    single.prepare(total, stencil_type)
    runs.prepare(max_out, 32)
    out = []
    for with_items, out_name in ((False, "indices"), (True, "indices + 4 B items")):
        outputs = dict(out_indices_ptr=out_indices.data_ptr(), items_ptr=items.data_ptr() if with_items else None,
                       out_items_ptr=out_items.data_ptr() if with_items else None, item_bytes=4, stencil_type=stencil_type, stream=stream)

        def floor():
            single.run_ptr(stencil.data_ptr(), total, max_out, num.data_ptr(), **outputs)

        def today():
            floor()
            single.run_ptr(stencil.data_ptr(), total, max_out, num2.data_ptr(), items_ptr=keys.data_ptr(), out_items_ptr=out_keys.data_ptr(),
                           item_bytes=4, stencil_type=stencil_type, stream=stream)
            runs.run_ptr(out_keys.data_ptr(), selected, run_offsets.data_ptr(), run_offsets.numel() - 1, num_runs.data_ptr(), stream=stream)

        shared = {"floor": median_ms(torch, reps, floor), "today": median_ms(torch, reps, today),
                  "torch": median_ms(torch, reps, lambda: torch.masked_select(items, mask)) if with_items else None}
        for form, form_name in ((G.SelectIndex_Global, "GLOBAL"), (G.SelectIndex_Local, "LOCAL")):
            def call():
                if offsets is None:
                    sel.run_batch_ptr(stencil.data_ptr(), count, parts, max_out, num.data_ptr(), out_offsets_ptr=out_offsets.data_ptr(),
                                      index_form=form, **outputs)
                else:
                    sel.run_batch_offsets_ptr(stencil.data_ptr(), total, offsets.data_ptr(), parts, max_out, num.data_ptr(),
                                              out_offsets_ptr=out_offsets.data_ptr(), index_form=form, **outputs)

            res = dict(shared, call=median_ms(torch, reps, call), selected=selected)
            torch.cuda.synchronize()
            assert int(num.item()) == selected and int(out_offsets[-1].item()) == selected, "the batched select gave a wrong number"
            out.append((out_name, form_name, res))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="the shapes at 2^20 elements and fewer")
    ap.add_argument("--only", default=None, help="shapes whose name contains this text only (e.g. 'one segment' under a profiler)")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    print("# %s" % G.device_info())
    print("# device events, 3 warm-up + %d repetitions, median (min .. max), ms; max_out = selected; NE against a NULL threshold; out_offsets always" % args.reps)
    print("%-30s %-6s %-4s %-19s %-6s %10s %8s %19s | %8s %19s %6s | %8s %6s | %8s" % (
        "shape", "stencil", "sel", "outputs", "form", "selected", "ms", "(min .. max)", "floor", "(min .. max)", "/floor", "today", "/today", "torch"))
    side = torch.cuda.Stream()  # (the handle of torch's default stream is 0, which the library reads as "the library queue")
    with torch.cuda.stream(side):
        for name, total, how in shapes(args.quick):
            if args.only is not None and args.only not in name:
                continue
            seg = make_segments(torch, G, side.cuda_stream, total, how)
            for stencil_name in ("uint32", "byte"):
                for share, share_name in SHARES:
                    for out_name, form_name, r in measure(torch, G, side.cuda_stream, args.reps, total, seg, stencil_name, share):
                        ms, lo, hi = r["call"]
                        fl, flo, fhi = r["floor"]
                        print("%-30s %-6s %-4s %-19s %-6s %10d %8.4f %19s | %8.4f %19s %6.2f | %8.4f %6.2f | %8s" % (
                            name, stencil_name, share_name, out_name, form_name, r["selected"], ms, "(%.4f .. %.4f)" % (lo, hi), fl,
                            "(%.4f .. %.4f)" % (flo, fhi), ms / fl, r["today"][0], ms / r["today"][0],
                            "%8.4f" % r["torch"][0] if r["torch"] else "-"))
                        sys.stdout.flush()
            del seg
            torch.cuda.empty_cache()
        side.synchronize()
    print("# /floor: the batched call over the single select with the same outputs (no offsets, no segments); /today: over the single select")
    print("# + a select of the keys + key runs on them; torch: masked_select(items, mask) on a ready bool mask")


if __name__ == "__main__":
    main()
