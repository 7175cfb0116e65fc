#!/usr/bin/env python3
"""Ladder of expand (glu_expand_run_ptr): segment ids, ranks and items per element from the offsets of the segments, against the one
composition there was before it (a materialised iota searched in the offsets) and against torch.

    python tools/expand_bench.py [--reps 20] [--quick] [--only TEXT] [--timeout 600] > profiles/expand/ladder.txt

Rows: total in 2^20, 2^24, 2^28, every segment of one length in 16, 256, 4096, 2^20, or one segment; at 2^28 also geometric lengths
(mean 37), the key-runs form (2^24 slots of which 2^16 hold runs, the rest `total`) and 2^22 segments of which half are empty.
Every row runs in a child process of its own under its own timeout, and the ladder stops at the first row that fails.  In a row the
offsets are made on the device once; device events on the call's stream around the call, 3 warm-up repetitions, median of --reps.
A row prints four lines, one per set of outputs: ids (out_segments), ids+ranks, items4 (4-byte items alone), items16.  Columns:
  expand    glu_expand_run_ptr after glu_expand_prepare: the partition kernel and the tile kernel; ms
  MB        the bytes the call must move: the offsets read once, each requested output written once
  GB/s      that over the time, and that rate over the 8 TB/s peak of HBM
  (a)       the composition without expand: glu_sorted_search_run_ptr, upper bounds of an iota 0 .. total - 1 in the offsets.  The
            iota is made outside the timed region.  It gives the ids alone (plus one), whatever the line asks for; ms, and (a) / expand
  (b)       torch.searchsorted(offsets, iota, right=True) on the same iota; ms, and (b) / expand
  (c)       torch.repeat_interleave(items, counts, output_size=total), on the item lines; ms, and (c) / expand
The ids of every row are compared with (a)'s bounds minus one, the items with those of (a)'s segments.  (c) is not tried for
2^28 outputs, which torch refuses to launch; the column says so.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

PEAK_GBS = 8000.0  # HBM3E of one MI355X
LINES = [("ids", True, False, 0), ("ids+ranks", True, True, 0), ("items4", False, False, 4), ("items16", False, False, 16)]


def rows():
    out = []
    for e in (20, 24, 28):
        for length, label in ((16, "16"), (256, "256"), (4096, "4096"), (1 << 20, "2^20"), (None, "one segment")):
            if length is not None and length >= (1 << e):
                continue  # (that is the one-segment row)
            out.append({"name": "2^%d, %s" % (e, "segments of " + label if length else label), "total": 1 << e, "kind": "even",
                        "length": length or (1 << e)})
    out.append({"name": "2^28, geometric mean 37", "total": 1 << 28, "kind": "geometric"})
    out.append({"name": "2^28, key runs 2^16 of 2^24", "total": 1 << 28, "kind": "key_runs"})
    out.append({"name": "2^28, 2^22 segments half empty", "total": 1 << 28, "kind": "half_empty"})
    return out


QUICK_ROWS = [{"name": "2^18, segments of 16", "total": 1 << 18, "kind": "even", "length": 16},
              {"name": "2^18, geometric mean 37", "total": 1 << 18, "kind": "geometric"}]
HEADER = "%-32s %-9s %9s %8s %7s %6s | %9s %8s | %9s %8s | %9s %8s" % (
    "row", "outputs", "expand", "MB", "GB/s", "peak", "(a)", "(a)/exp", "(b)", "(b)/exp", "(c)", "(c)/exp")


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


def make_lengths(torch, row):
    """int64 segment lengths on the device that sum to at most total"""
    total, kind = row["total"], row["kind"]
    gen = torch.Generator(device="cuda").manual_seed(total % 1000 + len(kind))
    if kind == "even":
        return torch.full((total // row["length"],), row["length"], dtype=torch.int64, device="cuda")
    if kind == "geometric":
        n = total // 37
        u = torch.rand(n, generator=gen, device="cuda", dtype=torch.float64)
        lens = torch.floor(torch.log1p(-u) / np.log1p(-1.0 / 38.0)).to(torch.int64)  # geometric from 0 on, mean 37
        keep = torch.cumsum(lens, 0) <= total
        return lens[keep]
    if kind == "key_runs":  # 2^16 runs of equal length, then slots that hold `total`: empty segments behind the last run
        runs, slots = 1 << 16, 1 << 24
        lens = torch.zeros(slots, dtype=torch.int64, device="cuda")
        lens[:runs] = total // runs
        return lens
    n = 1 << 22  # half_empty: every second segment empty, the others of one length
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    lens[::2] = total // (n // 2)
    return lens


def measure(torch, G, stream, row, reps):
    total = row["total"]
    lens = make_lengths(torch, row)
    n = lens.numel()
    offsets64 = torch.cat((torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(lens, 0)))
    assert int(offsets64[-1]) <= total < 2 ** 31
    offsets = offsets64.to(torch.int32)
    counts = lens.to(torch.int32)
    covered_total = int(offsets64[-1])  # (read here: no host read inside a timed region)
    del lens, offsets64
    iota = torch.arange(total, dtype=torch.int32, device="cuda")
    ids = torch.empty(total, dtype=torch.int32, device="cuda")
    ranks = torch.empty(total, dtype=torch.int32, device="cuda")
    upper = torch.empty(total, dtype=torch.int32, device="cuda")
    # items that follow from their segment (int32 arithmetic wraps), so that the outputs are checked with elementwise operations alone
    scrambled = torch.arange(n, dtype=torch.int32, device="cuda") * 40503 + 17
    items = {4: scrambled, 16: (scrambled[:, None] + torch.arange(4, dtype=torch.int32, device="cuda") * 0x01010101).contiguous()}
    torch.cuda.empty_cache()

    expand = G.Expand()
    expand.prepare(total, n)
    search = G.SortedSearch()
    a_ms = median_ms(torch, reps, lambda: search.run_ptr(offsets.data_ptr(), n + 1, iota.data_ptr(), total, None, upper.data_ptr(), "uint32",
                                                        stream=stream))
    b_ms = median_ms(torch, reps, lambda: torch.searchsorted(offsets, iota, right=True))
    results = []
    for label, want_ids, want_ranks, item_bytes in LINES:
        out = torch.empty((total, item_bytes // 4), dtype=torch.int32, device="cuda") if item_bytes else None
        it = items.get(item_bytes)
        ms = median_ms(torch, reps, lambda: expand.run_ptr(offsets.data_ptr(), n, total, ids.data_ptr() if want_ids else None,
                                                           ranks.data_ptr() if want_ranks else None, it.data_ptr() if item_bytes else None,
                                                           out.data_ptr() if item_bytes else None, item_bytes or 4, stream))
        assert expand.last() == G.plan_expand(total, n)[1:3]
        moved = 4 * (n + 1) + total * (4 * want_ids + 4 * want_ranks + item_bytes)
        c_ms = None
        if want_ids:
            covered = upper <= n
            covered &= upper >= 1
            zero = torch.zeros((), dtype=torch.int32, device="cuda")
            assert torch.equal(torch.where(covered, ids, zero), torch.where(covered, upper - 1, zero)), "the ids differ from the searched iota's"
            del covered
        if item_bytes:
            covered = (upper >= 1) & (upper <= n)
            want = (upper - 1) * 40503 + 17  # the item of (a)'s segment
            if item_bytes == 16:
                want, covered = want[:, None] + torch.arange(4, dtype=torch.int32, device="cuda") * 0x01010101, covered[:, None]
            zero = torch.zeros((), dtype=torch.int32, device="cuda")
            assert torch.equal(torch.where(covered, out.reshape(want.shape), zero), torch.where(covered, want, zero)), \
                "the items differ from those of the searched iota's segments"
            del want, covered
            if total >= 1 << 28:  # torch refuses this launch for 2^28 outputs ("invalid configuration argument"): not tried
                c_ms = float("nan")
            else:
                c_ms = median_ms(torch, reps, lambda: torch.repeat_interleave(it, counts, dim=0, output_size=covered_total))
        results.append((label, ms, moved, c_ms))
        del out
        torch.cuda.empty_cache()
    return a_ms, b_ms, results


def run_row(name, reps):
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    row = next(r for r in rows() + QUICK_ROWS if r["name"] == name)
    # a stream of our own, made current: the events go where the calls go (the handle of torch's default stream is 0, which the
    # library reads as "the library queue")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a_ms, b_ms, results = measure(torch, G, side.cuda_stream, row, reps)
        side.synchronize()
    for label, ms, moved, c_ms in results:
        gbs = moved / (ms * 1e-3) / 1e9
        c = "%9s %8s" % ("-", "-") if c_ms is None else "%9s %8s" % ("refused", "-") if c_ms != c_ms else "%9.4f %8.2f" % (c_ms, c_ms / ms)
        print("%-32s %-9s %9.4f %8.1f %7.0f %5.1f%% | %9.4f %8.2f | %9.4f %8.2f | %s" % (
            name, label, ms, moved / 1e6, gbs, 100.0 * gbs / PEAK_GBS, a_ms, a_ms / ms, b_ms, b_ms / ms, c))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="two small rows only")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only")
    ap.add_argument("--timeout", type=int, default=600, help="seconds a row's process may take")
    ap.add_argument("--row", default=None, help="(internal) measure this row in this process")
    args = ap.parse_args()
    if args.row is not None:
        run_row(args.row, args.reps)
        return 0
    table = [row for row in (QUICK_ROWS if args.quick else rows()) if args.only is None or args.only in row["name"]]
    print("# device events, 3 warm-up + %d repetitions, median; ms; MB = the offsets read once and each requested output written once; "
          "peak = GB/s over %d GB/s" % (args.reps, PEAK_GBS))
    print(HEADER)
    sys.stdout.flush()
    for row in table:
        # a fresh child per row, under its own time limit; a row that fails, dies or runs out of time ends the ladder
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", row["name"], "--reps", str(args.reps)], timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("# %s: no result within %d s; the ladder stops here" % (row["name"], args.timeout))
            return 124
        if p.returncode != 0:
            print("# %s: exit status %d; the ladder stops here" % (row["name"], p.returncode))
            return p.returncode if p.returncode > 0 else 1
    print("# (a): glu_sorted_search_run_ptr, upper bounds of an iota in the offsets, the iota made outside the timed region; "
          "(b): torch.searchsorted(offsets, iota, right=True); (c): torch.repeat_interleave(items, counts, output_size=total)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
