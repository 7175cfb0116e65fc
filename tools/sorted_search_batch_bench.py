#!/usr/bin/env python3
"""Ladder of the batched sorted search (glu_sorted_search_run_batch_ptr, glu_sorted_search_run_batch_offsets_ptr): every row's
needles in that row's own haystack, against torch.searchsorted on the 2-D tensors in the same process on the same data, against the
loop of this library's single calls, against one single DIRECT call over the same totals, and against itself without the LDS window.

    python tools/sorted_search_batch_bench.py [--reps 10] [--quick] [--only TEXT] [--timeout 600] > profiles/sorted_search_batch/ladder.txt

Every row runs in a child process of its own under its own timeout, and the ladder stops at the first row that fails.  In a row the
data are made on the device once; device events on the call's stream around the call, 3 warm-up repetitions, median of --reps.  Both
bounds are asked for everywhere.  Columns:
  glu       the batched call at the default window; ms, and million needles per second
  window 0  the same call after set_batch_window(0): every probe in global memory; ms, and window 0 / glu
  torch     torch.searchsorted(hay2d, needles2d) and the same with right=True, where the shape is rectangular (int32 results, as
            the library's); ms, and torch / glu
  loop      one glu_sorted_search_run_ptr per row on the AUTO path (it builds an index where that pays), up to 4096 rows; ms, and
            loop / glu
  direct    ONE glu_sorted_search_run_ptr on the DIRECT path over the same totals as one segment (all the keys as one haystack, all
            the needles): what the probes cost without the per-needle segment; the answers differ, the times compare; ms, and
            direct / glu
The batched outputs at both windows are compared with torch's (the ragged row: with the global bounds minus the segment's begin).
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

LOOP_ROWS_MAX = 4096


def rows():
    out = []
    for key_type in ("uint32", "uint64"):
        for needles in ("random", "sorted"):
            for b, e in ((65536, 7), (4096, 12), (64, 20), (8, 24)):
                out.append({"name": "%d x (2^%d, 2^%d) %s, %s needles" % (b, e, e, key_type, needles), "rows": b, "n": 1 << e, "m": 1 << e,
                            "key_type": key_type, "needles": needles})
        out.append({"name": "ragged: key runs of 2^26 %s keys, 2^16 groups" % key_type, "ragged": 26, "group_bits": 16, "key_type": key_type})
    return out


QUICK_ROWS = [{"name": "256 x (2^7, 2^7) uint32, random needles", "rows": 256, "n": 128, "m": 128, "key_type": "uint32", "needles": "random"},
              {"name": "4 x (2^14, 2^14) uint64, sorted needles", "rows": 4, "n": 1 << 14, "m": 1 << 14, "key_type": "uint64", "needles": "sorted"},
              {"name": "ragged: key runs of 2^18 uint32 keys, 2^8 groups", "ragged": 18, "group_bits": 8, "key_type": "uint32"}]
HEADER = "%-52s %9s %8s | %9s %6s | %9s %6s | %9s %6s | %9s %6s" % ("row", "glu", "Mneedle/s", "window 0", "/glu", "torch", "/glu", "loop",
                                                                  "/glu", "direct", "/glu")


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


def random_keys(torch, gen, shape, key_type):
    """non-negative keys, so that torch's signed order is the library's unsigned one"""
    if key_type == "uint32":
        return torch.randint(0, 2 ** 31 - 1, shape, generator=gen, dtype=torch.int32, device="cuda")
    return torch.randint(0, 2 ** 62, shape, generator=gen, dtype=torch.int64, device="cuda")


def direct_ms(torch, G, stream, reps, hay, needles, key_type, lower, upper):
    single = G.SortedSearch()
    single.set_option("PATH", G.SearchPath_Direct)
    return median_ms(torch, reps, lambda: single.run_ptr(hay.data_ptr(), hay.numel(), needles.data_ptr(), needles.numel(), lower.data_ptr(),
                                                         upper.data_ptr(), key_type, False, stream))


def measure_rows(torch, G, stream, row, reps):
    b, n, m, key_type = row["rows"], row["n"], row["m"], row["key_type"]
    gen = torch.Generator(device="cuda").manual_seed(b % 1000 + n % 1000)
    hay = torch.sort(random_keys(torch, gen, (b, n), key_type), dim=1).values.contiguous()
    needles = random_keys(torch, gen, (b, m), key_type)
    if row["needles"] == "sorted":
        needles = torch.sort(needles, dim=1).values.contiguous()
    lower, upper = torch.empty((b, m), dtype=torch.int32, device="cuda"), torch.empty((b, m), dtype=torch.int32, device="cuda")
    search = G.SortedSearch()
    call = lambda: search.run_batch_ptr(hay.data_ptr(), n, needles.data_ptr(), m, b, lower.data_ptr(), upper.data_ptr(), key_type, stream)
    torch.cuda.current_stream().synchronize()
    ms = median_ms(torch, reps, call)
    assert search.last() == (G.SearchPath_Batch, 0, 1)
    want_lower = torch.searchsorted(hay, needles, out_int32=True)
    want_upper = torch.searchsorted(hay, needles, right=True, out_int32=True)
    assert torch.equal(lower, want_lower) and torch.equal(upper, want_upper), "the batched search differs from torch.searchsorted"
    lower.fill_(-1)
    upper.fill_(-1)
    search.set_batch_window(0)
    ms0 = median_ms(torch, reps, call)
    assert torch.equal(lower, want_lower) and torch.equal(upper, want_upper), "window 0 differs from torch.searchsorted"
    del want_lower, want_upper
    torch_ms = median_ms(torch, reps, lambda: (torch.searchsorted(hay, needles, out_int32=True),
                                               torch.searchsorted(hay, needles, right=True, out_int32=True)))
    loop_ms = None
    if b <= LOOP_ROWS_MAX:
        single = G.SortedSearch()
        single.prepare(n, key_type)
        kb = hay.element_size()

        def loop():
            for p in range(b):
                single.run_ptr(hay.data_ptr() + p * n * kb, n, needles.data_ptr() + p * m * kb, m, lower.data_ptr() + 4 * p * m,
                               upper.data_ptr() + 4 * p * m, key_type, False, stream)

        loop_ms = median_ms(torch, reps, loop)
    d_ms = direct_ms(torch, G, stream, reps, hay, needles, key_type, lower, upper)
    return ms, b * m, ms0, torch_ms, loop_ms, d_ms


def measure_ragged(torch, G, stream, row, reps):
    """Two sorted arrays of 2^e keys; a group is the keys equal in their top group_bits bits (of the 31 or 62 bits drawn); key runs
    on either side writes the offsets on the device; every needle's bounds within the matching group of the haystack."""
    count, key_type, gb = 1 << row["ragged"], row["key_type"], row["group_bits"]
    bits = 31 if key_type == "uint32" else 62
    gen = torch.Generator(device="cuda").manual_seed(count % 1000 + gb)
    hay = torch.sort(random_keys(torch, gen, (count,), key_type)).values
    needles = torch.sort(random_keys(torch, gen, (count,), key_type)).values
    groups = 1 << gb
    offsets = [torch.empty(groups + 1, dtype=torch.int32, device="cuda") for _ in range(2)]
    num = torch.zeros(2, dtype=torch.int32, device="cuda")
    runs = G.KeyRuns()
    torch.cuda.current_stream().synchronize()
    for side, keys in enumerate((hay, needles)):
        runs.run_ptr(keys.data_ptr(), count, offsets[side].data_ptr(), groups, num.data_ptr() + 4 * side, None, 8 * keys.element_size(),
                     bits - gb, bits, stream)
    torch.cuda.current_stream().synchronize()
    assert num.tolist() == [groups, groups], "a group is missing on one side: %r" % (num.tolist(),)
    lower, upper = torch.empty(count, dtype=torch.int32, device="cuda"), torch.empty(count, dtype=torch.int32, device="cuda")
    search = G.SortedSearch()
    call = lambda: search.run_batch_offsets_ptr(hay.data_ptr(), count, offsets[0].data_ptr(), needles.data_ptr(), count, offsets[1].data_ptr(),
                                                groups, lower.data_ptr(), upper.data_ptr(), key_type, stream)
    ms = median_ms(torch, reps, call)
    # the whole haystack is sorted and a needle's group holds exactly the keys with its top bits: local = global - the group's begin
    begin = offsets[0][(needles >> (bits - gb)).long()]
    want_lower = torch.searchsorted(hay, needles, out_int32=True) - begin
    want_upper = torch.searchsorted(hay, needles, right=True, out_int32=True) - begin
    assert torch.equal(lower, want_lower) and torch.equal(upper, want_upper), "the batched search differs from the global bounds"
    lower.fill_(-1)
    upper.fill_(-1)
    search.set_batch_window(0)
    ms0 = median_ms(torch, reps, call)
    assert torch.equal(lower, want_lower) and torch.equal(upper, want_upper), "window 0 differs from the global bounds"
    del want_lower, want_upper, begin
    d_ms = direct_ms(torch, G, stream, reps, hay, needles, key_type, lower, upper)
    return ms, count, ms0, None, None, d_ms


def run_row(name, reps):
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    row = next(r for r in rows() + QUICK_ROWS if r["name"] == name)
    # a stream of our own, made current: the events go where the calls go
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ms, count, ms0, torch_ms, loop_ms, d_ms = (measure_ragged if "ragged" in row else measure_rows)(torch, G, side.cuda_stream, row, reps)
        side.synchronize()
    cell = lambda v: "%9s %6s" % ("-", "-") if v is None else "%9.4f %6.2f" % (v, v / ms)
    print("%-52s %9.4f %8.0f | %s | %s | %s | %s" % (name, ms, count / ms / 1e3, cell(ms0), cell(torch_ms), cell(loop_ms), cell(d_ms)))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="three small rows only")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only")
    ap.add_argument("--timeout", type=int, default=600, help="seconds a row's process may take")
    ap.add_argument("--row", default=None, help="(internal) measure this row in this process")
    args = ap.parse_args()
    if args.row is not None:
        run_row(args.row, args.reps)
        return 0
    table = [row for row in (QUICK_ROWS if args.quick else rows()) if args.only is None or args.only in row["name"]]
    print("# device events, 3 warm-up + %d repetitions, median; ms; both bounds; x/glu above 1: the batched call at the default window is "
          "ahead" % args.reps)
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
    print("# window 0: set_batch_window(0); torch: torch.searchsorted on the 2-D tensors, left and right; loop: one single call per row "
          "(AUTO); direct: one single DIRECT call over the same totals")
    return 0


if __name__ == "__main__":
    sys.exit(main())
