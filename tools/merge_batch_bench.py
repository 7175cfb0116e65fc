#!/usr/bin/env python3
"""Ladder of the batched merge (glu_merge_run_batch_offsets_ptr): the two sorted runs of every segment into one, all segments in one
call, beside the three other ways to spend the same device time.

    python tools/merge_batch_bench.py [--reps 20] [--quick] [--only TEXT] [--timeout 900] > profiles/merge_batch/ladder.txt

Rows: one segment of 2^27 + 2^27 uint32 pairs; 4096 x (32768 + 32768); 65536 x (2048 + 2048); 2^20 x (128 + 128); the 2^16 ragged
groups of 2^26 keys on each side (group = 16 random bits, what key runs finds in the sorted group keys); 2^24 segments around one
non-empty segment of 2^26 + 2^26; the first two rows again with uint64 keys and with keys alone; 2^20 + 2^20 in 64 segments.
Every row runs in a child process of its own under its own timeout, and the ladder stops at the first row that fails.  In a row the
data is made and sorted per segment on the device once; device events on the call's stream around each call; 3 warm-up repetitions,
then --reps repetitions in which the batched call and the floor ALTERNATE; median, and the lowest and highest repetition.  Columns:
  batch     glu_merge_run_batch_offsets_ptr with out_offsets after glu_merge_prepare_batch: partition kernel, tile kernel; ms
            (median, min .. max)
  GB/s      the bytes a merge has to move (every key and value read once and written once) over that time
  floor     glu_merge_run_ptr over the same totals with the segments ignored (both arrays sorted as a whole): the same bytes through
            kernels this ladder's subject does not touch; ms (median, min .. max); and batch / floor
  loop      glu_merge_run_ptr once per non-empty segment, host-known lengths; ms and loop / batch.  Above 4096 calls a repetition
            the loop is timed once after one untimed pass, not --reps times
  sort      what a caller had: the batched sort (glu_radix_sort_run_batch_offsets_ptr) of the rows A_s || B_s laid back to back
            (a pristine copy before every repetition, outside the timed region); ms and sort / batch
The batched call's keys, values and out_offsets are compared with torch's stable sort by (segment, key) of the same rows.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

ROWS = [
    {"name": "1 x (2^27 + 2^27) u32 pairs", "S": 1, "na": 1 << 27, "nb": 1 << 27, "key_type": "uint32", "vals": True, "shape": "equal"},
    {"name": "4096 x (32768 + 32768) u32 pairs", "S": 4096, "na": 1 << 27, "nb": 1 << 27, "key_type": "uint32", "vals": True, "shape": "equal"},
    {"name": "65536 x (2048 + 2048) u32 pairs", "S": 65536, "na": 1 << 27, "nb": 1 << 27, "key_type": "uint32", "vals": True, "shape": "equal"},
    {"name": "2^20 x (128 + 128) u32 pairs", "S": 1 << 20, "na": 1 << 27, "nb": 1 << 27, "key_type": "uint32", "vals": True, "shape": "equal"},
    {"name": "2^16 ragged groups, 2^26 + 2^26 u32 pairs", "S": 1 << 16, "na": 1 << 26, "nb": 1 << 26, "key_type": "uint32", "vals": True, "shape": "ragged"},
    {"name": "2^24 segments, one of 2^26 + 2^26 u32 pairs", "S": 1 << 24, "na": 1 << 26, "nb": 1 << 26, "key_type": "uint32", "vals": True, "shape": "one"},
    {"name": "1 x (2^27 + 2^27) u64 pairs", "S": 1, "na": 1 << 27, "nb": 1 << 27, "key_type": "uint64", "vals": True, "shape": "equal"},
    {"name": "4096 x (32768 + 32768) u64 pairs", "S": 4096, "na": 1 << 27, "nb": 1 << 27, "key_type": "uint64", "vals": True, "shape": "equal"},
    {"name": "1 x (2^27 + 2^27) u32 keys", "S": 1, "na": 1 << 27, "nb": 1 << 27, "key_type": "uint32", "vals": False, "shape": "equal"},
    {"name": "4096 x (32768 + 32768) u32 keys", "S": 4096, "na": 1 << 27, "nb": 1 << 27, "key_type": "uint32", "vals": False, "shape": "equal"},
    {"name": "64 x (16384 + 16384) u32 pairs", "S": 64, "na": 1 << 20, "nb": 1 << 20, "key_type": "uint32", "vals": True, "shape": "equal"},
]
QUICK_ROWS = [
    {"name": "quick 1 x (2^18 + 2^18) u32 pairs", "S": 1, "na": 1 << 18, "nb": 1 << 18, "key_type": "uint32", "vals": True, "shape": "equal"},
    {"name": "quick 2^12 ragged groups u64 keys", "S": 1 << 12, "na": 1 << 18, "nb": 1 << 17, "key_type": "uint64", "vals": False, "shape": "ragged"},
    {"name": "quick 2^16 segments, one non-empty", "S": 1 << 16, "na": 1 << 18, "nb": 1 << 18, "key_type": "uint32", "vals": True, "shape": "one"},
]
HEADER = "%-46s %24s %6s | %24s %6s | %10s %7s | %9s %6s" % ("row", "batch (min .. max)", "GB/s", "floor (min .. max)", "b/f", "loop", "l/b",
                                                            "sort", "s/b")
LOOP_REPS_ABOVE = 4096


def bytes_per_pair(row):
    return 2 * ((8 if row["key_type"] == "uint64" else 4) + (4 if row["vals"] else 0))


def timed(torch, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(times):
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def make_side(torch, row, n, gen):
    """(keys sorted per segment, offsets as a device int32 tensor of S + 1 words, the segment of every element)."""
    S, dtype = row["S"], torch.int32 if row["key_type"] == "uint32" else torch.int64
    if row["shape"] == "equal":
        seg = torch.arange(n, device="cuda", dtype=torch.int64) // (n // S)
    elif row["shape"] == "ragged":
        seg = torch.randint(0, S, (n,), generator=gen, device="cuda", dtype=torch.int64).sort().values
    else:  # one non-empty segment in the middle
        seg = torch.full((n,), S // 2, device="cuda", dtype=torch.int64)
    keys = torch.randint(0, 2 ** 31 - 1, (n,), generator=gen, device="cuda", dtype=torch.int64)
    keys = ((seg << 32) | keys).sort().values & 0xFFFFFFFF  # sorted inside every segment
    offsets = torch.searchsorted(seg, torch.arange(S + 1, device="cuda", dtype=torch.int64)).to(torch.int32)
    return keys.to(dtype), offsets, seg


def measure(torch, G, stream, row, reps):
    S, na, nb, key_type, with_vals = row["S"], row["na"], row["nb"], row["key_type"], row["vals"]
    total = na + nb
    gen = torch.Generator(device="cuda").manual_seed(total % 1000 + S % 977)
    a, ao, seg_a = make_side(torch, row, na, gen)
    b, bo, seg_b = make_side(torch, row, nb, gen)
    av = torch.arange(na, dtype=torch.int32, device="cuda") if with_vals else None
    bv = torch.arange(nb, dtype=torch.int32, device="cuda") + (-2 ** 31) if with_vals else None  # (the bits of iota + 2^31)
    out_k = torch.empty(total, dtype=a.dtype, device="cuda")
    out_v = torch.empty(total, dtype=torch.int32, device="cuda") if with_vals else None
    out_o = torch.empty(S + 1, dtype=torch.int32, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    kb = a.element_size()

    # the floor's inputs: the same keys sorted as a whole
    fa, fb = a.sort().values, b.sort().values
    floor_k = torch.empty_like(out_k)
    floor_v = torch.empty_like(out_v) if with_vals else None
    torch.cuda.empty_cache()

    merge, single = G.Merge(), G.Merge()
    merge.prepare_batch(total, key_type)
    single.prepare(total, key_type)
    batch = lambda: merge.run_batch_offsets_ptr(ptr(a), ptr(av), ptr(ao), na, ptr(b), ptr(bv), ptr(bo), nb, S, ptr(out_k), ptr(out_v),  # noqa: E731
                                                ptr(out_o), key_type, stream)
    floor = lambda: single.run_ptr(ptr(fa), ptr(av), na, ptr(fb), ptr(bv), nb, ptr(floor_k), ptr(floor_v), key_type, stream)  # noqa: E731
    tb, tf = [], []
    for rep in range(reps + 3):
        x, y = timed(torch, batch), timed(torch, floor)
        if rep >= 3:
            tb.append(x)
            tf.append(y)
    assert merge.last() == G.plan_merge_batch(total, S, key_type, with_vals)[1:3]
    res = {"batch": stats(tb), "floor": stats(tf)}
    del fa, fb, floor_k, floor_v

    # against torch: the stable sort by (segment, key) of A's rows in front of B's
    both_seg, both_k = torch.cat((seg_a, seg_b)), torch.cat((a, b)).to(torch.int64)
    order = ((both_seg << 32) | both_k).sort(stable=True).indices
    assert torch.equal(out_k, torch.cat((a, b))[order]), "the merged keys differ from torch's stable sort by (segment, key)"
    if with_vals:
        assert torch.equal(out_v, torch.cat((av, bv))[order]), "the merged values differ from torch's stable sort by (segment, key)"
    assert torch.equal(out_o, ao + bo), "out_offsets differ"
    del both_seg, both_k, order, seg_a, seg_b
    torch.cuda.empty_cache()

    # the loop of single calls, over the non-empty segments
    hao, hbo = ao.cpu().numpy().astype(np.int64), bo.cpu().numpy().astype(np.int64)
    live = np.flatnonzero((np.diff(hao) + np.diff(hbo)) > 0)
    calls = [(int(hao[s]), int(hao[s + 1] - hao[s]), int(hbo[s]), int(hbo[s + 1] - hbo[s])) for s in live]
    loop_k = torch.empty_like(out_k)
    loop_v = torch.empty_like(out_v) if with_vals else None

    def loop():
        for a0, la, b0, lb in calls:
            o = a0 + b0
            single.run_ptr(ptr(a) + kb * a0, ptr(av) + 4 * a0 if with_vals else None, la, ptr(b) + kb * b0, ptr(bv) + 4 * b0 if with_vals else None,
                           lb, ptr(loop_k) + kb * o, ptr(loop_v) + 4 * o if with_vals else None, key_type, stream)

    if len(calls) > LOOP_REPS_ABOVE:
        timed(torch, loop)
        res["loop"] = timed(torch, loop)
    else:
        res["loop"] = float(np.median([timed(torch, loop) for _ in range(reps + 3)][3:]))
    assert torch.equal(loop_k, out_k), "the loop's keys differ from the batched call's"
    del loop_k, loop_v

    # what a caller had: the batched sort of the rows A_s || B_s laid back to back (the merged rows hold the same elements per row)
    work_k = torch.empty_like(out_k)
    work_v = torch.empty_like(out_v) if with_vals else None
    perm = torch.randperm(total, device="cuda") if S == 1 else None  # (one row: any order of it is a fair input)
    sort = G.RadixSort()
    sort.prepare_batch(total, S, kb, with_vals)

    def pristine():
        work_k.copy_(out_k if perm is None else out_k[perm])
        if with_vals:
            work_v.copy_(out_v if perm is None else out_v[perm])

    ts = []
    for rep in range(reps + 3):
        pristine()
        ts.append(timed(torch, lambda: sort.sort_batch_offsets_ptr(ptr(work_k), ptr(work_v), total, ptr(out_o), S, key_type, stream)))
    res["sort"] = float(np.median(ts[3:]))
    assert torch.equal(work_k, out_k), "the batched sort of the rows differs from the batched merge"
    return res


def run_row(name, reps):
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    row = next(r for r in ROWS + QUICK_ROWS if r["name"] == name)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r = measure(torch, G, side.cuda_stream, row, reps)
        side.synchronize()
    b, f = r["batch"], r["floor"]
    gbs = bytes_per_pair(row) * (row["na"] + row["nb"]) / (b[0] * 1e-3) / 1e9
    print("%-46s %8.4f (%6.4f .. %6.4f) %6.0f | %8.4f (%6.4f .. %6.4f) %6.3f | %10.3f %7.1f | %9.4f %6.2f" % (
        name, b[0], b[1], b[2], gbs, f[0], f[1], f[2], b[0] / f[0], r["loop"], r["loop"] / b[0], r["sort"], r["sort"] / b[0]))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="three small rows only")
    ap.add_argument("--only", default=None, help="rows whose name contains this text only")
    ap.add_argument("--timeout", type=int, default=900, help="seconds a row's process may take")
    ap.add_argument("--row", default=None, help="(internal) measure this row in this process")
    args = ap.parse_args()
    if args.row is not None:
        run_row(args.row, args.reps)
        return 0
    table = [row for row in (QUICK_ROWS if args.quick else ROWS) if args.only is None or args.only in row["name"]]
    print("# device events, 3 warm-up + %d repetitions (batch and floor alternate), median (min .. max); ms; GB/s = the bytes a merge has "
          "to move over the batched call's median" % args.reps)
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
    print("# floor: glu_merge_run_ptr over the same totals, both arrays sorted as a whole; loop: glu_merge_run_ptr per non-empty segment "
          "(timed once above %d calls); sort: the batched sort of the rows A_s || B_s" % LOOP_REPS_ABOVE)
    return 0


if __name__ == "__main__":
    sys.exit(main())
