#!/usr/bin/env python3
"""Ladder of the batched set operations (glu_set_ops_run_batch_offsets_ptr): the set operation of the two sorted runs of every segment,
all segments in one call, beside the other ways to spend the same device time.

    python tools/set_ops_batch_bench.py [--reps 20] [--quick] [--only TEXT] [--timeout 900] > profiles/set_ops_batch/ladder.txt

Rows: one segment of 2^27 + 2^27 uint32 pairs, about half of the keys shared, once per operation and once only counting; then, as a
union (the operation that writes the most): 4096 x (32768 + 32768); 65536 x (2048 + 2048); 2^20 x (128 + 128); the 2^16 ragged groups
of 2^26 keys on each side; 2^24 segments around one non-empty segment of 2^26 + 2^26; keys alone; uint64 pairs; 2^20 + 2^20 in 64
segments.  Every row runs in a child process of its own under its own timeout, and the ladder stops at the first row that fails.  In a
row the data is made and sorted per segment on the device once (the keys of a segment are drawn from 1.44 x its length values: about
half of A's keys are in B); device events on the call's stream around each call; 3 warm-up repetitions, then --reps repetitions in which
the batched call, the floor and the batched merge ALTERNATE; median, and the lowest and highest repetition.  Columns:
  batch     glu_set_ops_run_batch_offsets_ptr with out_offsets after glu_set_ops_prepare_batch; ms (median, min .. max)
  floor     glu_set_ops_run_ptr over the same totals with the segments ignored (both arrays sorted as a whole): other results, the
            same bytes and the same walk through kernels this ladder's subject does not touch; ms (median, min .. max); batch / floor
  merge     glu_merge_run_batch_offsets_ptr of the same inputs; ms and batch / merge
  loop      glu_set_ops_run_ptr once per non-empty segment, host-known lengths, num_out words side by side; ms and loop / batch; only
            where the row says so; above 4096 calls a repetition it is timed once after one untimed pass
Checks: with one segment the batched call's bytes are the floor's; where the loop runs, its keys and counts are the batched call's;
everywhere out_offsets[S] = *num_out and the four cardinalities satisfy |U| + |I| = a_total + b_total, |D| = a_total - |I|,
|SD| = |U| - |I| (counting calls with out_offsets).
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))

OPS = ["union", "intersection", "difference", "symmetric_difference"]


def row(name, S, na, nb, key_type="uint32", vals=True, shape="equal", op="union", count_only=False, loop=False):
    return {"name": name, "S": S, "na": na, "nb": nb, "key_type": key_type, "vals": vals, "shape": shape, "op": op, "count_only": count_only,
            "loop": loop}


BIG = 1 << 27
ROWS = [row("1 x (2^27 + 2^27) u32 pairs, %s" % op, 1, BIG, BIG, op=op) for op in OPS] + [
    row("1 x (2^27 + 2^27) u32, intersection, count only", 1, BIG, BIG, vals=False, op="intersection", count_only=True),
    row("4096 x (32768 + 32768) u32 pairs", 4096, BIG, BIG, loop=True),
    row("65536 x (2048 + 2048) u32 pairs", 65536, BIG, BIG, loop=True),
    row("2^20 x (128 + 128) u32 pairs", 1 << 20, BIG, BIG),
    row("2^16 ragged groups, 2^26 + 2^26 u32 pairs", 1 << 16, 1 << 26, 1 << 26, shape="ragged"),
    row("2^24 segments, one of 2^26 + 2^26 u32 pairs", 1 << 24, 1 << 26, 1 << 26, shape="one"),
    row("4096 x (32768 + 32768) u32 keys", 4096, BIG, BIG, vals=False),
    row("4096 x (32768 + 32768) u64 pairs", 4096, BIG, BIG, key_type="uint64"),
    row("64 x (16384 + 16384) u32 pairs", 64, 1 << 20, 1 << 20, loop=True),
]
QUICK_ROWS = [
    row("quick 1 x (2^18 + 2^18) u32 pairs, difference", 1, 1 << 18, 1 << 18, op="difference", loop=True),
    row("quick 2^12 ragged groups u64 keys", 1 << 12, 1 << 18, 1 << 17, key_type="uint64", vals=False, shape="ragged", loop=True),
    row("quick 2^16 segments, one non-empty", 1 << 16, 1 << 18, 1 << 18, shape="one", op="symmetric_difference"),
]
HEADER = "%-50s %24s | %24s %6s | %9s %6s | %10s %7s" % ("row", "batch (min .. max)", "floor (min .. max)", "b/f", "merge", "b/m", "loop", "l/b")
LOOP_REPS_ABOVE = 4096


def timed(torch, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(times):
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def make_side(torch, r, n, gen):
    """(keys sorted per segment, offsets as a device int32 tensor of S + 1 words)."""
    S, dtype = r["S"], torch.int32 if r["key_type"] == "uint32" else torch.int64
    if r["shape"] == "equal":
        seg = torch.arange(n, device="cuda", dtype=torch.int64) // (n // S)
    elif r["shape"] == "ragged":
        seg = torch.randint(0, S, (n,), generator=gen, device="cuda", dtype=torch.int64).sort().values
    else:  # one non-empty segment in the middle
        seg = torch.full((n,), S // 2, device="cuda", dtype=torch.int64)
    per = n if r["shape"] == "one" else max(1, n // S)
    keys = torch.randint(0, max(2, int(1.44 * per)), (n,), generator=gen, device="cuda", dtype=torch.int64)
    keys = ((seg << 32) | keys).sort().values & 0xFFFFFFFF  # sorted inside every segment
    offsets = torch.searchsorted(seg, torch.arange(S + 1, device="cuda", dtype=torch.int64)).to(torch.int32)
    return keys.to(dtype), offsets


def measure(torch, G, stream, r, reps):
    S, na, nb, key_type, op = r["S"], r["na"], r["nb"], r["key_type"], r["op"]
    with_vals, with_arrays = r["vals"] and not r["count_only"], not r["count_only"]
    total = na + nb
    gen = torch.Generator(device="cuda").manual_seed(total % 1000 + S % 977)
    a, ao = make_side(torch, r, na, gen)
    b, bo = make_side(torch, r, nb, gen)
    av = torch.arange(na, dtype=torch.int32, device="cuda") if with_vals else None
    bv = torch.arange(nb, dtype=torch.int32, device="cuda") + (-2 ** 31) if with_vals else None  # (the bits of iota + 2^31)
    out_k = torch.zeros(total, dtype=a.dtype, device="cuda") if with_arrays else None
    out_v = torch.zeros(total, dtype=torch.int32, device="cuda") if with_vals else None
    out_o = torch.empty(S + 1, dtype=torch.int32, device="cuda")
    out_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    kb = a.element_size()
    b_vals = bv if op in ("union", "symmetric_difference") else None

    # the floor's inputs: the same keys sorted as a whole; the batched merge's outputs
    fa, fb = a.sort().values, b.sort().values
    floor_k = torch.zeros_like(out_k) if with_arrays else None
    floor_v = torch.zeros_like(out_v) if with_vals else None
    floor_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    merge_k = torch.empty(total, dtype=a.dtype, device="cuda")
    merge_v = torch.empty(total, dtype=torch.int32, device="cuda") if with_vals else None
    torch.cuda.empty_cache()

    sets, single, merge = G.SetOps(), G.SetOps(), G.Merge()
    sets.prepare_batch(total, S, key_type)
    single.prepare(total, key_type)
    merge.prepare_batch(total, key_type)
    batch = lambda: sets.run_batch_offsets_ptr(op, ptr(a), ptr(av), ptr(ao), na, ptr(b), ptr(b_vals), ptr(bo), nb, S, ptr(out_k), ptr(out_v),  # noqa: E731
                                               total, ptr(out_n), ptr(out_o), key_type, stream)
    floor = lambda: single.run_ptr(op, ptr(fa), ptr(av), na, ptr(fb), ptr(b_vals), nb, ptr(floor_k), ptr(floor_v), total, ptr(floor_n),  # noqa: E731
                                   key_type, stream)
    merged = lambda: merge.run_batch_offsets_ptr(ptr(a), ptr(av), ptr(ao), na, ptr(b), ptr(bv), ptr(bo), nb, S, ptr(merge_k), ptr(merge_v),  # noqa: E731
                                                 None, key_type, stream)
    tb, tf, tm = [], [], []
    for rep in range(reps + 3):
        x, y, z = timed(torch, batch), timed(torch, floor), timed(torch, merged)
        if rep >= 3:
            tb.append(x)
            tf.append(y)
            tm.append(z)
    assert sets.last() == G.plan_set_ops_batch(na, nb, S, key_type, with_arrays, True)[1:3]
    res = {"batch": stats(tb), "floor": stats(tf), "merge": float(np.median(tm))}
    kept = int(out_n.cpu().numpy().view(np.uint32)[0])
    assert int(out_o[-1].cpu().numpy().view(np.uint32)) == kept and int(out_o[0]) == 0, "out_offsets[S] is not *num_out"
    if S == 1:  # the floor is the same call
        assert kept == int(floor_n.cpu().numpy().view(np.uint32)[0]), "one segment: num_out differs from the single call's"
        if with_arrays:
            assert torch.equal(out_k, floor_k), "one segment: the keys differ from the single call's"
        if with_vals:
            assert torch.equal(out_v, floor_v), "one segment: the values differ from the single call's"
    del fa, fb, floor_k, floor_v, merge_k, merge_v
    torch.cuda.empty_cache()

    # the four cardinalities, by counting calls with out_offsets
    card = {}
    for o in OPS:
        sets.run_batch_offsets_ptr(o, ptr(a), None, ptr(ao), na, ptr(b), None, ptr(bo), nb, S, None, None, 0, ptr(out_n), ptr(out_o), key_type, stream)
        card[o] = int(out_n.cpu().numpy().view(np.uint32)[0])
        assert int(out_o[-1].cpu().numpy().view(np.uint32)) == card[o]
    assert card[op] == kept, "the counting call and the writing call disagree"
    assert card["union"] + card["intersection"] == total and card["difference"] == na - card["intersection"]
    assert card["symmetric_difference"] == card["union"] - card["intersection"]
    res["kept"] = kept

    # the loop of single calls, over the non-empty segments
    res["loop"] = None
    if r["loop"]:
        hao, hbo = ao.cpu().numpy().astype(np.int64), bo.cpu().numpy().astype(np.int64)
        live = np.flatnonzero((np.diff(hao) + np.diff(hbo)) > 0)
        calls = [(int(hao[s]), int(hao[s + 1] - hao[s]), int(hbo[s]), int(hbo[s + 1] - hbo[s])) for s in live]
        # (where a segment's result starts is known only on the device: the loop writes every segment at its MERGED offset, which
        # is what a caller without the batched call could do; the keys are compared segment by segment)
        loop_k = torch.zeros(total, dtype=a.dtype, device="cuda") if with_arrays else None
        loop_v = torch.zeros(total, dtype=torch.int32, device="cuda") if with_vals else None
        loop_n = torch.zeros(S, dtype=torch.int32, device="cuda")

        def loop():
            for i, (a0, la, b0, lb) in enumerate(calls):
                o = a0 + b0
                single.run_ptr(op, ptr(a) + kb * a0, ptr(av) + 4 * a0 if with_vals else None, la, ptr(b) + kb * b0,
                               ptr(b_vals) + 4 * b0 if b_vals is not None else None, lb, ptr(loop_k) + kb * o if with_arrays else None,
                               ptr(loop_v) + 4 * o if with_vals else None, la + lb, ptr(loop_n) + 4 * int(live[i]), key_type, stream)

        if len(calls) > LOOP_REPS_ABOVE:
            timed(torch, loop)
            res["loop"] = timed(torch, loop)
        else:
            res["loop"] = float(np.median([timed(torch, loop) for _ in range(reps + 3)][3:]))
        batch()  # (out_offsets was overwritten by the counting calls)
        torch.cuda.synchronize()
        counts = loop_n.cpu().numpy().view(np.uint32).astype(np.int64)
        offs = out_o.cpu().numpy().view(np.uint32).astype(np.int64)
        assert (np.diff(offs) == counts).all(), "the loop's counts differ from the batched call's out_offsets"
        if with_arrays:
            merged_at = hao + hbo
            idx = torch.from_numpy(np.repeat(merged_at[:-1] - offs[:-1], counts) + np.arange(int(counts.sum()))).cuda()
            assert torch.equal(loop_k[idx], out_k[:kept]), "the loop's keys differ from the batched call's"
            if with_vals:
                assert torch.equal(loop_v[idx], out_v[:kept]), "the loop's values differ from the batched call's"
    return res


def run_row(name, reps):
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU (no CPU fallback)"
    torch.cuda.init()  # (torch first: INTEGRATION.md section 3)
    import glu_hip as G

    r = next(x for x in ROWS + QUICK_ROWS if x["name"] == name)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        res = measure(torch, G, side.cuda_stream, r, reps)
        side.synchronize()
    b, f = res["batch"], res["floor"]
    loop = ("%10.3f %7.1f" % (res["loop"], res["loop"] / b[0])) if res["loop"] is not None else "%10s %7s" % ("-", "-")
    print("%-50s %8.4f (%6.4f .. %6.4f) | %8.4f (%6.4f .. %6.4f) %6.3f | %9.4f %6.3f | %s   kept %d" % (
        name, b[0], b[1], b[2], f[0], f[1], f[2], b[0] / f[0], res["merge"], b[0] / res["merge"], loop, res["kept"]))
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
    table = [r for r in (QUICK_ROWS if args.quick else ROWS) if args.only is None or args.only in r["name"]]
    print("# device events, 3 warm-up + %d repetitions (batch, floor and merge alternate), median (min .. max); ms; rows without an "
          "operation in their name are unions" % args.reps)
    print(HEADER)
    sys.stdout.flush()
    for r in table:
        # a fresh child per row, under its own time limit; a row that fails, dies or runs out of time ends the ladder
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", r["name"], "--reps", str(args.reps)], timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("# %s: no result within %d s; the ladder stops here" % (r["name"], args.timeout))
            return 124
        if p.returncode != 0:
            print("# %s: exit status %d; the ladder stops here" % (r["name"], p.returncode))
            return p.returncode if p.returncode > 0 else 1
    print("# floor: glu_set_ops_run_ptr over the same totals, both arrays sorted as a whole; merge: glu_merge_run_batch_offsets_ptr of the "
          "same inputs; loop: glu_set_ops_run_ptr per non-empty segment (timed once above %d calls)" % LOOP_REPS_ABOVE)
    return 0


if __name__ == "__main__":
    sys.exit(main())
