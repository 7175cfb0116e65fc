"""Same-process A/B of the narrow hand-off: two sort objects in one process, GLU_HIP_SORT_NARROW_HANDOFF=1 and
=0, sort the same 2^28 pairs alternately; per-sort device time from events on the sort's stream.  Isolates the change from the
machine and from where a process's arrays happen to lie.

  python tools/narrow_handoff_ab.py [--log2 28] [--rounds 12] [--inputs uniform,zeros_1pct,distinct_1000,all_zero] [--one-object]

Two objects own two sets of scratch arrays, and where a sort's arrays lie moves it by a few percent: the
"zeros_1pct" rows, where neither object takes the narrow hand-off, show how much of a difference is that.  --one-object takes it out:
ONE object, prepared with the option at 1 (it owns the side array), sorts with the option switched to 1 and 0 in turn -- the same
scratch, the same caller arrays, only the hand-off differs.

Inputs besides uniform keys are the ones of profiles/r06/distributions_2p28.txt at which the narrow hand-off is NOT taken (a long run
for the segmented passes, long runs of one value, a refused sort): there the option may cost one launch that returns at once."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-radix-sort_amd"))


def draw(torch, name, n, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    if name == "all_zero":
        return torch.zeros(n, dtype=torch.int32, device="cuda:0")
    keys = torch.randint(-2**31, 2**31, (n,), dtype=torch.int32, device="cuda:0", generator=g)
    if name == "zeros_1pct":
        keys[torch.rand(n, device="cuda:0", generator=g) < 0.01] = 0
    elif name == "distinct_1000":
        pool = torch.randint(-2**31, 2**31, (1000,), dtype=torch.int32, device="cuda:0", generator=g)
        keys = pool[torch.randint(0, 1000, (n,), device="cuda:0", generator=g)]
    return keys


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--log2", type=int, default=28)
    p.add_argument("--rounds", type=int, default=12)
    p.add_argument("--inputs", default="uniform,zeros_1pct,distinct_1000,all_zero")
    p.add_argument("--one-object", action="store_true", help="one object, the option switched between sorts (same scratch arrays)")
    args = p.parse_args()
    import torch

    import glu_hip as G

    n = 1 << args.log2
    sorters = {}
    for option in (1, 0):
        s = G.RadixSort(options={"SORT_NARROW_HANDOFF": option})
        s.prepare_internal_buffers(n)
        sorters[option] = s
    if args.one_object:
        sorters[0] = sorters[1]
    print("ONE object, the option switched between sorts" if args.one_object else "TWO objects")
    print("n = 2^%d pairs, %d rounds, scratch bytes: option 1 %d, option 0 %d (difference %d = n x 2)" % (
        args.log2, args.rounds, sorters[1].scratch_size(), sorters[0].scratch_size(), sorters[1].scratch_size() - sorters[0].scratch_size()))
    stream = torch.cuda.Stream()
    vals0 = torch.arange(n, dtype=torch.int32, device="cuda:0")
    kt, vt = torch.empty_like(vals0), torch.empty_like(vals0)
    for name in args.inputs.split(","):
        keys0 = draw(torch, name, n, 20 + len(name))
        times = {1: [], 0: []}
        took = {}
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for rnd in range(args.rounds + 2):  # (two rounds of warm-up)
                for option in ((1, 0) if rnd % 2 == 0 else (0, 1)):
                    kt.copy_(keys0)
                    vt.copy_(vals0)
                    if args.one_object:
                        sorters[option].set_option("SORT_NARROW_HANDOFF", option)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    sorters[option].run_ptr(kt.data_ptr(), vt.data_ptr(), n, 0, stream.cuda_stream)
                    b.record(stream)
                    stream.synchronize()
                    if rnd >= 2:
                        times[option].append(a.elapsed_time(b))
                    took[option] = (sorters[option].read_finish(), sorters[option].read_handoff()["narrow"])
            flipped = kt ^ torch.tensor(-2**31, dtype=torch.int32, device="cuda:0")
            assert bool((flipped[1:] >= flipped[:-1]).all()), "not sorted"
        print("%-14s" % name)
        for option in (1, 0):
            t = np.array(times[option])
            fin, narrow = took[option]
            print("  option %d: median %.4f ms  min %.4f  max %.4f  (accepted %d, tile %d, narrow %d)  all: %s" % (
                option, np.median(t), t.min(), t.max(), fin["accepted"], fin["capacity"], narrow, " ".join("%.3f" % x for x in t)))
        m1, m0 = np.median(times[1]), np.median(times[0])
        print("  option 1 - option 0: median %+.4f ms (%+.2f %%), min %+.4f ms" % (m1 - m0, 100.0 * (m1 - m0) / m0, min(times[1]) - min(times[0])))
        del keys0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
