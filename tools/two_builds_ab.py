"""Same-process A/B of two BUILDS of the library (the shape of tools/narrow_handoff_ab.py, which alternates an option): both
libglu_hip.so files are loaded into one process, one sort object each, and the two objects sort the same pairs in the same caller
arrays alternately; per-sort device time from events on the sort's stream.  Takes the machine and where the caller's arrays lie out
of the comparison; each object still owns its own scratch arrays.

  python tools/two_builds_ab.py --lib-a PARENT/libglu_hip.so --lib-b gl-radix-sort_amd/lib/libglu_hip.so [--log2 28] [--rounds 12]

Prints every time, medians, and b - a."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gl-radix-sort_amd", "glu_hip")


def load(alias, lib_path):
    """The Python binding once more under another module name, bound to the library at lib_path."""
    os.environ["GLU_HIP_LIB_PATH"] = os.path.abspath(lib_path)
    spec = importlib.util.spec_from_file_location(alias, os.path.join(PKG, "__init__.py"), submodule_search_locations=[PKG])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[alias] = mod
    spec.loader.exec_module(mod)
    mod.lib()
    del os.environ["GLU_HIP_LIB_PATH"]
    return mod


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lib-a", required=True)
    p.add_argument("--lib-b", required=True)
    p.add_argument("--log2", type=int, default=28)
    p.add_argument("--rounds", type=int, default=12)
    args = p.parse_args()
    import torch

    n = 1 << args.log2
    builds = {"a": load("glu_hip_a", args.lib_a), "b": load("glu_hip_b", args.lib_b)}
    sorters = {}
    for name, G in builds.items():
        sorters[name] = G.RadixSort()
        sorters[name].prepare_internal_buffers(n)
        print("%s: %s  %s" % (name, G.LIB_PATH, G.lib().glu_version().decode()))
    g = torch.Generator(device="cuda:0")
    g.manual_seed(28)
    keys0 = torch.randint(-2**31, 2**31, (n,), dtype=torch.int32, device="cuda:0", generator=g)
    vals0 = torch.arange(n, dtype=torch.int32, device="cuda:0")
    kt, vt = torch.empty_like(vals0), torch.empty_like(vals0)
    stream = torch.cuda.Stream()
    times, outs = {"a": [], "b": []}, {}
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for rnd in range(args.rounds + 2):  # (two rounds of warm-up)
            for name in (("a", "b") if rnd % 2 == 0 else ("b", "a")):
                kt.copy_(keys0)
                vt.copy_(vals0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                sorters[name].run_ptr(kt.data_ptr(), vt.data_ptr(), n, 0, stream.cuda_stream)
                b.record(stream)
                stream.synchronize()
                if rnd >= 2:
                    times[name].append(a.elapsed_time(b))
                if rnd == 0:
                    outs[name] = (kt.clone(), vt.clone(), sorters[name].read_finish())
    assert bool((outs["a"][0] == outs["b"][0]).all()) and bool((outs["a"][1] == outs["b"][1]).all()), "the two builds' outputs differ"
    print("n = 2^%d pairs, %d rounds; outputs of the two builds identical" % (args.log2, args.rounds))
    for name in ("a", "b"):
        t = np.array(times[name])
        print("  %s: median %.4f ms  min %.4f  max %.4f  %s  all: %s" % (name, np.median(t), t.min(), t.max(), outs[name][2],
                                                                      " ".join("%.3f" % x for x in t)))
    ma, mb = np.median(times["a"]), np.median(times["b"])
    print("  b - a: median %+.4f ms (%+.2f %%), min %+.4f ms" % (mb - ma, 100.0 * (mb - ma) / ma, min(times["b"]) - min(times["a"])))


if __name__ == "__main__":
    main()
