"""CPU tests of the host half of expand: the six entry points are declared, exported and bound; glu_expand_plan (a pure function: no
device needed) against a restatement; the limits; the C++ header compiles alone and beside its siblings; without a device the calls
fail loudly (run_ptr reports its argument errors only once the device is entered, as merge does: tests/test_gpu_expand.py holds
them); the build knows the new unit, and its kernels use no scratch memory and at most 32 KiB of LDS."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["glu_expand_create", "glu_expand_destroy", "glu_expand_prepare", "glu_expand_run_ptr", "glu_expand_plan", "glu_expand_last"]
LIMIT = 2 ** 32 - 1
MAX_SEGMENTS = 2 ** 24


def header_tile():
    text = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "expand_path.hpp")).read()
    threads = int(re.search(r"kExpandThreads = (\d+);", text).group(1))
    items = int(re.search(r"kExpandItems = (\d+);", text).group(1))
    assert threads == 256 and items % 2 == 1  # neighbouring lanes scan an odd number of words apart
    return threads * items


def restated(total, num_segments):
    """The header's rule: the merged sequence has M = num_segments + 1 + total items; tiles = ceil(M / tile), two kernels and a split
    table of (tiles + 1) words; nothing where there is no element or no segment."""
    tile = header_tile()
    if not total or not num_segments:
        return tile, 0, 0, 0
    tiles = -(-(num_segments + 1 + total) // tile)
    return tile, tiles, 2, (tiles + 1) * 4


def test_the_six_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in bound, name
    for method in ("prepare", "run_ptr", "last", "destroy"):
        assert callable(getattr(built.Expand, method))
    assert callable(built.plan_expand)
    # every entry is marked as the library's own
    raw = open(os.path.join(ROOT, "include", "glu_hip.h")).read()
    for name in SYMBOLS:
        before = raw[:raw.index("GLU_API glu_status %s(" % name)]
        assert before[before.rindex("/*"):].startswith("/* Not in the reference"), name


def test_the_plan_follows_the_restated_rule(built):
    T = header_tile()
    totals = [0, 1, 5, T - 2, T - 1, T, T + 1, 2 * T, 3 * T + 17, 257 * T + 9, 2 ** 20, 2 ** 28]
    segments = [0, 1, 2, T - 2, T - 1, T, 3 * T + 5, 2 ** 16, MAX_SEGMENTS]
    for total in totals:
        for n in segments:
            assert built.plan_expand(total, n) == restated(total, n), (total, n)
    for total, n in ((LIMIT - 2, 1), (LIMIT - MAX_SEGMENTS - 1, MAX_SEGMENTS), (2 ** 31, 2 ** 20)):
        assert built.plan_expand(total, n) == restated(total, n), (total, n)
    assert built.plan_expand(1, 1) == (T, 1, 2, 8)
    assert built.plan_expand(T - 2, 1) == (T, 1, 2, 8)  # M == T
    assert built.plan_expand(T - 1, 1) == (T, 2, 2, 12)  # M == T + 1
    built.check(built.lib().glu_expand_plan(100, 100, None, None, None, None))  # any pointer may be NULL


def test_the_limits_are_invalid_arguments_that_name_the_argument(built):
    cases = [
        (lambda: built.plan_expand(100, MAX_SEGMENTS + 1), "num_segments"),
        (lambda: built.plan_expand(0, 2 ** 40), "num_segments"),
        (lambda: built.plan_expand(2 ** 32, 1), "total"),
        (lambda: built.plan_expand(LIMIT - 1, 1), "total + num_segments + 1"),
        (lambda: built.plan_expand(LIMIT - MAX_SEGMENTS, MAX_SEGMENTS), "total + num_segments + 1"),
        (lambda: built.plan_expand(2 ** 64 - 1, 2), "total"),  # (the sum of the two size_t's wraps)
    ]
    for call, message in cases:
        with pytest.raises(built.GluError) as e:
            call()
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert message in e.value.message, e.value.message


def test_the_calls_fail_loudly_without_a_device_or_an_object(built):
    """No device: every call that would touch one says so (GLU_ERROR_NO_DEVICE, through GluError) before it looks at its
    arguments.  With a device the same calls, given no object, are invalid arguments."""
    import torch

    want = built.GLU_ERROR_INVALID_ARGUMENT if torch.cuda.is_available() else built.GLU_ERROR_NO_DEVICE
    L = built.lib()
    calls = [
        lambda: L.glu_expand_run_ptr(None, None, 64, 64, None, 4, None, None, None, None),
        lambda: L.glu_expand_prepare(None, 64, 64),
        lambda: L.glu_expand_last(None, None, None),
        lambda: L.glu_expand_create(None),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want
        assert e.value.message
    if not torch.cuda.is_available():
        with pytest.raises(built.GluError) as e:
            built.Expand()
        assert e.value.status == built.GLU_ERROR_NO_DEVICE
        assert "no CPU fallback" in e.value.message


def syntax_only(*args):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + list(args))


def test_the_cpp_header_compiles_alone_and_beside_its_siblings(tmp_path):
    includes = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gl-radix-sort_amd")]
    alone = tmp_path / "expand_alone.cpp"
    alone.write_text('#include "glu/Expand.hpp"\nint main() { return 0; }\n')
    syntax_only(*includes, str(alone))
    src = tmp_path / "expand_tu.cpp"
    src.write_text('#include "glu/Expand.hpp"\n'
                   '#include "glu/Histogram.hpp"\n'
                   '#include "glu/Merge.hpp"\n'
                   '#include "glu/SortedSearch.hpp"\n'
                   '#include "glu/Select.hpp"\n'
                   '#include "glu/KeyRuns.hpp"\n'
                   '#include "glu/Reduce.hpp"\n'
                   '#include "glu/BlellochScan.hpp"\n'
                   '#include "glu/RadixSort.hpp"\n'
                   "void f(glu::Expand& e, const uint32_t* offsets, const double* items, double* out, uint32_t* seg, uint32_t* rank,\n"
                   "       glu::ShaderStorageBuffer& x, glu::ShaderStorageBuffer& y, glu::ShaderStorageBuffer& z, void* stream)\n"
                   "{\n"
                   "    e.prepare(70500, 300);\n"
                   "    e(offsets, 300, 70500, items, 8, out, seg, rank, stream);\n"
                   "    e(offsets, 300, 70500, nullptr, 0, nullptr, seg, nullptr);\n"
                   "    e(x, 300, 70500, y, z);\n"
                   "    e.segment_ids(offsets, 300, 70500, seg, stream);\n"
                   "    e.ranks(offsets, 300, 70500, rank);\n"
                   "    e.gather(offsets, 300, 70500, items, 8, out, stream);\n"
                   "    glu::Expand::Plan p = glu::Expand::plan(70500, 300);\n"
                   "    (void) p.tile; (void) p.tiles; (void) p.kernels; (void) p.scratch_bytes;\n"
                   "    glu::Expand::Last l = e.last();\n"
                   "    (void) l.tiles; (void) l.kernels;\n"
                   "}\n"
                   "int main() { return 0; }\n")
    syntax_only(*includes, str(src))


def test_the_standalone_header_is_generated_and_compiles(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dist.py"), str(tmp_path)])
    assert os.path.exists(tmp_path / "Expand.hpp")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "Expand.hpp"\n#include "Histogram.hpp"\n#include "Merge.hpp"\n#include "KeyRuns.hpp"\n#include "Reduce.hpp"\n'
                  '#include "BlellochScan.hpp"\n#include "RadixSort.hpp"\n'
                  "int main() { return glu::Expand::plan(0, 0).tiles; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", str(tmp_path), str(tu)])
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "$(DIST)/Expand.hpp" in mk


def test_the_library_makefile_and_the_build_know_the_new_unit():
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "glu_expand" in mk and "expand_kernels.hpp" in mk and "expand_path.hpp" in mk and "glu_expand_object.hpp" in mk


def test_the_expand_kernels_are_built_without_scratch(built):
    """lib/kernel_resources.log of this build: the partition kernel and the tile kernel for no items and for items of 1, 2, 4 and 8
    words, none with scratch memory, the tile kernels with the slice and the marks in at most 32 KiB of LDS."""
    log = os.path.join(ROOT, "gl-radix-sort_amd", "lib", "kernel_resources.log")
    assert os.path.exists(log), "the library's Makefile writes the log beside the library"
    scratch, lds, cur = {}, {}, None
    for line in open(log).read().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and cur:
            lds[cur] = int(m.group(1))
    ours = {k: v for k, v in scratch.items() if "expand_partition_kernel" in k or "expand_tile_kernel" in k}
    assert any("expand_partition_kernel" in name for name in ours)
    T = header_tile()
    for words in (0, 1, 2, 4, 8):
        name = next((n for n in ours if re.search(r"expand_tile_kernelILj%dEE" % words, n)), None)
        assert name, words
        assert (2 * T + 1) * 4 <= lds[name] <= 32768, (name, lds[name])
    assert len(ours) == 6 and all(v == 0 for v in ours.values()), ours
