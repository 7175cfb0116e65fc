"""CPU tests of the host half of merge: the six entry points are declared, exported and bound; glu_merge_plan (a pure function: no
device needed) against a restatement; the limit a_count + b_count <= 2^32 - 1; the C++ header compiles alone and beside its
siblings; without a device the calls fail loudly; the build knows the new unit, and its kernels use no scratch memory and at most
32 KiB of LDS."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["glu_merge_create", "glu_merge_destroy", "glu_merge_prepare", "glu_merge_run_ptr", "glu_merge_plan", "glu_merge_last"]
KEY_TYPES = ["uint32", "int32", "float32", "uint64", "int64", "float64"]
THREADS = 256
ITEMS = {4: 11, 8: 7}  # outputs per thread and tile, by key width (merge_path.hpp: merge_items)
LIMIT = 2 ** 32 - 1


def restated(a_count, b_count, key_bytes):
    """The header's rule: tile = 256 x ITEMS of the key width, tiles = ceil(total / tile), two kernels unless there is nothing to
    merge, a split table of (tiles + 1) words."""
    total = a_count + b_count
    tile = THREADS * ITEMS[key_bytes]
    tiles = -(-total // tile)
    return tile, tiles, 2 if total else 0, (tiles + 1) * 4 if total else 0


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
        assert callable(getattr(built.Merge, method))
    assert callable(built.plan_merge)
    # the tile this file restates is the header's
    path = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "merge_path.hpp")).read()
    m = re.search(r"merge_items\(.*?\)\s*\{\s*return key_bytes == 4 \? (\d+)u : (\d+)u;", path)
    assert m and (int(m.group(1)), int(m.group(2))) == (ITEMS[4], ITEMS[8])
    assert int(re.search(r"kMergeThreads\s*=\s*(\d+)", path).group(1)) == THREADS
    assert all(i % 2 == 1 for i in ITEMS.values())  # neighbouring lanes start an odd number of words apart
    assert all(THREADS * i * (kb + 4) + 32 <= 32768 for kb, i in ITEMS.items())  # keys and values of a tile, a pack more of each


@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_the_plan_follows_the_restated_rule(built, key_type):
    key_bytes = 8 if key_type.endswith("64") else 4
    T = THREADS * ITEMS[key_bytes]
    counts = [0, 1, 5, T - 1, T, T + 1, 2 * T, 3 * T + 17, 257 * T + 9, 2 ** 20, 2 ** 28]
    for a_count in counts:
        for b_count in counts:
            for with_vals in (True, False):
                assert built.plan_merge(a_count, b_count, key_type, with_vals) == restated(a_count, b_count, key_bytes), (a_count, b_count)
    for a_count, b_count in ((LIMIT, 0), (0, LIMIT), (2 ** 31, 2 ** 31 - 1), (LIMIT - T, T)):
        assert built.plan_merge(a_count, b_count, key_type) == restated(a_count, b_count, key_bytes)
    assert built.plan_merge(0, 0, key_type) == (T, 0, 0, 0)
    assert built.plan_merge(1, 0, key_type) == (T, 1, 2, 8)
    built.check(built.lib().glu_merge_plan(100, 100, built.KEY_TYPES[key_type], 1, None, None, None, None))  # any pointer may be NULL


def test_a_total_of_two_to_the_32_and_a_bad_key_type_are_invalid_arguments(built):
    L = built.lib()
    cases = [
        (lambda: built.plan_merge(2 ** 31, 2 ** 31), "a_count + b_count below 2^32"),
        (lambda: built.plan_merge(2 ** 32, 0), "a_count + b_count below 2^32"),
        (lambda: built.plan_merge(0, 2 ** 32, "float64", False), "a_count + b_count below 2^32"),
        (lambda: built.plan_merge(LIMIT, 1), "a_count + b_count below 2^32"),
        (lambda: built.plan_merge(2 ** 64 - 1, 2), "a_count + b_count below 2^32"),  # (the sum of the two size_t's wraps)
        (lambda: built.check(L.glu_merge_plan(100, 100, 6, 1, None, None, None, None)), "Invalid key type"),
        (lambda: built.check(L.glu_merge_plan(100, 100, -1, 1, None, None, None, None)), "Invalid key type"),
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
        lambda: L.glu_merge_run_ptr(None, None, None, 64, None, None, 64, None, None, 0, None),
        lambda: L.glu_merge_prepare(None, 64, 0),
        lambda: L.glu_merge_last(None, None, None),
        lambda: L.glu_merge_create(None),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want
        assert e.value.message
    if not torch.cuda.is_available():
        with pytest.raises(built.GluError) as e:
            built.Merge()
        assert e.value.status == built.GLU_ERROR_NO_DEVICE
        assert "no CPU fallback" in e.value.message


def syntax_only(*args):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + list(args))


def test_the_cpp_header_compiles_alone_and_beside_its_siblings(tmp_path):
    includes = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gl-radix-sort_amd")]
    alone = tmp_path / "merge_alone.cpp"
    alone.write_text('#include "glu/Merge.hpp"\nint main() { return 0; }\n')
    syntax_only(*includes, str(alone))
    src = tmp_path / "merge_tu.cpp"
    src.write_text('#include "glu/Merge.hpp"\n'
                   '#include "glu/SortedSearch.hpp"\n'
                   '#include "glu/Select.hpp"\n'
                   '#include "glu/KeyRuns.hpp"\n'
                   '#include "glu/Reduce.hpp"\n'
                   '#include "glu/BlellochScan.hpp"\n'
                   '#include "glu/RadixSort.hpp"\n'
                   "void f(glu::Merge& m, const double* a, const double* b, const uint32_t* av, const uint32_t* bv, double* out, uint32_t* ov,\n"
                   "       glu::ShaderStorageBuffer& x, glu::ShaderStorageBuffer& y, glu::ShaderStorageBuffer& z, void* stream)\n"
                   "{\n"
                   "    m.prepare(70500, GLU_KEY_FLOAT64);\n"
                   "    m(a, av, 70000, b, bv, 500, out, ov, GLU_KEY_FLOAT64, stream);\n"
                   "    m(a, nullptr, 70000, b, nullptr, 500, out, nullptr, GLU_KEY_FLOAT64);\n"
                   "    m(x, x, 10, y, y, 20, z, z);\n"
                   "    m(x, 10, y, 20, z);\n"
                   "    glu::Merge::Plan p = glu::Merge::plan(70000, 500, GLU_KEY_FLOAT64, false);\n"
                   "    (void) p.tile; (void) p.tiles; (void) p.kernels; (void) p.scratch_bytes;\n"
                   "    glu::Merge::Last l = m.last();\n"
                   "    (void) l.tiles; (void) l.kernels;\n"
                   "}\n"
                   "int main() { return 0; }\n")
    syntax_only(*includes, str(src))


def test_the_standalone_header_is_generated_and_compiles(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dist.py"), str(tmp_path)])
    assert os.path.exists(tmp_path / "Merge.hpp")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "Merge.hpp"\n#include "SortedSearch.hpp"\n#include "Select.hpp"\n#include "KeyRuns.hpp"\n#include "Reduce.hpp"\n'
                  '#include "BlellochScan.hpp"\n#include "RadixSort.hpp"\n'
                  "int main() { return glu::Merge::plan(0, 0).tiles; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", str(tmp_path), str(tu)])
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "$(DIST)/Merge.hpp" in mk


def test_the_library_makefile_and_the_build_know_the_new_unit():
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "glu_merge" in mk and "merge_kernels.hpp" in mk and "merge_path.hpp" in mk and "glu_merge_object.hpp" in mk


def test_the_merge_kernels_are_built_for_both_key_widths_without_scratch(built):
    """lib/kernel_resources.log of this build: the partition kernel for 4- and 8-byte keys (their Itanium codes: j, m) and the tile
    kernel for both widths with and without values, none with scratch memory, the tile kernels with LDS of at most 32 KiB."""
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
    ours = {k: v for k, v in scratch.items() if "merge_partition_kernel" in k or "merge_tile_kernel" in k}
    for k in "jm":
        assert any(re.search(r"merge_partition_kernelI%sE" % k, name) for name in ours), k
        for vals in "01":
            name = next((n for n in ours if re.search(r"merge_tile_kernelI%sLb%sE" % (k, vals), n)), None)
            assert name, (k, vals)
            key_bytes = 4 if k == "j" else 8
            keys = THREADS * ITEMS[key_bytes] * key_bytes
            assert keys <= lds[name] <= 32768, (name, lds[name])
            if vals == "1":
                assert lds[name] >= keys + THREADS * ITEMS[key_bytes] * 4
    assert len(ours) == 6 and all(v == 0 for v in ours.values()), ours
