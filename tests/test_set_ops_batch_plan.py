"""CPU tests of the host half of the batched set operations: the four entry points are declared, exported and bound;
glu_set_ops_plan_batch (a pure function: no device needed) against a restatement of the header's formulas and against the single
plan's tile; the limits num_segments <= 2^24 and a_total + b_total <= 2^32 - 1; the C++ surface compiles; the build knows the new
headers; the new kernels use no scratch memory and no more LDS than the merge tile kernel; the existing kernels of merge, the batched
merge and the single set operations are still built."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["glu_set_ops_prepare_batch", "glu_set_ops_run_batch_offsets_ptr", "glu_set_ops_run_batch_ptr", "glu_set_ops_plan_batch"]
KEY_TYPES = ["uint32", "int32", "float32", "uint64", "int64", "float64"]
THREADS = 256
ITEMS = {4: 11, 8: 7}  # (merge_path.hpp: merge_items)
LIMIT = 2 ** 32 - 1
MAX_SEGMENTS = 2 ** 24


def restated(total, num_segments, key_bytes, with_arrays, with_offsets):
    """The header's rule: merge's tile; bounds, count and scan, the offsets kernel where out_offsets is given and the write kernel where
    something can be written; the scan and the offsets kernel where there are no keys; the scan alone where there are no segments.
    16 bytes a boundary, 4 a tile, and 4 per thread and tile unless the call only counts and has no out_offsets."""
    tile = THREADS * ITEMS[key_bytes]
    tiles = -(-total // tile)
    if not num_segments:
        kernels = 1
    elif not tiles:
        kernels = 1 + with_offsets
    else:
        kernels = 3 + with_offsets + with_arrays
    scratch = ((tiles + 1) * 16 + tiles * 4 + (tiles * THREADS * 4 if with_arrays or with_offsets else 0)) if tiles else 0
    return tile, tiles, kernels, scratch


def test_the_four_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in bound, name
    for method in ("prepare_batch", "run_batch_ptr", "run_batch_offsets_ptr"):
        assert callable(getattr(built.SetOps, method))
    assert callable(built.plan_set_ops_batch)


@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_the_plan_follows_the_restated_rule_and_the_single_plans_tile(built, key_type):
    key_bytes = 8 if key_type.endswith("64") else 4
    T = THREADS * ITEMS[key_bytes]
    for total in (0, 1, T - 1, T, T + 1, 257 * T + 9, 2 ** 28, LIMIT):
        for num_segments in (0, 1, 37, 2 ** 20, MAX_SEGMENTS):
            for with_arrays in (True, False):
                for with_offsets in (True, False):
                    a_total = total // 3
                    got = built.plan_set_ops_batch(a_total, total - a_total, num_segments, key_type, with_arrays, with_offsets)
                    assert got == restated(total, num_segments, key_bytes, with_arrays, with_offsets), (total, num_segments, with_arrays, with_offsets)
                    assert got[0] == built.plan_set_ops(1, 1, key_type)[0] == built.plan_merge(1, 1, key_type)[0]
                    if total:
                        assert got[1] == built.plan_set_ops(total, 0, key_type)[1]
    assert built.plan_set_ops_batch(0, 0, 1, key_type) == (T, 0, 2, 0)
    assert built.plan_set_ops_batch(0, 0, 0, key_type) == (T, 0, 1, 0)
    assert built.plan_set_ops_batch(T, 1, 5, key_type) == (T, 2, 5, 3 * 16 + 2 * 4 + 2 * 1024)
    assert built.plan_set_ops_batch(T, 1, 5, key_type, False, False) == (T, 2, 3, 3 * 16 + 2 * 4)
    built.check(built.lib().glu_set_ops_plan_batch(60, 40, 3, built.KEY_TYPES[key_type], 1, 1, None, None, None, None))  # any pointer may be NULL


def test_the_binding_states_the_headers_tile(built):
    """merge_path.hpp's merge_tile is what the binding reports: 2816 outputs for 4-byte keys, 1792 for 8-byte keys."""
    text = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "merge_path.hpp")).read()
    m = re.search(r"merge_items\(uint32_t key_bytes, bool[^)]*\) \{ return key_bytes == 4 \? (\d+)u : (\d+)u; \}", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (ITEMS[4], ITEMS[8])
    assert int(re.search(r"kMergeThreads = (\d+);", text).group(1)) == THREADS
    for key_type, key_bytes in (("uint32", 4), ("float32", 4), ("uint64", 8), ("int64", 8)):
        for with_arrays in (True, False):
            assert built.plan_set_ops_batch(1, 1, 1, key_type, with_arrays)[0] == THREADS * ITEMS[key_bytes] == {4: 2816, 8: 1792}[key_bytes]


def test_too_many_segments_a_total_of_two_to_the_32_and_a_bad_key_type_are_invalid_arguments(built):
    L = built.lib()
    cases = [
        (lambda: built.plan_set_ops_batch(100, 0, MAX_SEGMENTS + 1), "exceeds 2^24"),
        (lambda: built.plan_set_ops_batch(0, 0, 2 ** 32), "exceeds 2^24"),
        (lambda: built.plan_set_ops_batch(2 ** 32, 0, 1), "a_count + b_count below 2^32"),
        (lambda: built.plan_set_ops_batch(2 ** 31, 2 ** 31, 1, "float64", False), "a_count + b_count below 2^32"),
        (lambda: built.plan_set_ops_batch(1, 2 ** 64 - 1, 0), "a_count + b_count below 2^32"),
        (lambda: built.check(L.glu_set_ops_plan_batch(100, 0, 1, 6, 1, 1, None, None, None, None)), "Invalid key type"),
        (lambda: built.check(L.glu_set_ops_plan_batch(100, 0, 1, -1, 1, 1, None, None, None, None)), "Invalid key type"),
    ]
    for call, message in cases:
        with pytest.raises(built.GluError) as e:
            call()
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert message in e.value.message, e.value.message


def test_the_calls_fail_loudly_without_a_device_or_an_object(built):
    import torch

    want = built.GLU_ERROR_INVALID_ARGUMENT if torch.cuda.is_available() else built.GLU_ERROR_NO_DEVICE
    L = built.lib()
    calls = [
        lambda: L.glu_set_ops_run_batch_offsets_ptr(None, 0, None, None, None, 64, None, None, None, 64, 1, None, None, 0, None, None, 0, None),
        lambda: L.glu_set_ops_run_batch_ptr(None, 0, None, None, 8, None, None, 8, 8, None, None, 0, None, None, 0, None),
        lambda: L.glu_set_ops_prepare_batch(None, 64, 1, 0),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want
        assert e.value.message


def test_the_cpp_surface_compiles(tmp_path):
    src = tmp_path / "set_ops_batch_tu.cpp"
    src.write_text('#include "glu/SetOps.hpp"\n'
                   "void f(glu::SetOps& m, const double* a, const double* b, const uint32_t* av, const uint32_t* bv, const uint32_t* ao,\n"
                   "       const uint32_t* bo, double* out, uint32_t* ov, uint32_t* oo, uint32_t* n, void* stream)\n"
                   "{\n"
                   "    m.prepare_batch(70500, 37, GLU_KEY_FLOAT64);\n"
                   "    m.set_op_batch_offsets(GLU_SET_UNION, a, av, ao, 70000, b, bv, bo, 500, 37, out, ov, 70500, n, oo, GLU_KEY_FLOAT64, stream);\n"
                   "    m.set_op_batch_offsets(GLU_SET_INTERSECTION, a, nullptr, ao, 70000, b, nullptr, bo, 500, 37, nullptr, nullptr, 0, n);\n"
                   "    m.set_op_batch(GLU_SET_DIFFERENCE, a, av, 700, b, nullptr, 5, 100, out, ov, 70000, n, oo, GLU_KEY_FLOAT64, stream);\n"
                   "    m.set_op_batch(GLU_SET_SYMMETRIC_DIFFERENCE, a, nullptr, 700, b, nullptr, 0, 100, out, nullptr, 70000, n);\n"
                   "    glu::SetOps::Plan p = glu::SetOps::plan_batch(70000, 500, 37, GLU_KEY_FLOAT64, false, true);\n"
                   "    (void) p.tile; (void) p.tiles; (void) p.kernels; (void) p.scratch_bytes;\n"
                   "}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "gl-radix-sort_amd"), str(src)])


def test_the_library_makefile_knows_the_new_headers():
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    kernel_headers = re.search(r"KERNEL_HEADERS :=(.*?)\nHOST_HEADERS", mk, re.S).group(1).split()
    assert "set_ops_batch_kernels.hpp" in kernel_headers and "set_ops_batch_path.hpp" in kernel_headers


def resources():
    log = os.path.join(ROOT, "gl-radix-sort_amd", "lib", "kernel_resources.log")
    assert os.path.exists(log), "the library's Makefile writes the log beside the library"
    seen, cur = {}, None
    for line in open(log).read().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            seen.setdefault(cur, {})
            continue
        for field, pattern in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("vgprs", r" VGPRs: (\d+)")):
            m = re.search(pattern, line)
            if m and cur:
                seen[cur][field] = int(m.group(1))
    return seen


def test_the_new_kernels_are_built_for_both_key_widths_without_scratch(built):
    """lib/kernel_resources.log of this build: bounds, count and offsets kernels for 4- and 8-byte keys and the write kernel for both
    widths with and without values: none with scratch memory, none with more LDS than the merge tile kernel of its key width, all with
    registers left for five waves to the SIMD (512 / 5 = 102)."""
    seen = resources()
    ours = {k: v for k, v in seen.items() if re.search(r"set_batch_\w+_kernelI", k)}
    assert len(ours) == 10 and all(v["scratch"] == 0 for v in ours.values()), ours
    for k in "jm":
        merge_lds = next(v["lds"] for n, v in seen.items() if re.search(r"7glu_hip17merge_tile_kernelI%sLb1E" % k, n))
        for kernel in ("bounds", "count", "offsets"):
            name = next((n for n in ours if re.search(r"set_batch_%s_kernelI%sE" % (kernel, k), n)), None)
            assert name and ours[name]["lds"] <= merge_lds and ours[name]["vgprs"] <= 102, (kernel, k, name and ours[name])
        for vals in "01":
            name = next((n for n in ours if re.search(r"set_batch_write_kernelI%sLb%sE" % (k, vals), n)), None)
            assert name and ours[name]["lds"] <= merge_lds <= 32768 and ours[name]["vgprs"] <= 102, (k, vals, name and ours[name])


def test_the_kernels_of_merge_the_batched_merge_and_the_single_set_operations_are_still_built(built):
    seen = resources()
    for kernel, count in (("merge_partition_kernel", 2), ("merge_tile_kernel", 4), ("merge_batch_partition_kernel", 2), ("merge_batch_tile_kernel", 4),
                          ("set_ops_bounds_kernel", 2), ("set_ops_count_kernel", 2), ("set_ops_write_kernel", 4)):
        names = [n for n in seen if re.search(r"7glu_hip\d+%sI" % kernel, n)]
        assert len(names) == count and all(seen[n]["scratch"] == 0 for n in names), (kernel, names)
