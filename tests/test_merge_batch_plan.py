"""CPU tests of the host half of the batched merge: the four entry points are declared, exported and bound; glu_merge_plan_batch (a
pure function: no device needed) against a restatement and against the single plan's tile; the limits num_segments <= 2^24 and
a_total + b_total <= 2^32 - 1; the C++ surface compiles; the build knows the new headers, and the new kernels use no scratch memory
and no more LDS than five workgroups to the CU allow."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["glu_merge_prepare_batch", "glu_merge_run_batch_offsets_ptr", "glu_merge_run_batch_ptr", "glu_merge_plan_batch"]
KEY_TYPES = ["uint32", "int32", "float32", "uint64", "int64", "float64"]
THREADS = 256
ITEMS = {4: 11, 8: 7}  # (merge_path.hpp: merge_items)
LIMIT = 2 ** 32 - 1
MAX_SEGMENTS = 2 ** 24


def restated(total, num_segments, key_bytes):
    """The header's rule: merge's tile, tiles = ceil(total / tile), the partition kernel whenever there are segments and the tile
    kernel where there are tiles, a boundary of two words per tile and one more."""
    tile = THREADS * ITEMS[key_bytes]
    tiles = -(-total // tile)
    return tile, tiles, (2 if tiles else 1) if num_segments else 0, (tiles + 1) * 8


def test_the_four_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in bound, name
    for method in ("prepare_batch", "run_batch_ptr", "run_batch_offsets_ptr"):
        assert callable(getattr(built.Merge, method))
    assert callable(built.plan_merge_batch)


@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_the_plan_follows_the_restated_rule_and_the_single_plans_tile(built, key_type):
    key_bytes = 8 if key_type.endswith("64") else 4
    T = THREADS * ITEMS[key_bytes]
    for total in (0, 1, T - 1, T, T + 1, 257 * T + 9, 2 ** 28, LIMIT):
        for num_segments in (0, 1, 37, 2 ** 20, MAX_SEGMENTS):
            for with_vals in (True, False):
                got = built.plan_merge_batch(total, num_segments, key_type, with_vals)
                assert got == restated(total, num_segments, key_bytes), (total, num_segments, with_vals)
                assert got[0] == built.plan_merge(1, 1, key_type, with_vals)[0]
                if total:
                    assert got[1] == built.plan_merge(total, 0, key_type, with_vals)[1]
    assert built.plan_merge_batch(0, 1, key_type) == (T, 0, 1, 8)
    assert built.plan_merge_batch(0, 0, key_type) == (T, 0, 0, 8)
    assert built.plan_merge_batch(T + 1, 5, key_type) == (T, 2, 2, 24)
    built.check(built.lib().glu_merge_plan_batch(100, 3, built.KEY_TYPES[key_type], 1, None, None, None, None))  # any pointer may be NULL


def test_too_many_segments_a_total_of_two_to_the_32_and_a_bad_key_type_are_invalid_arguments(built):
    L = built.lib()
    cases = [
        (lambda: built.plan_merge_batch(100, MAX_SEGMENTS + 1), "exceeds 2^24"),
        (lambda: built.plan_merge_batch(0, 2 ** 32), "exceeds 2^24"),
        (lambda: built.plan_merge_batch(2 ** 32, 1), "a_count + b_count below 2^32"),
        (lambda: built.plan_merge_batch(2 ** 32, 1, "float64", False), "a_count + b_count below 2^32"),
        (lambda: built.plan_merge_batch(2 ** 64 - 1, 0), "a_count + b_count below 2^32"),
        (lambda: built.check(L.glu_merge_plan_batch(100, 1, 6, 1, None, None, None, None)), "Invalid key type"),
        (lambda: built.check(L.glu_merge_plan_batch(100, 1, -1, 1, None, None, None, None)), "Invalid key type"),
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
        lambda: L.glu_merge_run_batch_offsets_ptr(None, None, None, None, 64, None, None, None, 64, 1, None, None, None, 0, None),
        lambda: L.glu_merge_run_batch_ptr(None, None, None, 8, None, None, 8, 8, None, None, None, 0, None),
        lambda: L.glu_merge_prepare_batch(None, 64, 0),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want
        assert e.value.message


def test_the_cpp_surface_compiles(tmp_path):
    src = tmp_path / "merge_batch_tu.cpp"
    src.write_text('#include "glu/Merge.hpp"\n'
                   "void f(glu::Merge& m, const double* a, const double* b, const uint32_t* av, const uint32_t* bv, const uint32_t* ao,\n"
                   "       const uint32_t* bo, double* out, uint32_t* ov, uint32_t* oo, void* stream)\n"
                   "{\n"
                   "    m.prepare_batch(70500, GLU_KEY_FLOAT64);\n"
                   "    m.merge_batch_offsets(a, av, ao, 70000, b, bv, bo, 500, 37, out, ov, oo, GLU_KEY_FLOAT64, stream);\n"
                   "    m.merge_batch_offsets(a, nullptr, ao, 70000, b, nullptr, bo, 500, 37, out, nullptr);\n"
                   "    m.merge_batch(a, av, 700, b, bv, 5, 100, out, ov, oo, GLU_KEY_FLOAT64, stream);\n"
                   "    m.merge_batch(a, nullptr, 700, b, nullptr, 0, 100, out, nullptr);\n"
                   "    glu::Merge::Plan p = glu::Merge::plan_batch(70500, 37, GLU_KEY_FLOAT64, false);\n"
                   "    (void) p.tile; (void) p.tiles; (void) p.kernels; (void) p.scratch_bytes;\n"
                   "}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "gl-radix-sort_amd"), str(src)])


def test_the_library_makefile_knows_the_new_headers():
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "merge_batch_kernels.hpp" in mk and "merge_batch_path.hpp" in mk


def test_the_new_kernels_are_built_for_both_key_widths_without_scratch(built):
    """lib/kernel_resources.log of this build: the batched partition kernel for 4- and 8-byte keys and the batched tile kernel for both
    widths with and without values, none with scratch memory, the tile kernels with no more than 32 KiB of LDS (five workgroups to the
    CU) and enough registers left for five waves to the SIMD (512 / 5 = 102)."""
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
    ours = {k: v for k, v in seen.items() if "merge_batch_partition_kernel" in k or "merge_batch_tile_kernel" in k}
    assert len(ours) == 6 and all(v["scratch"] == 0 for v in ours.values()), ours
    for k in "jm":
        assert any(re.search(r"merge_batch_partition_kernelI%sE" % k, name) for name in ours), k
        for vals in "01":
            name = next((n for n in ours if re.search(r"merge_batch_tile_kernelI%sLb%sE" % (k, vals), n)), None)
            assert name, (k, vals)
            key_bytes = 4 if k == "j" else 8
            tile = THREADS * ITEMS[key_bytes]
            assert tile * (key_bytes + 4) <= ours[name]["lds"] <= 32768, (name, ours[name])
            assert ours[name]["vgprs"] <= 102, (name, ours[name])
