"""CPU tests of the batched scan's host half: the four entry points are declared, exported and bound; which class a segment takes
(glu_scan_plan_batch is a pure function: no device needed); the C++ wrappers compile; without a device the calls fail loudly."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["glu_scan_run_batch_offsets_ptr", "glu_scan_prepare_batch", "glu_scan_plan_batch", "glu_scan_read_batch"]
ELEM_BYTES = [4, 8, 16, 32]


def test_the_four_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in bound, name
    for method in ("run_batch_offsets_ptr", "prepare_batch", "read_batch"):
        assert callable(getattr(built.BlellochScan, method))
    assert callable(built.plan_scan_batch)


@pytest.mark.parametrize("elem_bytes", ELEM_BYTES)
def test_an_empty_segment_is_path_zero(built, elem_bytes):
    assert built.plan_scan_batch(0, elem_bytes) == (0, 0)
    assert built.plan_scan_batch(1, elem_bytes) == (1, 1)


@pytest.mark.parametrize("elem_bytes", ELEM_BYTES)
def test_paths_are_monotone_and_every_class_is_reached(built, elem_bytes):
    """The path never goes down as the segment grows, and neither does the number of workgroups; paths 1 and 2 use one workgroup,
    path 3 more than one, enough of them that 2^28 elements spread over a device of 256 CUs several times."""
    counts = sorted(set(list(range(0, 2100)) + [2 ** k + d for k in range(11, 33) for d in (-1, 0, 1)] + [5000, 100000, 3000001]))
    last_path, last_wg, seen = 0, 0, set()
    for count in counts:
        path, wg = built.plan_scan_batch(count, elem_bytes)
        assert path in (0, 1, 2, 3)
        assert path >= last_path, (count, path, last_path)
        assert wg >= last_wg, (count, wg, last_wg)
        if path in (1, 2):
            assert wg == 1, (count, wg)
        if path == 3:
            assert wg > 1, (count, wg)
        last_path, last_wg = path, wg
        seen.add(path)
    assert seen == {0, 1, 2, 3}
    assert built.plan_scan_batch(1 << 28, elem_bytes)[1] >= 1024


@pytest.mark.parametrize("elem_bytes", ELEM_BYTES)
def test_the_class_boundaries_are_byte_sizes(built, elem_bytes):
    """The classes are drawn in bytes: the last length of a class times the element size is the same for every element size."""
    def last_of(path, es):
        lo, hi = 0, 1 << 40  # plan(lo).path <= path < plan(hi).path
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if built.plan_scan_batch(mid, es)[0] <= path:
                lo = mid
            else:
                hi = mid
        return lo

    for path in (1, 2):
        last = last_of(path, elem_bytes)
        assert last * elem_bytes == last_of(path, 4) * 4
        assert built.plan_scan_batch(last + 1, elem_bytes)[0] == path + 1
    assert built.plan_scan_batch(last_of(2, elem_bytes) + 1, elem_bytes)[1] >= 2


def test_other_element_sizes_are_invalid_arguments(built):
    for elem_bytes in (0, 1, 2, 3, 12, 64):
        with pytest.raises(built.GluError) as e:
            built.plan_scan_batch(100, elem_bytes)
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert "elem_bytes" in e.value.message


def test_the_batched_calls_fail_loudly_without_a_device_or_an_object(built):
    """No device: every batched call that would compute says so (GLU_ERROR_NO_DEVICE, through GluError) before it looks at its
    arguments.  With a device the same calls, given no object, are invalid arguments."""
    import torch

    want = built.GLU_ERROR_INVALID_ARGUMENT if torch.cuda.is_available() else built.GLU_ERROR_NO_DEVICE
    L = built.lib()
    calls = [
        lambda: L.glu_scan_run_batch_offsets_ptr(None, None, 64, None, 4, None),
        lambda: L.glu_scan_prepare_batch(None, 64, 4),
        lambda: L.glu_scan_read_batch(None, None, None, None),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want
        assert e.value.message
    if not torch.cuda.is_available():
        with pytest.raises(built.GluError) as e:
            built.BlellochScan(built.DataType_Uint)
        assert e.value.status == built.GLU_ERROR_NO_DEVICE


def test_the_cpp_wrappers_instantiate(tmp_path):
    src = tmp_path / "scan_batch_tu.cpp"
    src.write_text('#include "glu/BlellochScan.hpp"\n'
                   "void f(glu::BlellochScan& s, float* a, const uint32_t* o)\n"
                   "{\n"
                   "    s.scan_batch_offsets(a, 700, o, 7);\n"
                   "    s.prepare_batch(700, 7);\n"
                   "    glu::BlellochScan::BatchReport b = s.read_batch();\n"
                   "    (void) b.wave_segments; (void) b.block_segments; (void) b.long_segments;\n"
                   "}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "gl-radix-sort_amd"), str(src)])


def test_the_library_makefile_and_the_build_know_the_new_unit():
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "glu_scan_batch" in mk and "scan_batch_kernels.hpp" in mk and "glu_scan_object.hpp" in mk


def test_every_new_kernel_is_built_for_all_types_without_scratch(built):
    """lib/kernel_resources.log of this build: 12 instantiations of the two new kernels, none with scratch memory."""
    log = os.path.join(ROOT, "gl-radix-sort_amd", "lib", "kernel_resources.log")
    assert os.path.exists(log), "the library's Makefile writes the log beside the library"
    kernels, cur = {}, None
    for line in open(log).read().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            kernels[cur] = int(m.group(1))
    for name in ("scan_batch_wave_kernel", "scan_batch_block_kernel"):
        mine = {k: v for k, v in kernels.items() if name in k}
        assert len(mine) == 12, (name, sorted(mine))
        assert all(v == 0 for v in mine.values()), mine
