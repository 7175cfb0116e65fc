"""CPU tests of the batched reduce's host half: the five entry points are declared, exported and bound; which class a segment
takes (glu_reduce_plan_batch is a pure function: no device needed); the C++ wrappers compile; without a device the calls fail
loudly."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["glu_reduce_run_batch_ptr", "glu_reduce_run_batch_offsets_ptr", "glu_reduce_prepare_batch", "glu_reduce_plan_batch",
           "glu_reduce_read_batch"]
ELEM_BYTES = [4, 8, 16, 32]


def test_the_five_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in bound, name
    for method in ("run_batch_ptr", "run_batch_offsets_ptr", "prepare_batch", "read_batch"):
        assert callable(getattr(built.Reduce, method))
    assert callable(built.plan_reduce_batch)


def test_the_header_states_that_data_is_read_only(built):
    text = open(os.path.join(ROOT, "include", "glu_hip.h")).read()
    section = text[text.index("---- batched reduce"):]
    assert "READ ONLY" in section and "must not overlap" in section and "identity" in section


@pytest.mark.parametrize("elem_bytes", ELEM_BYTES)
def test_an_empty_segment_is_path_zero(built, elem_bytes):
    assert built.plan_reduce_batch(0, elem_bytes) == (0, 0)
    assert built.plan_reduce_batch(1, elem_bytes) == (1, 1)


@pytest.mark.parametrize("elem_bytes", ELEM_BYTES)
def test_paths_are_monotone_and_every_class_is_reached(built, elem_bytes):
    """The path never goes down as the segment grows, and neither does the number of workgroups; paths 1 and 2 use one workgroup,
    path 3 more than one, enough of them that 2^28 elements spread over a device of 256 CUs several times."""
    counts = sorted(set(list(range(0, 2100)) + [2 ** k + d for k in range(11, 33) for d in (-1, 0, 1)] + [5000, 100000, 3000001]))
    last_path, last_wg, seen = 0, 0, set()
    for count in counts:
        path, wg = built.plan_reduce_batch(count, elem_bytes)
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
    assert built.plan_reduce_batch(1 << 28, elem_bytes)[1] >= 1024


@pytest.mark.parametrize("elem_bytes", ELEM_BYTES)
def test_the_class_boundaries_are_byte_sizes(built, elem_bytes):
    """A wave's share ends at 4 KiB, a workgroup's at 256 KiB, whatever the element size; 32-element segments are a wave's."""
    wave_limit = max(c for c in range(1, 2100) if built.plan_reduce_batch(c, elem_bytes)[0] == 1)
    assert wave_limit * elem_bytes == 4096
    assert built.plan_reduce_batch(wave_limit + 1, elem_bytes) == (2, 1)
    block_limit = 256 * 1024 // elem_bytes
    assert built.plan_reduce_batch(block_limit, elem_bytes) == (2, 1)
    assert built.plan_reduce_batch(block_limit + 1, elem_bytes) == (3, 2)
    assert built.plan_reduce_batch(32, elem_bytes)[0] == 1


def test_other_element_sizes_are_invalid_arguments(built):
    for elem_bytes in (0, 1, 2, 3, 12, 64):
        with pytest.raises(built.GluError) as e:
            built.plan_reduce_batch(100, elem_bytes)
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert "elem_bytes" in e.value.message


def test_the_batched_calls_fail_loudly_without_a_device_or_an_object(built):
    """No device: every batched call that would compute says so (GLU_ERROR_NO_DEVICE, through GluError) before it looks at its
    arguments.  With a device the same calls, given no object, are invalid arguments."""
    import torch

    want = built.GLU_ERROR_INVALID_ARGUMENT if torch.cuda.is_available() else built.GLU_ERROR_NO_DEVICE
    L = built.lib()
    calls = [
        lambda: L.glu_reduce_run_batch_ptr(None, None, None, 16, 4, None),
        lambda: L.glu_reduce_run_batch_offsets_ptr(None, None, None, 64, None, 4, None),
        lambda: L.glu_reduce_prepare_batch(None, 64, 4),
        lambda: L.glu_reduce_read_batch(None, None, None, None),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want
        assert e.value.message
    if not torch.cuda.is_available():
        with pytest.raises(built.GluError) as e:
            built.Reduce(built.DataType_Uint, built.ReduceOperator_Sum)
        assert e.value.status == built.GLU_ERROR_NO_DEVICE and "no CPU fallback" in e.value.message


def test_the_cpp_wrappers_instantiate(tmp_path):
    src = tmp_path / "reduce_batch_tu.cpp"
    src.write_text('#include "glu/Reduce.hpp"\n'
                   "void f(glu::Reduce& r, const float* a, float* out, const uint32_t* o)\n"
                   "{\n"
                   "    r.reduce_batch(a, out, 100, 7);\n"
                   "    r.reduce_batch_offsets(a, out, 700, o, 7);\n"
                   "    r.prepare_batch(700, 7);\n"
                   "    glu::Reduce::BatchReport b = r.last_batch();\n"
                   "    (void) b.wave_segments; (void) b.block_segments; (void) b.long_segments;\n"
                   "}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "gl-radix-sort_amd"), str(src)])


def test_the_library_makefile_and_the_build_know_the_new_unit():
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "glu_reduce_batch" in mk and "reduce_batch_kernels.hpp" in mk
