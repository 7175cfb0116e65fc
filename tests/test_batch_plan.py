"""CPU tests of the batched radix sort's host half: the five entry points are declared, exported and bound; which path and tile an
equal-length batch takes (glu_radix_sort_plan_batch is a pure function: no device needed); the C++ wrappers compile."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["glu_radix_sort_run_batch_ptr", "glu_radix_sort_run_batch_offsets_ptr", "glu_radix_sort_prepare_batch",
           "glu_radix_sort_plan_batch", "glu_radix_sort_read_batch"]


def test_the_five_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in bound, name
    for method in ("sort_batch_ptr", "sort_batch_offsets_ptr", "prepare_batch", "read_batch"):
        assert callable(getattr(built.RadixSort, method))
    assert callable(built.plan_batch)


@pytest.mark.parametrize("key_bytes", [4, 8])
@pytest.mark.parametrize("with_vals", [True, False])
def test_nothing_to_do_below_two_elements(built, key_bytes, with_vals):
    assert built.plan_batch(0, key_bytes, with_vals)[0] == 0
    assert built.plan_batch(1, key_bytes, with_vals)[0] == 0
    assert built.plan_batch(2, key_bytes, with_vals)[0] == 1


@pytest.mark.parametrize("key_bytes,limit", [(4, 16384), (8, 8192)])
@pytest.mark.parametrize("with_vals", [True, False])
def test_paths_are_monotone_and_tiles_hold_the_partition(built, key_bytes, limit, with_vals):
    """The path never goes down as the partitions grow; on the two in-LDS paths the tile holds the partition; the workgroup path
    ends exactly at the single-block limit of the ordinary sort (16384 elements with 4-byte keys, 8192 with 8-byte keys)."""
    counts = sorted(set(list(range(0, 1100)) + [2 ** k + d for k in range(10, 21) for d in (-1, 0, 1)] + [limit - 1, limit, limit + 1,
                                                                                                         5000, 12288, 12289, 100000]))
    last_path, last_tile = 0, 0
    for count in counts:
        path, tile = built.plan_batch(count, key_bytes, with_vals)
        assert path in (0, 1, 2, 3)
        assert path >= last_path, (count, path, last_path)
        if path in (1, 2):
            assert tile >= count, (count, tile)
            assert tile >= last_tile, (count, tile, last_tile)
            last_tile = tile
        last_path = path
    assert built.plan_batch(limit, key_bytes, with_vals) == (2, limit)
    assert built.plan_batch(limit + 1, key_bytes, with_vals)[0] == 3
    wave_limit = max(c for c in counts if built.plan_batch(c, key_bytes, with_vals)[0] == 1)
    assert 64 <= wave_limit < 1024  # a wave holds a few elements per lane, not a workgroup's tile
    assert built.plan_batch(wave_limit + 1, key_bytes, with_vals)[0] == 2


def test_bad_key_bytes_is_an_invalid_argument(built):
    for key_bytes in (0, 2, 3, 16):
        with pytest.raises(built.GluError) as e:
            built.plan_batch(100, key_bytes)
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT


def test_the_cpp_wrappers_instantiate(tmp_path):
    src = tmp_path / "batch_tu.cpp"
    src.write_text('#include "glu/RadixSort.hpp"\n'
                   "void f(glu::RadixSort& s, float* a, uint64_t* b, uint32_t* v, const uint32_t* o)\n"
                   "{\n"
                   "    s.sort_batch<float>(a, v, 100, 7);\n"
                   "    s.sort_batch_offsets<uint64_t>(b, nullptr, 700, o, 7);\n"
                   "    s.prepare_internal_buffers_batch(700, 7, 8, false);\n"
                   "    (void) s.last_batch();\n"
                   "}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "gl-radix-sort_amd"), str(src)])
