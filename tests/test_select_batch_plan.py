"""CPU tests of the host half of the batched select: the four entry points are declared, exported and bound;
glu_select_plan_batch (a pure function: no device needed) against a restatement in Python -- tile and tiles equal to glu_select_plan's,
the rounds of the scan of tiles + 1 counts, the kernels, a scratch of about total / 8 bytes that grows with total and is 0 where total
is 0; the refusals that need no device; the C++ header compiles with the new members; without a device the calls fail loudly; the new
kernels use no scratch memory."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
SYMBOLS = ["glu_select_run_batch_ptr", "glu_select_run_batch_offsets_ptr", "glu_select_prepare_batch", "glu_select_plan_batch"]
STENCILS = {0: 4, 1: 8, 2: 4, 3: 4, 12: 1}  # stencil type: bytes of an element
SCAN_ROUND = 4096


def restated(total, num_segments, elem_bytes):
    """The header's rule: (tile, tiles, scan_rounds, kernels, scratch_bytes)."""
    tile = 256 * (1 if elem_bytes == 1 else 4) * (16 // elem_bytes)
    tiles = -(-total // tile)
    if total == 0:
        return tile, 0, 0, 0, 0
    held = tiles + 1  # a stencil behind a 16-byte boundary can take a tile more
    counts = -(-(held + 1) * 4 // 16) * 16
    return tile, tiles, -(-(tiles + 1) // SCAN_ROUND), 4 if num_segments else 0, counts + 16 * held + held * tile // 8


def test_the_four_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in bound, name
    for method in ("run_batch_ptr", "run_batch_offsets_ptr", "prepare_batch"):
        assert callable(getattr(built.Select, method))
    assert callable(built.plan_select_batch)
    assert re.search(r"\bGLU_SELECT_INDEX_GLOBAL = 0\b", text) and re.search(r"\bGLU_SELECT_INDEX_LOCAL = 1\b", text)
    assert (built.SelectIndex_Global, built.SelectIndex_Local) == (0, 1)


@pytest.mark.parametrize("stencil_type", sorted(STENCILS))
def test_the_plan_follows_the_restated_rule(built, stencil_type):
    elem_bytes = STENCILS[stencil_type]
    tile = restated(1, 1, elem_bytes)[0]
    totals = [0, 1, tile - 1, tile, tile + 1, 3 * tile + 17, (SCAN_ROUND - 1) * tile, (SCAN_ROUND - 1) * tile + 1, SCAN_ROUND * tile + 5, 2 ** 28,
              2 ** 32 - 1]
    last = -1
    for total in totals:
        for form in (built.SelectIndex_Global, built.SelectIndex_Local):
            for segments in (0, 1, 1000, 2 ** 24):
                got = built.plan_select_batch(total, segments, stencil_type, form)
                assert got == restated(total, segments, elem_bytes), (total, segments, form)
                assert got[:2] == built.plan_select(total, stencil_type)[:2]  # tile and tiles are the single call's
        scratch = built.plan_select_batch(total, 1, stencil_type)[4]
        assert scratch >= last and (scratch > last or total <= tile)  # monotone in total: it grows with every tile
        assert total // 8 <= scratch <= total // 8 + tile // 4 + (total // tile + 2) * 20 + 32  # about total / 8: 20 bytes a tile besides
        last = scratch
    assert built.plan_select_batch(0, 5, stencil_type)[4] == 0
    # two rounds of the count scan from 4095 full tiles on: the scan takes tiles + 1 counts
    assert built.plan_select_batch((SCAN_ROUND - 1) * tile, 1, stencil_type)[2] == 1
    assert built.plan_select_batch((SCAN_ROUND - 1) * tile + 1, 1, stencil_type)[2] == 2
    built.check(built.lib().glu_select_plan_batch(100, 10, stencil_type, 0, None, None, None, None, None))  # any pointer may be NULL


def test_limits_and_bad_arguments_are_invalid_arguments(built):
    cases = [
        (lambda: built.plan_select_batch(2 ** 32, 10), "fewer than 2^32"),
        (lambda: built.plan_select_batch(100, 2 ** 24 + 1), "exceeds 2^24"),
        (lambda: built.plan_select_batch(100, 10, 4), "stencil_type"),
        (lambda: built.plan_select_batch(100, 10, -1), "stencil_type"),
        (lambda: built.plan_select_batch(100, 10, 3, 2), "index_form must be"),
        (lambda: built.plan_select_batch(100, 10, 3, -1), "index_form must be"),
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
        lambda: L.glu_select_run_batch_ptr(None, None, 3, 1, None, 64, 2, None, 4, None, None, 0, 64, None, None, None),
        lambda: L.glu_select_run_batch_offsets_ptr(None, None, 3, 1, None, 128, None, 2, None, 4, None, None, 0, 64, None, None, None),
        lambda: L.glu_select_prepare_batch(None, 64, 2, 3),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want and e.value.message


def test_the_cpp_header_compiles_with_the_batched_members(tmp_path):
    src = tmp_path / "select_batch_tu.cpp"
    src.write_text('#include "glu/Select.hpp"\n'
                   "void f(glu::Select& s, const glu::SelectArrays& a, const uint32_t* offsets, uint32_t* out_offsets, void* stream)\n"
                   "{\n"
                   "    s.prepare_batch(70000, 37, glu::SelectStencil_Byte);\n"
                   "    s.select_batch(a, 1000, 70, out_offsets);\n"
                   "    s.select_batch(a, 1000, 70, nullptr, glu::SelectIndex_Local, stream);\n"
                   "    s.select_batch_offsets(a, offsets, 37, out_offsets);\n"
                   "    s.select_batch_offsets(a, offsets, 37, out_offsets, glu::SelectIndex_Local, stream);\n"
                   "    glu::Select::BatchPlan p = glu::Select::plan_batch(70000, 37, glu::SelectStencil_Double, glu::SelectIndex_Local);\n"
                   "    (void) p.tile; (void) p.tiles; (void) p.scan_rounds; (void) p.kernels; (void) p.scratch_bytes;\n"
                   '    static_assert(GLU_SELECT_INDEX_GLOBAL == 0 && GLU_SELECT_INDEX_LOCAL == 1, "");\n'
                   "}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "gl-radix-sort_amd"), str(src)])
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_select_batch_api.cpp"))


def test_the_library_makefile_knows_the_new_headers():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for name in ("select_batch_kernels.hpp", "select_batch_rank.hpp"):
        assert name in mk, name


def test_the_batched_kernels_are_built_without_scratch_memory(built):
    """lib/kernel_resources.log of this build: the count kernel for the five stencil types, the offsets kernel for the three widths,
    the write kernel for three widths x five item sizes x two forms; none with scratch memory, and the single call's kernels are
    still there in their twenty-five and five instantiations."""
    log = os.path.join(ROOT, "gl-radix-sort_amd", "lib", "kernel_resources.log")
    assert os.path.exists(log), "the library's Makefile writes the log beside the library"
    scratch, cur = {}, None
    for line in open(log).read().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
    ours = {k: v for k, v in scratch.items() if "select_batch_" in k}
    for kernel, instances in (("select_batch_count_kernel", 5), ("select_batch_offsets_kernel", 3), ("select_batch_write_kernel", 30)):
        assert sum(kernel in k for k in ours) == instances, (kernel, sorted(ours))
    assert len(ours) == 38 and all(v == 0 for v in ours.values()), ours
    single = [k for k in scratch if re.search(r"select_(count|write)_kernel", k) and "select_batch_" not in k]
    assert len(single) == 30 and all(scratch[k] == 0 for k in single)
