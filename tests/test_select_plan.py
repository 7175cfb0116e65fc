"""CPU tests of the host half of select: the five entry points are declared, exported and bound; glu_select_plan (a pure function:
no device needed) is consistent for the five stencil types; the C++ header compiles alone and beside its siblings; without a
device the calls fail loudly; the build knows the new unit and none of its kernels uses scratch memory."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["glu_select_create", "glu_select_destroy", "glu_select_prepare", "glu_select_run_ptr", "glu_select_plan"]
STENCILS = {"float": (0, 4), "double": (1, 8), "int": (2, 4), "uint": (3, 4), "byte": (12, 1)}  # name: (stencil_type, bytes)


def test_the_five_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in bound, name
    for method in ("prepare", "run_ptr", "destroy"):
        assert callable(getattr(built.Select, method))
    assert callable(built.plan_select)
    assert [built.SelectStencil_Float, built.SelectStencil_Double, built.SelectStencil_Int, built.SelectStencil_Uint,
            built.SelectStencil_Byte] == [0, 1, 2, 3, 12]
    assert [built.SelectOperator_EQ, built.SelectOperator_NE, built.SelectOperator_LT, built.SelectOperator_LE, built.SelectOperator_GT,
            built.SelectOperator_GE] == list(range(6))
    assert re.search(r"#define\s+GLU_SELECT_STENCIL_BYTE\s+12\b", text)
    for i, name in enumerate(("EQ", "NE", "LT", "LE", "GT", "GE")):
        assert re.search(r"GLU_SELECT_%s\b" % name, text), name
    assert re.search(r"GLU_SELECT_EQ\s*=\s*0\s*,\s*GLU_SELECT_NE\s*,\s*GLU_SELECT_LT\s*,\s*GLU_SELECT_LE\s*,\s*GLU_SELECT_GT\s*,\s*GLU_SELECT_GE\b", text)


@pytest.mark.parametrize("stencil", sorted(STENCILS))
def test_the_plan_is_consistent(built, stencil):
    """tiles == ceil(count / tile) with one tile size per stencil type (a whole number of 16-byte packs), no tiles for no elements,
    and the rounds of the count scan never go down as the count grows, start at one for one tile and reach two below 2^26."""
    stencil_type, nbytes = STENCILS[stencil]
    tile = built.plan_select(1, stencil_type)[0]
    assert tile > 0 and (tile * nbytes) % 16 == 0
    assert built.plan_select(0, stencil_type) == (tile, 0, 0)
    assert built.plan_select(1, stencil_type) == (tile, 1, 1)
    counts = sorted(set(list(range(0, 70)) + [tile * m + d for m in (1, 2, 3, 255, 256, 4095, 4096, 4097, 8192) for d in (-1, 0, 1)]
                        + [2 ** k + d for k in range(8, 33) for d in (-1, 0, 1)]))
    assert 2 ** 32 - 1 in counts
    last_rounds, seen = 0, set()
    for count in counts:
        if count >= 2 ** 32:
            continue
        t, tiles, rounds = built.plan_select(count, stencil_type)
        assert t == tile
        assert tiles == -(-count // tile), (count, tiles)
        assert rounds >= last_rounds, (count, rounds, last_rounds)
        assert (rounds == 0) == (tiles == 0)
        assert rounds <= tiles
        last_rounds = rounds
        seen.add(rounds)
    assert {0, 1, 2} <= seen
    assert built.plan_select((1 << 26) - 1, stencil_type)[2] >= 2


def test_other_stencil_types_and_counts_are_invalid_arguments(built):
    for stencil_type in list(range(4, 12)) + [13, -1]:
        with pytest.raises(built.GluError) as e:
            built.plan_select(100, stencil_type)
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert "stencil_type" in e.value.message
    with pytest.raises(built.GluError) as e:
        built.plan_select(1 << 32, built.SelectStencil_Uint)
    assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
    assert "count" in e.value.message and "2^32" in e.value.message


def test_the_calls_fail_loudly_without_a_device_or_an_object(built):
    """No device: every call that would touch one says so (GLU_ERROR_NO_DEVICE, through GluError) before it looks at its
    arguments.  With a device the same calls, given no object, are invalid arguments (tests/test_gpu_select.py has one call for
    every case the host can check)."""
    import torch

    want = built.GLU_ERROR_INVALID_ARGUMENT if torch.cuda.is_available() else built.GLU_ERROR_NO_DEVICE
    L = built.lib()
    calls = [
        lambda: L.glu_select_run_ptr(None, None, 3, 1, None, 64, None, 4, None, None, 4, None, None),
        lambda: L.glu_select_run_ptr(None, None, 7, 9, None, 1 << 40, None, 5, None, None, 1 << 40, None, None),
        lambda: L.glu_select_prepare(None, 64, 3),
        lambda: L.glu_select_create(None),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want
        assert e.value.message
    if not torch.cuda.is_available():
        with pytest.raises(built.GluError) as e:
            built.Select()
        assert e.value.status == built.GLU_ERROR_NO_DEVICE
        assert "no CPU fallback" in e.value.message


def test_a_threshold_outside_the_stencils_type_is_refused_before_the_call(built):
    """run_ptr packs a Python number into the stencil's type; 256 is no byte, -1 no uint32, 2.5 no int32: refused by the binding
    itself, before any call into the library (so also without a device)."""
    sel = built.Select.__new__(built.Select)
    sel._h = ctypes.c_void_p()
    for stencil_type, threshold in ((built.SelectStencil_Byte, 256), (built.SelectStencil_Uint, -1), (built.SelectStencil_Int, 1 << 31),
                                    (built.SelectStencil_Int, 2.5)):
        with pytest.raises(built.GluError) as e:
            sel.run_ptr(0, 0, 0, 0, stencil_type=stencil_type, threshold=threshold)
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert "threshold" in e.value.message


def syntax_only(*args):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + list(args))


def test_the_cpp_header_compiles_alone_and_beside_its_siblings(tmp_path):
    includes = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gl-radix-sort_amd")]
    alone = tmp_path / "select_alone.cpp"
    alone.write_text('#include "glu/Select.hpp"\nint main() { return 0; }\n')
    syntax_only(*includes, str(alone))
    src = tmp_path / "select_tu.cpp"
    src.write_text('#include "glu/Select.hpp"\n'
                   '#include "glu/KeyRuns.hpp"\n'
                   '#include "glu/Reduce.hpp"\n'
                   '#include "glu/BlellochScan.hpp"\n'
                   "void f(glu::Select& s, const float* stencil, const void* items, void* out_items, uint32_t* indices, uint32_t* n,\n"
                   "       void* stream)\n"
                   "{\n"
                   "    const float threshold = 0.5f;\n"
                   "    s.prepare(700, glu::SelectStencil_Float);\n"
                   "    s(stencil, glu::SelectStencil_Float, glu::SelectOperator_Greater, &threshold, 700, items,\n"
                   "      glu::Select::item_bytes(glu::DataType_Vec4), out_items, indices, 32, n, stream);\n"
                   "    glu::Select::Plan p = glu::Select::plan(700, glu::SelectStencil_Byte);\n"
                   "    (void) p.tile; (void) p.tiles; (void) p.scan_rounds;\n"
                   "    glu::SelectArrays a;\n"
                   "    a.stencil = stencil; a.stencil_type = glu::SelectStencil_Float; a.op = glu::SelectOperator_LessEqual;\n"
                   "    a.threshold = &threshold; a.count = 700; a.out_indices = indices; a.max_out = 32; a.num_selected = n;\n"
                   "    s(a, stream);\n"
                   "    s(a);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    syntax_only(*includes, str(src))


def test_the_standalone_header_is_generated_and_compiles(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dist.py"), str(tmp_path)])
    assert os.path.exists(tmp_path / "Select.hpp")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "Select.hpp"\n#include "KeyRuns.hpp"\n#include "Reduce.hpp"\n#include "BlellochScan.hpp"\n#include "RadixSort.hpp"\n'
                  "int main() { return glu::Select::plan(0).tiles; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", str(tmp_path), str(tu)])
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "$(DIST)/Select.hpp" in mk


def test_the_library_makefile_and_the_build_know_the_new_unit():
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "glu_select" in mk and "select_kernels.hpp" in mk and "glu_select_object.hpp" in mk


def test_every_new_kernel_is_built_for_the_five_stencil_types_without_scratch(built):
    """lib/kernel_resources.log of this build: the count kernel for the five stencil types (their Itanium codes: f, d, i, j, h) and
    the write kernel for every stencil type without items and with items of 4, 8, 16 and 32 bytes, none with scratch memory."""
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
    count = {k: v for k, v in kernels.items() if "select_count_kernel" in k}
    assert len(count) == 5, sorted(count)
    assert {re.search(r"select_count_kernelI(\w)E", k).group(1) for k in count} == set("fdijh")
    write = {k: v for k, v in kernels.items() if "select_write_kernel" in k}
    assert len(write) == 25, sorted(write)
    assert {re.search(r"select_write_kernelI(\w)Lj(\d+)EE", k).groups() for k in write} == {(s, b) for s in "fdijh" for b in ("0", "4", "8", "16", "32")}
    assert all(v == 0 for v in count.values()) and all(v == 0 for v in write.values()), (count, write)
