"""CPU tests of the set operations' host side: glu_set_ops_plan against a restatement in Python, the limits, the build's knowledge of
the new headers, the C++ header alone and as the generated stand-alone header, and the compiler's resource report of the new
kernels.  No device needed."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_BYTES = {"uint32": 4, "int32": 4, "float32": 4, "uint64": 8, "int64": 8, "float64": 8}


def restated(a_count, b_count, key_type, with_arrays):
    """(tile, tiles, kernels, scratch_bytes): merge's tile; a boundary is three words (split, start in A, start in B), a tile count one;
    bounds, count, scan, write -- no write where nothing can be written, the scan alone (it writes 0) where there is nothing to look at."""
    tile = 256 * (11 if KEY_BYTES[key_type] == 4 else 7)
    total = a_count + b_count
    tiles = -(-total // tile)
    kernels = (4 if with_arrays else 3) if total else 1
    return tile, tiles, kernels, ((tiles + 1) * 12 + tiles * 4) if total else 0


def test_plan_is_the_restatement(built):
    for key_type in KEY_BYTES:
        T = restated(1, 1, key_type, True)[0]
        assert T == built.plan_merge(1, 1, key_type)[0]
        for a_count, b_count in ((0, 0), (0, 1), (1, 0), (T - 1, 0), (T, 0), (T // 2, T // 2 + 1), (3 * T, 17), (70001, 70001), (1 << 31, (1 << 31) - 1),
                                 ((1 << 32) - 1, 0), (0, (1 << 32) - 1)):
            for with_arrays in (True, False):
                assert built.plan_set_ops(a_count, b_count, key_type, with_arrays) == restated(a_count, b_count, key_type, with_arrays)
    assert built.plan_set_ops(0, 0) == (2816, 0, 1, 0)
    assert built.plan_set_ops(2816, 1, "uint32", False) == (2816, 2, 3, 3 * 12 + 2 * 4)
    assert built.plan_set_ops(1792, 1, "float64") == (1792, 2, 4, 3 * 12 + 2 * 4)


def test_the_limits(built):
    """a_count + b_count <= 2^32 - 1, each count held before their sum; a bad key type."""
    for a_count, b_count in (((1 << 32) - 1, 1), (1 << 31, 1 << 31), (1 << 32, 0), (0, 1 << 32), ((1 << 64) - 1, 2), (1 << 63, 1 << 63)):
        with pytest.raises(built.GluError) as e:
            built.plan_set_ops(a_count, b_count)
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert "set operations take a_count + b_count below 2^32" in e.value.message
    with pytest.raises(built.GluError) as e:
        built.check(built.lib().glu_set_ops_plan(1, 1, 6, 1, None, None, None, None))
    assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT and "Invalid key type" in e.value.message
    built.check(built.lib().glu_set_ops_plan(1, 1, 0, 1, None, None, None, None))  # (any pointer may be NULL)


def test_the_binding_names_the_operations(built):
    assert built.SET_OPS == {"union": 0, "intersection": 1, "difference": 2, "symmetric_difference": 3}
    assert (built.SetOp_Union, built.SetOp_Intersection, built.SetOp_Difference, built.SetOp_SymmetricDifference) == (0, 1, 2, 3)
    header = open(os.path.join(ROOT, "include", "glu_hip.h")).read()
    for name, value in (("GLU_SET_UNION", 0), ("GLU_SET_INTERSECTION", 1), ("GLU_SET_DIFFERENCE", 2), ("GLU_SET_SYMMETRIC_DIFFERENCE", 3)):
        assert re.search(r"\b%s = %d," % (name, value), header), name


def test_the_library_makefile_knows_the_new_headers():
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    kernel_headers = re.search(r"KERNEL_HEADERS :=(.*?)\nHOST_HEADERS", mk, re.S).group(1).split()
    host_headers = re.search(r"HOST_HEADERS :=(.*)", mk).group(1).split()
    assert "set_ops_kernels.hpp" in kernel_headers and "set_ops_path.hpp" in kernel_headers
    assert "glu_set_ops_object.hpp" in host_headers
    assert "$(DIST)/SetOps.hpp" in re.search(r"DIST_HEADERS :=(.*)", mk).group(1).split()
    unit = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "glu_merge.hip")).read()
    for header in ("glu_set_ops_object.hpp", "set_ops_kernels.hpp"):
        assert '#include "%s"' % header in unit


def syntax_only(*args):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + list(args))


USE = ("void f(glu::SetOps& s, const float* a, const uint32_t* av, const float* b, const uint32_t* bv, float* out, uint32_t* ov, uint32_t* n,\n"
       "       void* stream)\n"
       "{\n"
       "    s.prepare(1400, GLU_KEY_FLOAT32);\n"
       "    s.set_union(a, av, 700, b, bv, 700, out, ov, 1400, n, GLU_KEY_FLOAT32, stream);\n"
       "    s.set_intersection(a, av, 700, b, 700, out, ov, 700, n, GLU_KEY_FLOAT32, stream);\n"
       "    s.set_difference(a, nullptr, 700, b, 700, out, nullptr, 700, n, GLU_KEY_FLOAT32);\n"
       "    s.set_symmetric_difference(a, av, 700, b, bv, 700, nullptr, nullptr, 0, n, GLU_KEY_FLOAT32);\n"
       "    s(GLU_SET_UNION, a, av, 700, b, bv, 700, out, ov, 1400, n, GLU_KEY_FLOAT32, stream);\n"
       "    glu::SetOps::Plan p = glu::SetOps::plan(700, 700, GLU_KEY_FLOAT32, false);\n"
       "    (void) p.tile; (void) p.tiles; (void) p.kernels; (void) p.scratch_bytes;\n"
       "    glu::SetOps::Last l = s.last();\n"
       "    (void) l.tiles; (void) l.kernels;\n"
       "}\n"
       "int main() { return 0; }\n")


def test_the_cpp_header_compiles_alone_and_beside_its_siblings(tmp_path):
    includes = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gl-radix-sort_amd")]
    alone = tmp_path / "set_ops_alone.cpp"
    alone.write_text('#include "glu/SetOps.hpp"\nint main() { return 0; }\n')
    syntax_only(*includes, str(alone))
    src = tmp_path / "set_ops_tu.cpp"
    src.write_text('#include "glu/SetOps.hpp"\n#include "glu/Merge.hpp"\n#include "glu/KeyRuns.hpp"\n#include "glu/RadixSort.hpp"\n' + USE)
    syntax_only(*includes, str(src))


def test_the_standalone_header_is_generated_and_compiles(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dist.py"), str(tmp_path)])
    assert os.path.exists(tmp_path / "SetOps.hpp")
    alone = tmp_path / "alone.cpp"
    alone.write_text('#include "SetOps.hpp"\n' + USE)
    syntax_only("-I", str(tmp_path), str(alone))
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "SetOps.hpp"\n#include "Merge.hpp"\n#include "RadixSort.hpp"\nint main() { return glu::SetOps::plan(0, 0).tiles; }\n')
    syntax_only("-I", str(tmp_path), str(tu))


def test_every_new_kernel_is_built_for_both_key_widths_without_scratch(built):
    """lib/kernel_resources.log of this build: the bounds and the count kernel for 4- and 8-byte keys (their Itanium codes: j, m), the
    write kernel for both with and without values, none with scratch memory."""
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
    ours = {k: v for k, v in kernels.items() if "set_ops_" in k}
    assert {re.search(r"set_ops_bounds_kernelI(\w)E", k).group(1) for k in ours if "bounds" in k} == set("jm")
    assert {re.search(r"set_ops_count_kernelI(\w)E", k).group(1) for k in ours if "count" in k} == set("jm")
    assert {re.search(r"set_ops_write_kernelI(\w)Lb(\d)EE", k).groups() for k in ours if "write" in k} == {(k, v) for k in "jm" for v in "01"}
    assert len(ours) == 8, sorted(ours)
    assert all(v == 0 for v in ours.values()), ours
