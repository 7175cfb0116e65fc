"""CPU tests of the host half of sorted search: the eight entry points are declared, exported and bound; glu_sorted_search_plan (a
pure function: no device needed) against a restatement of the level rule; the C++ header compiles alone and beside its siblings;
without a device the calls fail loudly; the build knows the new unit and none of its kernels uses scratch memory."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["glu_sorted_search_create", "glu_sorted_search_destroy", "glu_sorted_search_prepare", "glu_sorted_search_set_option",
           "glu_sorted_search_index_ptr", "glu_sorted_search_run_ptr", "glu_sorted_search_plan", "glu_sorted_search_last"]
DIRECT, INDEXED = 1, 2
LDS_BYTES = 32768  # the top level of the index lies in LDS
NEEDLE_RATIO = 128  # AUTO takes the index iff needle_count * 128 >= hay_count


def level_rule(hay_count, needle_count, key_bytes, top_entries=0):
    """The issue's rule, restated: F = 128 / key_bytes; len_k = hay_count // F^k; L = the smallest k with len_k <= top_entries;
    every level's room a multiple of 128 bytes; AUTO takes INDEXED iff L >= 1 and needle_count * 128 >= hay_count."""
    fanout = 128 // key_bytes
    top = top_entries or LDS_BYTES // key_bytes
    levels, index_bytes = 0, 0
    while hay_count // fanout ** levels > top:
        levels += 1
        index_bytes += -(-(hay_count // fanout ** levels * key_bytes) // 128) * 128
    path = INDEXED if levels >= 1 and needle_count * NEEDLE_RATIO >= hay_count else DIRECT
    return path, levels, fanout, index_bytes


def test_the_eight_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in bound, name
    for method in ("prepare", "set_option", "index_ptr", "run_ptr", "last", "destroy"):
        assert callable(getattr(built.SortedSearch, method))
    assert callable(built.plan_sorted_search)
    assert [built.SearchPath_Auto, built.SearchPath_Direct, built.SearchPath_Indexed] == [0, 1, 2]
    assert re.search(r"GLU_SEARCH_PATH_AUTO\s*=\s*0\s*,\s*GLU_SEARCH_PATH_DIRECT\s*=\s*1\s*,\s*GLU_SEARCH_PATH_INDEXED\s*=\s*2\b", text)
    # the needle tile the binding states is the kernels'
    kernels = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "sorted_search_kernels.hpp")).read()
    assert int(re.search(r"kSearchPacks\s*=\s*(\d+)", kernels).group(1)) == built.SortedSearch.NEEDLE_PACKS
    assert built.SortedSearch.needle_tile("uint32") == 2 * built.SortedSearch.needle_tile("float64") == 256 * built.SortedSearch.NEEDLE_PACKS * 4
    # the ratio the host uses is the one the header and this file state
    host = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "glu_sorted_search_object.hpp")).read()
    assert int(re.search(r"kIndexNeedleRatio\s*=\s*(\d+)", host).group(1)) == NEEDLE_RATIO


@pytest.mark.parametrize("key_type", ["uint32", "int32", "float32", "uint64", "int64", "float64"])
def test_the_plan_follows_the_level_rule(built, key_type):
    key_bytes = 8 if key_type.endswith("64") else 4
    F = 128 // key_bytes
    counts = [0, 1, F - 1, F, F + 1, F * F - 1, F * F, F * F + 1, 8192, 8193, 2 ** 20, 2 ** 28, 2 ** 32 - 1]
    seen_levels, seen_paths = set(), set()
    for top in (0, F, 100, LDS_BYTES // key_bytes):
        for hay_count in counts:
            edge = -(-hay_count // NEEDLE_RATIO)  # the fewest needles that take the index
            for needle_count in sorted({0, 1, max(edge - 1, 0), edge, edge + 1, 2 ** 32 - 1}):
                got = built.plan_sorted_search(hay_count, needle_count, key_type, top)
                assert got == level_rule(hay_count, needle_count, key_bytes, top), (hay_count, needle_count, top)
                seen_levels.add(got[1])
                seen_paths.add(got[0])
                assert got[2] == F
                assert got[3] % 128 == 0 and (got[3] == 0) == (got[1] == 0)
                # the index holds fewer than hay_count / (F - 1) keys (before every level is rounded up to a line)
                assert got[3] <= hay_count * key_bytes // (F - 1) + 128 * got[1]
    assert {0, 1, 2, 3} <= seen_levels and seen_paths == {DIRECT, INDEXED}
    # the defaults: what LDS holds needs no index, one key more takes one level of hay_count // F entries
    top = LDS_BYTES // key_bytes
    assert built.plan_sorted_search(top, top, key_type) == (DIRECT, 0, F, 0)
    assert built.plan_sorted_search(top + 1, top, key_type) == (INDEXED, 1, F, -(-((top + 1) // F * key_bytes) // 128) * 128)
    # 2^28 uint32 keys: three levels (2^23, 2^18 and 2^13 entries, the last one in LDS), 35 MB
    if key_type == "uint32":
        path, levels, _, index_bytes = built.plan_sorted_search(2 ** 28, 2 ** 28, key_type)
        assert (path, levels) == (INDEXED, 3) and index_bytes == (2 ** 23 + 2 ** 18 + 2 ** 13) * 4
        assert built.plan_sorted_search(2 ** 28, 2 ** 21 - 1, key_type)[0] == DIRECT
        assert built.plan_sorted_search(2 ** 28, 2 ** 21, key_type)[0] == INDEXED
        assert built.plan_sorted_search(2 ** 20, 0, key_type, 32)[1] == 3  # (what the GPU tests use to reach three levels)


def test_counts_key_types_and_top_entries_out_of_range_are_invalid_arguments(built):
    L = built.lib()
    cases = [
        (lambda: built.plan_sorted_search(1 << 32, 1, "uint32"), "hay_count below 2^32"),
        (lambda: built.plan_sorted_search(1, 1 << 32, "uint32"), "needle_count below 2^32"),
        (lambda: built.check(L.glu_sorted_search_plan(100, 100, 6, 0, None, None, None, None)), "Invalid key type"),
        (lambda: built.check(L.glu_sorted_search_plan(100, 100, -1, 0, None, None, None, None)), "Invalid key type"),
        (lambda: built.plan_sorted_search(100, 100, "uint32", 31), "TOP_ENTRIES"),
        (lambda: built.plan_sorted_search(100, 100, "uint32", 8193), "TOP_ENTRIES"),
        (lambda: built.plan_sorted_search(100, 100, "uint64", 15), "TOP_ENTRIES"),
        (lambda: built.plan_sorted_search(100, 100, "uint64", 4097), "TOP_ENTRIES"),
    ]
    for call, message in cases:
        with pytest.raises(built.GluError) as e:
            call()
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert message in e.value.message, e.value.message
    assert built.plan_sorted_search(2 ** 32 - 1, 2 ** 32 - 1, "uint64", 16)[1] == 7  # the most levels there are
    built.check(L.glu_sorted_search_plan(100, 100, 0, 0, None, None, None, None))  # any pointer may be NULL


def test_the_calls_fail_loudly_without_a_device_or_an_object(built):
    """No device: every call that would touch one says so (GLU_ERROR_NO_DEVICE, through GluError) before it looks at its
    arguments.  With a device the same calls, given no object, are invalid arguments."""
    import torch

    want = built.GLU_ERROR_INVALID_ARGUMENT if torch.cuda.is_available() else built.GLU_ERROR_NO_DEVICE
    L = built.lib()
    calls = [
        lambda: L.glu_sorted_search_run_ptr(None, None, 64, None, 64, 0, None, None, 0, None),
        lambda: L.glu_sorted_search_index_ptr(None, None, 64, 0, None),
        lambda: L.glu_sorted_search_prepare(None, 64, 0),
        lambda: L.glu_sorted_search_set_option(None, b"PATH", 0),
        lambda: L.glu_sorted_search_last(None, None, None, None),
        lambda: L.glu_sorted_search_create(None),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want
        assert e.value.message
    if not torch.cuda.is_available():
        with pytest.raises(built.GluError) as e:
            built.SortedSearch()
        assert e.value.status == built.GLU_ERROR_NO_DEVICE
        assert "no CPU fallback" in e.value.message


def syntax_only(*args):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + list(args))


def test_the_cpp_header_compiles_alone_and_beside_its_siblings(tmp_path):
    includes = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gl-radix-sort_amd")]
    alone = tmp_path / "sorted_search_alone.cpp"
    alone.write_text('#include "glu/SortedSearch.hpp"\nint main() { return 0; }\n')
    syntax_only(*includes, str(alone))
    src = tmp_path / "sorted_search_tu.cpp"
    src.write_text('#include "glu/SortedSearch.hpp"\n'
                   '#include "glu/Select.hpp"\n'
                   '#include "glu/KeyRuns.hpp"\n'
                   '#include "glu/Reduce.hpp"\n'
                   '#include "glu/BlellochScan.hpp"\n'
                   '#include "glu/RadixSort.hpp"\n'
                   "void f(glu::SortedSearch& s, const double* hay, const double* needles, uint32_t* lower, uint32_t* upper, void* stream)\n"
                   "{\n"
                   "    s.prepare(70000, GLU_KEY_FLOAT64);\n"
                   "    s.set_path(glu::SearchPath_Indexed);\n"
                   '    s.set_option("TOP_ENTRIES", 16);\n'
                   "    s.index(hay, 70000, GLU_KEY_FLOAT64, stream);\n"
                   "    s(hay, 70000, needles, 500, GLU_KEY_FLOAT64, lower, upper, true, stream);\n"
                   "    s.lower_bound(hay, 70000, needles, 500, GLU_KEY_FLOAT64, lower);\n"
                   "    s.upper_bound(hay, 70000, needles, 500, GLU_KEY_FLOAT64, upper, stream);\n"
                   "    s.equal_range(hay, 70000, needles, 500, GLU_KEY_FLOAT64, lower, upper, stream);\n"
                   "    glu::SortedSearch::Plan p = glu::SortedSearch::plan(70000, 500, GLU_KEY_FLOAT64, 16);\n"
                   "    (void) p.path; (void) p.levels; (void) p.fanout; (void) p.index_bytes;\n"
                   "    glu::SortedSearch::Last l = s.last();\n"
                   "    (void) l.path; (void) l.levels; (void) l.kernels;\n"
                   "}\n"
                   "int main() { return 0; }\n")
    syntax_only(*includes, str(src))


def test_the_standalone_header_is_generated_and_compiles(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dist.py"), str(tmp_path)])
    assert os.path.exists(tmp_path / "SortedSearch.hpp")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "SortedSearch.hpp"\n#include "Select.hpp"\n#include "KeyRuns.hpp"\n#include "Reduce.hpp"\n'
                  '#include "BlellochScan.hpp"\n#include "RadixSort.hpp"\n'
                  "int main() { return glu::SortedSearch::plan(0, 0).levels; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", str(tmp_path), str(tu)])
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "$(DIST)/SortedSearch.hpp" in mk


def test_the_library_makefile_and_the_build_know_the_new_unit():
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "glu_sorted_search" in mk and "sorted_search_kernels.hpp" in mk and "glu_sorted_search_object.hpp" in mk


def test_the_index_and_search_kernels_are_built_for_both_key_widths_without_scratch(built):
    """lib/kernel_resources.log of this build: the index kernel for 4- and 8-byte keys (their Itanium codes: j, m), the direct and
    the indexed search kernels for both widths and for lower, upper and both bounds (1, 2, 3), none with scratch memory, and the
    indexed search kernels with their 32 KiB of LDS."""
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
    index = {k for k in scratch if "sorted_search_index_kernel" in k}
    assert {re.search(r"sorted_search_index_kernelI(\w)E", k).group(1) for k in index} == set("jm") and len(index) == 2, sorted(index)
    direct = {k for k in scratch if "sorted_search_direct_kernel" in k}
    assert {re.search(r"sorted_search_direct_kernelI(\w)Li(\d)EE", k).groups() for k in direct} == {(w, b) for w in "jm" for b in "123"}
    search = {k for k in scratch if re.search(r"\d+sorted_search_kernelI", k)}
    assert {re.search(r"sorted_search_kernelI(\w)Li(\d)EE", k).groups() for k in search} == {(w, b) for w in "jm" for b in "123"}
    assert len(direct) == len(search) == 6
    for k in index | direct | search:
        assert scratch[k] == 0, (k, scratch[k])
    assert all(lds[k] == LDS_BYTES for k in search) and all(lds[k] == 0 for k in index | direct)
