"""CPU tests of the host half of histogram: the seven entry points are declared, exported and bound; glu_histogram_plan (a pure
function: no device needed) against a restatement; the limits; the C++ header compiles alone and beside its siblings; without a
device the calls fail loudly; the build knows the new unit, and its kernels use no scratch memory and the LDS that DESIGN.md 4.15
states."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
SYMBOLS = ["glu_histogram_create", "glu_histogram_destroy", "glu_histogram_prepare", "glu_histogram_run_even_ptr",
           "glu_histogram_run_edges_ptr", "glu_histogram_plan", "glu_histogram_last"]
KEY_TYPES = ["uint32", "int32", "float32", "uint64", "int64", "float64"]
LDS, GLOBAL = 0, 1
LDS_BINS, MAX_EVEN_BINS, PACKS = 8192, 2 ** 24, 4
LIMIT = 2 ** 32 - 1


def constants(key_bytes, mode):
    """(threads, groups_max) of histogram_bins.hpp: 16 waves to the CU beside 32, 64 and 96 KiB of LDS."""
    if mode == "even":
        return 256, 1024
    return (512, 512) if key_bytes == 4 else (1024, 256)


def restated(count, bins, key_bytes, mode):
    """The header's rule for a call that does not accumulate."""
    threads, groups_max = constants(key_bytes, mode)
    tile = threads * PACKS * (16 // key_bytes)
    tiles = -(-count // tile)
    groups = min(tiles, groups_max)
    if bins <= LDS_BINS:
        return LDS, threads, tile, groups, 2 if count else 1, groups * bins * 4
    return GLOBAL, threads, tile, groups, 2 if count else 1, 0


def test_the_seven_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in bound, name
    for method in ("prepare", "run_even_ptr", "run_edges_ptr", "last", "destroy"):
        assert callable(getattr(built.Histogram, method))
    assert callable(built.plan_histogram)
    for name, value in (("GLU_HISTOGRAM_EVEN", 0), ("GLU_HISTOGRAM_EDGES", 1), ("GLU_HISTOGRAM_PATH_LDS", 0), ("GLU_HISTOGRAM_PATH_GLOBAL", 1)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    assert (built.HistogramMode_Even, built.HistogramMode_Edges, built.HistogramPath_Lds, built.HistogramPath_Global) == (0, 1, 0, 1)
    # the constants this file restates are the header's
    src = open(os.path.join(CSRC, "histogram_bins.hpp")).read()
    assert re.search(r"hist_threads\(.*?\)\s*\{\s*return mode == HIST_EVEN \? 256u : key_bytes == 4 \? 512u : 1024u;", src)
    assert re.search(r"hist_groups_max\(.*?\)\s*\{\s*return mode == HIST_EVEN \? 1024u : key_bytes == 4 \? 512u : 256u;", src)
    assert int(re.search(r"kHistLdsBins\s*=\s*(\d+)", src).group(1)) == LDS_BINS
    assert int(re.search(r"kHistPacks\s*=\s*(\d+)", src).group(1)) == PACKS
    assert re.search(r"kHistMaxEvenBins\s*=\s*1u << 24", src)


# (64-bit integers have no even bins: test_limits_and_bad_types_are_invalid_arguments)
@pytest.mark.parametrize("key_type,mode", [(k, m) for m in ("even", "edges") for k in KEY_TYPES if not (m == "even" and k in ("uint64", "int64"))])
def test_the_plan_follows_the_restated_rule(built, key_type, mode):
    key_bytes = 8 if key_type.endswith("64") else 4
    threads, groups_max = constants(key_bytes, mode)
    T = threads * PACKS * (16 // key_bytes)
    counts = [0, 1, 5, T - 1, T, T + 1, 3 * T + 17, groups_max * T - 1, groups_max * T, groups_max * T + 1, 2 ** 28, LIMIT]
    all_bins = [1, 2, 63, 64, 65, 8191, 8192] + ([8193, 2 ** 20, MAX_EVEN_BINS] if mode == "even" else [])
    for count in counts:
        for bins in all_bins:
            assert built.plan_histogram(count, bins, key_type, mode) == restated(count, bins, key_bytes, mode), (count, bins)
    assert built.plan_histogram(0, 100, key_type, mode) == (LDS, threads, T, 0, 1, 0)
    assert built.plan_histogram(1, 100, key_type, mode) == (LDS, threads, T, 1, 2, 400)
    assert built.plan_histogram(LIMIT, 8192, key_type, mode)[3:] == (groups_max, 2, groups_max * 8192 * 4)
    if mode == "even":
        assert built.plan_histogram(LIMIT, 8193, key_type, mode) == (GLOBAL, threads, T, groups_max, 2, 0)
        assert built.plan_histogram(0, 8193, key_type, mode) == (GLOBAL, threads, T, 0, 1, 0)
    built.check(built.lib().glu_histogram_plan(100, 100, built.KEY_TYPES[key_type], built.HISTOGRAM_MODES[mode], None, None, None, None, None,
                                               None))  # any pointer may be NULL


def test_limits_and_bad_types_are_invalid_arguments(built):
    L = built.lib()
    cases = [
        (lambda: built.plan_histogram(2 ** 32, 10), "count below 2^32"),
        (lambda: built.plan_histogram(2 ** 64 - 1, 10, "float64", "edges"), "count below 2^32"),
        (lambda: built.plan_histogram(100, 0), "bins must be 1 .. 16777216"),
        (lambda: built.plan_histogram(100, MAX_EVEN_BINS + 1), "bins must be 1 .. 16777216"),
        (lambda: built.plan_histogram(100, 0, "uint32", "edges"), "bins must be 1 .. 8192"),
        (lambda: built.plan_histogram(100, 8193, "uint64", "edges"), "bins must be 1 .. 8192"),
        (lambda: built.plan_histogram(100, 8193, "float32", "edges"), "sort the samples, search the edges"),
        (lambda: built.plan_histogram(100, 10, "uint64", "even"), "glu_histogram_run_edges_ptr"),
        (lambda: built.plan_histogram(100, 10, "int64", "even"), "has no even bins"),
        (lambda: built.plan_histogram(100, 10, "uint32", 2), "Invalid mode"),
        (lambda: built.plan_histogram(100, 10, "uint32", -1), "Invalid mode"),
        (lambda: built.check(L.glu_histogram_plan(100, 10, 6, 0, None, None, None, None, None, None)), "Invalid key type"),
        (lambda: built.check(L.glu_histogram_plan(100, 10, -1, 1, None, None, None, None, None, None)), "Invalid key type"),
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
        lambda: L.glu_histogram_run_even_ptr(None, None, 64, 0, None, None, 10, None, 0, None),
        lambda: L.glu_histogram_run_edges_ptr(None, None, 64, 0, None, 10, None, 0, None),
        lambda: L.glu_histogram_prepare(None, 64, 10),
        lambda: L.glu_histogram_last(None, None, None, None),
        lambda: L.glu_histogram_create(None),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want
        assert e.value.message
    if not torch.cuda.is_available():
        with pytest.raises(built.GluError) as e:
            built.Histogram()
        assert e.value.status == built.GLU_ERROR_NO_DEVICE
        assert "no CPU fallback" in e.value.message


def syntax_only(*args):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + list(args))


def test_the_cpp_header_compiles_alone_and_beside_its_siblings(tmp_path):
    includes = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gl-radix-sort_amd")]
    alone = tmp_path / "histogram_alone.cpp"
    alone.write_text('#include "glu/Histogram.hpp"\nint main() { return 0; }\n')
    syntax_only(*includes, str(alone))
    src = tmp_path / "histogram_tu.cpp"
    src.write_text('#include "glu/Histogram.hpp"\n'
                   '#include "glu/Merge.hpp"\n'
                   '#include "glu/SortedSearch.hpp"\n'
                   '#include "glu/Select.hpp"\n'
                   '#include "glu/KeyRuns.hpp"\n'
                   '#include "glu/Reduce.hpp"\n'
                   '#include "glu/BlellochScan.hpp"\n'
                   '#include "glu/RadixSort.hpp"\n'
                   "void f(glu::Histogram& h, const double* d, const float* x, const int32_t* i, const uint32_t* u, const uint64_t* w, const int64_t* s,\n"
                   "       const double* de, const uint64_t* we, const int64_t* se, uint32_t* out, glu::ShaderStorageBuffer& a, glu::ShaderStorageBuffer& b,\n"
                   "       void* stream)\n"
                   "{\n"
                   "    h.prepare(70000, 8192);\n"
                   "    h.even(d, 70000, -1.0, 1.0, 100, out, false, stream);\n"
                   "    h.even(x, 70000, 0.0f, 1.0f, 100, out, true);\n"
                   "    h.even(i, 70000, -50, 50, 100, out);\n"
                   "    h.even(u, 70000, 0u, 1u << 20, 1 << 20, out);\n"
                   "    h.edges(d, 70000, de, 8192, out, false, stream);\n"
                   "    h.edges(w, 70000, we, 10, out);\n"
                   "    h.edges(s, 70000, se, 10, out, true);\n"
                   "    h.bincount(u, 70000, 1000, out, false, stream);\n"
                   "    h.bincount(a, 10, 20, b);\n"
                   "    glu::Histogram::Plan p = glu::Histogram::plan(70000, 500, GLU_KEY_FLOAT64, GLU_HISTOGRAM_EDGES);\n"
                   "    (void) p.path; (void) p.threads; (void) p.tile; (void) p.groups; (void) p.kernels; (void) p.scratch_bytes;\n"
                   "    glu::Histogram::Last l = h.last();\n"
                   "    (void) l.path; (void) l.groups; (void) l.kernels;\n"
                   "}\n"
                   "int main() { return 0; }\n")
    syntax_only(*includes, str(src))


def test_the_standalone_header_is_generated_and_compiles(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dist.py"), str(tmp_path)])
    assert os.path.exists(tmp_path / "Histogram.hpp")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "Histogram.hpp"\n#include "Merge.hpp"\n#include "SortedSearch.hpp"\n#include "Select.hpp"\n#include "KeyRuns.hpp"\n'
                  '#include "Reduce.hpp"\n#include "BlellochScan.hpp"\n#include "RadixSort.hpp"\n'
                  "int main() { return glu::Histogram::plan(0, 1).groups; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", str(tmp_path), str(tu)])
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(DIST)/Histogram.hpp" in mk


def test_the_library_makefile_and_the_build_know_the_new_unit():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for name in ("glu_histogram", "histogram_kernels.hpp", "histogram_bins.hpp", "glu_histogram_object.hpp"):
        assert name in mk, name
    assert "glu_histogram.hip" in open(os.path.join(CSRC, "glu_host.hpp")).read()


def test_the_histogram_kernels_are_built_without_scratch_and_with_the_stated_lds(built):
    """lib/kernel_resources.log of this build: the counting kernel for the four even types (256 threads, the table: 32 KiB) and the six
    edges types (the table and 8193 edges: 64 KiB + 16 with 512 threads, 96 KiB + 16 with 1024), the GLOBAL kernel for the four even
    types (no LDS), the column sum and the clear; none with scratch memory.  The sizes are those of DESIGN.md 4.15."""
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
    ours = {k: v for k, v in scratch.items() if re.search(r"histogram_(count|global|sum|clear)_kernel", k)}
    table = LDS_BINS * 4
    # (Itanium codes: j uint32, i int32, f float, d double, m uint64, l int64)
    for code, rule in (("j", "HistEvenInt"), ("i", "HistEvenInt"), ("f", "HistEvenFloat"), ("d", "HistEvenFloat")):
        name = next((n for n in ours if re.search(r"histogram_count_kernelI%sNS_\d+%sELj256E" % (code, rule), n)), None)
        assert name, (code, rule)
        assert table <= lds[name] <= table + 16, (name, lds[name])
        name = next((n for n in ours if re.search(r"histogram_global_kernelI%sNS_\d+%sELj256E" % (code, rule), n)), None)
        assert name and lds[name] == 0, (code, rule)
    for code, threads, key_bytes in (("j", 512, 4), ("i", 512, 4), ("f", 512, 4), ("m", 1024, 8), ("l", 1024, 8), ("d", 1024, 8)):
        name = next((n for n in ours if re.search(r"histogram_count_kernelI%sNS_\d+HistEdgesI%sEELj%dE" % (code, code, threads), n)), None)
        assert name, (code, threads)
        want = table + (LDS_BINS + 1) * key_bytes
        assert want <= lds[name] <= want + 16, (name, lds[name])
        assert (160 * 1024 // lds[name]) * threads == 1024  # 16 waves to the CU
    assert any("histogram_sum_kernel" in n for n in ours) and any("histogram_clear_kernel" in n for n in ours)
    assert len(ours) == 4 + 4 + 6 + 2 and all(v == 0 for v in ours.values()), ours
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("4.15"):]
    for figure in ("32 KiB", "64 KiB", "96 KiB"):
        assert figure in section, figure
