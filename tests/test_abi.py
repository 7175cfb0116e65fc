"""CPU tests of the drop-in boundary: libglu_hip.so loads without a GPU, exports every symbol include/glu_hip.h
declares, the ctypes table matches the header, the C++ headers compile, and compute calls fail loudly (no CPU
fallback) when no MI355X is present."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "glu_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)


def test_header_declares_the_expected_surface():
    names = declared_symbols()
    assert len(names) == len(set(names)) >= 38
    for needed in ("glu_radix_sort_create", "glu_radix_sort_prepare", "glu_radix_sort_run", "glu_scan_run",
                   "glu_reduce_run", "glu_buffer_create_with_data", "glu_buffer_read", "glu_timer_begin", "glu_last_error",
                   "glu_scratch_filled_bytes"):
        assert needed in names


def test_library_exports_every_declared_symbol(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(L, name), "libglu_hip.so does not export %s" % name


def test_ctypes_table_matches_header(built):
    assert sorted(n for n, _, _ in built.SYMBOLS) == sorted(declared_symbols())


def test_no_oracle_or_cpu_path_in_product():
    """The product must not route through the oracle: nothing under gl-radix-sort_amd/ mentions it."""
    pkg = os.path.join(ROOT, "gl-radix-sort_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hpp", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "glu_oracle" not in text and "import oracle" not in text, f
    out = subprocess.run(["ldd", os.path.join(pkg, "lib", "libglu_hip.so")], capture_output=True, text=True).stdout
    assert "oracle" not in out


def test_no_product_kernel_spills_registers_unnoticed(built):
    """The build writes the compiler's per-kernel resource remarks to lib/kernel_resources.log.  Every instantiation of the line
    scatter kernel -- the kernel every large pass runs, one 1024-thread workgroup per CU at exactly 128 registers -- must come
    out with ScratchSize 0 (round 4 had 24 instantiations with 12 .. 80 bytes per lane; 32-bit element indices and a smaller
    tile for the segmented form removed them).  The exceptions are listed with their reason and their bound."""
    import re

    log = os.path.join(ROOT, "gl-radix-sort_amd", "lib", "kernel_resources.log")
    if not os.path.exists(log) or os.path.getmtime(log) < os.path.getmtime(os.path.join(ROOT, "gl-radix-sort_amd", "lib", "libglu_hip.so")) - 600:
        pytest.skip("no resource log beside this build of the library (built by an older Makefile)")
    text = open(log).read()
    kernels = {}
    cur = None
    for line in text.splitlines():
        m = re.search(r"remark: (?:\s*)Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            kernels[cur] = int(m.group(1))
    lines = {k: v for k, v in kernels.items() if "radix_scatter_lines_kernel" in k}
    assert len(lines) >= 20, "the resource log does not hold the line scatter kernels"
    allowed = {
        # 8-byte keys WITH values and 4-bit digits (glu_radix_sort_set_digit_bits(4) on 64-bit keys: the comparison mode with the
        # reference's pass structure): 8 pairs per thread spill 28 / 44 bytes per lane; 5 pairs per thread do not and are not
        # faster (profiles/r05/u64_4bit_kpt_ab.txt)
        "radix_scatter_lines_kernelImLi4ELi1024ELi8E": 48,
        # the SEGMENTED form (sub-block loop around the pass body: the sharded sort's local sort, the long runs of a sort that ends
        # in LDS; last template flags ...ELb1ELb0ELb0E): 24 bytes per lane at 10 pairs per thread, none at 8 -- and 8 is 5 % slower
        # (profiles/r05/seg_scatter_kpt_ab.txt)
        "radix_scatter_lines_kernelIjLi8ELi1024ELi10ELb0ELb1ELi0ELb0ELi4ELb1ELb1ELi0ELb1E": 24,
        "radix_scatter_lines_kernelIjLi8ELi1024ELi10ELb0ELb1ELi0ELb0ELi4ELb1ELb0ELi0ELb1E": 24,
        # round 6: the same segmented form for the LONG RUNS of typed, keys-only and 64-bit sorts that end in LDS (launch_long_run_passes:
        # only the pairs of runs longer than the in-LDS pass's tile pass through them; round 5 sent such sorts to four / eight ordinary
        # passes as a whole).  The sub-block loop keeps 6-13 values more than the 128 registers of a 1024-thread workgroup hold:
        # 24-52 bytes per lane.  Not on the path of any BASELINE configuration (uniform keys have no long runs); measured only
        # through the parity tests (tests/test_gpu_lds_finish.py::test_long_runs_of_every_key_kind).
        "radix_scatter_lines_kernelIjLi8ELi1024ELi10ELb1ELb1ELi0ELb0ELi4ELb1ELb1ELi0ELb1E": 28,  # u32 pairs, typed (decodes on store)
        "radix_scatter_lines_kernelIjLi8ELi1024ELi16ELb1ELb0ELi0ELb0ELi6ELb1ELb1ELi0ELb1E": 24,  # u32 keys only, typed
        "radix_scatter_lines_kernelIjLi8ELi1024ELi16ELb0ELb0ELi0ELb0ELi6ELb1ELb1ELi0ELb1E": 24,  # u32 keys only
        "radix_scatter_lines_kernelImLi8ELi1024ELi6ELb1ELb1ELi0ELb0ELi2ELb1ELb1ELi0ELb1E": 52,   # u64 pairs, typed
        "radix_scatter_lines_kernelImLi8ELi1024ELi6ELb0ELb1ELi0ELb0ELi2ELb1ELb1ELi0ELb1E": 32,   # u64 pairs
        "radix_scatter_lines_kernelImLi8ELi1024ELi10ELb1ELb0ELi0ELb0ELi4ELb1ELb1ELi0ELb1E": 52,  # u64 keys only, typed
        "radix_scatter_lines_kernelImLi8ELi1024ELi10ELb0ELb0ELi0ELb0ELi4ELb1ELb1ELi0ELb1E": 32,  # u64 keys only
    }
    bad = []
    for name, scratch in lines.items():
        limit = max([v for k, v in allowed.items() if k in name] + [0])
        if scratch > limit:
            bad.append((name, scratch))
    assert not bad, bad
    # the in-LDS pass of 64-bit keys asks for six waves per SIMD (three workgroups per CU) and pays a few spilled registers for
    # it: 1.77 against 2.22 ms for 2^28 pairs (profiles/r05/finish_stamps_u64_rank16*.txt); nothing else may spill more
    others = {k: v for k, v in kernels.items() if v > 0 and "radix_scatter_lines_kernel" not in k}
    for name, scratch in others.items():
        # (since round 6 that kernel only takes the runs radix_finish_bucket_kernel lists as crowded; the bucket kernel itself has no scratch)
        assert "radix_finish_sort_kernelImLi512ELi9E" in name and scratch <= 24, (name, scratch)


def test_version_and_error_strings(built):
    L = built.lib()
    assert b"gfx950" in L.glu_version()
    assert L.glu_last_error() is not None


def test_compute_fails_loudly_without_gpu(built):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert built.device_count() == 0
    with pytest.raises(built.GluError) as e:
        built.RadixSort()
    assert e.value.status == built.GLU_ERROR_NO_DEVICE
    assert "no CPU fallback" in e.value.message
    with pytest.raises(built.GluError):
        built.ShaderStorageBuffer(size=16)
    with pytest.raises(built.GluError):
        built.BlellochScan(built.DataType_Uint)
    with pytest.raises(built.GluError):
        built.Reduce(built.DataType_Uint, built.ReduceOperator_Sum)


def test_cpp_headers_compile_standalone(tmp_path):
    """Each public header compiles on its own with g++ -std=c++17 (the reference ships compile-only TUs for its
    amalgamated headers: test/generated/test_include_*.cpp)."""
    for hdr in ("RadixSort.hpp", "BlellochScan.hpp", "Reduce.hpp", "gl_utils.hpp", "data_types.hpp", "errors.hpp"):
        src = tmp_path / ("inc_" + hdr.replace(".", "_") + ".cpp")
        src.write_text('#include "glu/%s"\nint main() { return 0; }\n' % hdr)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "gl-radix-sort_amd"), str(src)])


def test_cpp_api_exit_code_convention_without_gpu(built):
    """GLU_CHECK_* keep the reference's convention (errors.hpp:8-18): message on stderr, exit(1)."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_reduce_api")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 1
    assert "no CPU fallback" in p.stderr


def test_one_make_in_tests_cpp_builds_every_api_test(built):
    """tests/cpp/Makefile finds its programs itself: from its default goal it links every test_*_api.cpp on disk, bench_ladder and
    the RCCL test double; build() runs it once, without -f."""
    import inspect

    import __graft_entry__ as entry

    cpp = os.path.join(ROOT, "tests", "cpp")
    out = subprocess.run(["make", "-C", cpp, "--dry-run", "--always-make"], capture_output=True, text=True, check=True).stdout
    links = [ln for ln in out.splitlines() if " -o bin/" in ln]
    sources = sorted(f for f in os.listdir(cpp) if re.fullmatch(r"test_\w+_api\.cpp", f))
    assert len(sources) >= 13
    for src in sources + ["bench_ladder.cpp"]:
        exe = "bin/" + src[:-len(".cpp")]
        assert [ln for ln in links if "-o %s %s " % (exe, src) in ln and "-lglu_hip" in ln], src
    assert [ln for ln in links if "-o bin/libmock_rccl.so mock_rccl.cpp" in ln and "-shared" in ln]
    assert len(links) == len(sources) + 2
    build = inspect.getsource(entry.build)
    makes = [ln for ln in build.splitlines() if '_run(["make"' in ln and '"tests", "cpp"' in ln]
    assert len(makes) == 1 and '"-f"' not in build and ".mk" not in build, makes


def test_standalone_dist_headers_are_current_and_compile(tmp_path):
    """dist/{RadixSort,BlellochScan,Reduce}.hpp (the reference ships the same three, built by its generate.py) are what
    tools/make_dist.py produces from the current headers, and one translation unit can include all three."""
    import subprocess, sys, filecmp

    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dist.py"), str(tmp_path)])
    for name in ("RadixSort.hpp", "BlellochScan.hpp", "Reduce.hpp"):
        assert filecmp.cmp(os.path.join(ROOT, "dist", name), str(tmp_path / name), shallow=False), name + " is stale"
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "RadixSort.hpp"\n#include "BlellochScan.hpp"\n#include "Reduce.hpp"\n'
                  "int main() { return glu::is_power_of_2(8) ? 0 : 1; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "dist"), str(tu)])


def test_rccl_test_double_exports_what_the_library_binds(built):
    """tests/cpp/mock_rccl.cpp (the file transport of the multi-rank GPU tests) must define every librccl entry point
    glu_dist_* looks up with dlsym -- and the product must not mention it."""
    import re

    src = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "glu_dist.hip")).read()
    bound = set(re.findall(r'sym\("(nccl\w+)"\)', src))
    assert len(bound) == 9
    mock = os.path.join(ROOT, "tests", "cpp", "bin", "libmock_rccl.so")
    assert os.path.exists(mock)
    out = subprocess.run(["nm", "-D", "--defined-only", mock], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert bound <= exported, bound - exported
    for dirpath, _, files in os.walk(os.path.join(ROOT, "gl-radix-sort_amd")):
        for f in files:
            if f.endswith((".py", ".hpp", ".hip", ".h")):
                assert "mock_rccl" not in open(os.path.join(dirpath, f), errors="ignore").read(), f
