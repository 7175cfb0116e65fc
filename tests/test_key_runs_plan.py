"""CPU tests of the host half of key runs: the five entry points are declared, exported and bound; glu_key_runs_plan (a pure
function: no device needed) is consistent; the C++ header and the two compositions compile; without a device the calls fail
loudly; the build knows the new unit and none of its kernels uses scratch memory."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["glu_key_runs_create", "glu_key_runs_destroy", "glu_key_runs_prepare", "glu_key_runs_run_ptr", "glu_key_runs_plan"]


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
        assert callable(getattr(built.KeyRuns, method))
    assert callable(built.plan_key_runs)
    assert callable(built.Reduce.run_by_key_ptr) and callable(built.BlellochScan.run_by_key_ptr)


@pytest.mark.parametrize("key_bits", [32, 64])
def test_the_plan_is_consistent(built, key_bits):
    """tiles == ceil(count / tile) with one tile size per key width (a fixed number of 16-byte packs: 8-byte keys have half the
    tile of 4-byte keys), no tiles for no keys, and the rounds of the count scan never go down as the count grows, start at one
    for one tile and reach two well inside the counts the call takes."""
    tile = built.plan_key_runs(1, key_bits)[0]
    assert tile > 0 and tile % (128 // key_bits) == 0
    assert built.plan_key_runs(1, 32)[0] * 32 == built.plan_key_runs(1, 64)[0] * 64
    assert built.plan_key_runs(0, key_bits) == (tile, 0, 0)
    assert built.plan_key_runs(1, key_bits) == (tile, 1, 1)
    counts = sorted(set(list(range(0, 70)) + [tile * m + d for m in (1, 2, 3, 255, 256, 4095, 4096, 4097, 8192) for d in (-1, 0, 1)]
                        + [2 ** k + d for k in range(8, 33) for d in (-1, 0, 1)]))
    last_rounds, seen = 0, set()
    for count in counts:
        if count >= 2 ** 32:
            continue
        t, tiles, rounds = built.plan_key_runs(count, key_bits)
        assert t == tile
        assert tiles == -(-count // tile), (count, tiles)
        assert rounds >= last_rounds, (count, rounds, last_rounds)
        assert (rounds == 0) == (tiles == 0)
        assert rounds <= tiles
        last_rounds = rounds
        seen.add(rounds)
    assert {0, 1, 2} <= seen
    assert built.plan_key_runs(1 << 26, key_bits)[2] >= 2


def test_other_key_widths_and_counts_are_invalid_arguments(built):
    for key_bits in (0, 1, 8, 16, 31, 33, 48, 128):
        with pytest.raises(built.GluError) as e:
            built.plan_key_runs(100, key_bits)
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert "key_bits" in e.value.message
    with pytest.raises(built.GluError) as e:
        built.plan_key_runs(1 << 32, 32)
    assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
    assert "2^32" in e.value.message


def test_the_calls_fail_loudly_without_a_device_or_an_object(built):
    """No device: every call that would touch one says so (GLU_ERROR_NO_DEVICE, through GluError) before it looks at its
    arguments.  With a device the same calls, given no object, are invalid arguments (tests/test_gpu_key_runs.py has one call for
    every case the host can check)."""
    import torch

    want = built.GLU_ERROR_INVALID_ARGUMENT if torch.cuda.is_available() else built.GLU_ERROR_NO_DEVICE
    L = built.lib()
    calls = [
        lambda: L.glu_key_runs_run_ptr(None, None, 64, 32, 0, 32, None, None, 4, None, None),
        lambda: L.glu_key_runs_run_ptr(None, None, 64, 16, 9, 3, None, None, 1 << 40, None, None),
        lambda: L.glu_key_runs_prepare(None, 64, 32),
        lambda: L.glu_key_runs_create(None),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want
        assert e.value.message
    if not torch.cuda.is_available():
        with pytest.raises(built.GluError) as e:
            built.KeyRuns()
        assert e.value.status == built.GLU_ERROR_NO_DEVICE
        assert "no CPU fallback" in e.value.message


def test_the_compositions_refuse_more_runs_than_a_batch_holds(built):
    """max_runs > 2^24 is refused by the composition itself, before any call into the library (so also without a device)."""
    for cls, args in ((built.Reduce, (None, 1, 2, 3, 64, 4, (1 << 24) + 1, 5)), (built.BlellochScan, (None, 1, 2, 64, 4, (1 << 24) + 1, 5))):
        obj = cls.__new__(cls)
        obj._h = ctypes.c_void_p()
        with pytest.raises(built.GluError) as e:
            obj.run_by_key_ptr(*args)
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert "2^24" in e.value.message


def test_the_cpp_header_and_the_compositions_instantiate(tmp_path):
    src = tmp_path / "key_runs_tu.cpp"
    src.write_text('#include "glu/KeyRuns.hpp"\n'
                   '#include "glu/Reduce.hpp"\n'
                   '#include "glu/BlellochScan.hpp"\n'
                   "void f(glu::KeyRuns& r, glu::Reduce& red, glu::BlellochScan& scan, const uint64_t* keys, uint64_t* unique, uint32_t* o,\n"
                   "       uint32_t* n, float* v, float* out, void* stream)\n"
                   "{\n"
                   "    r.prepare(700, 64);\n"
                   "    r(keys, 700, 64, 8, 40, unique, o, 32, n, stream);\n"
                   "    r(keys, 700, 64, 0, 64, nullptr, o, 32, n);\n"
                   "    glu::KeyRuns::Plan p = glu::KeyRuns::plan(700, 64);\n"
                   "    (void) p.tile; (void) p.tiles; (void) p.scan_rounds;\n"
                   "    glu::KeyRunsArrays k;\n"
                   "    k.keys = keys; k.count = 700; k.key_bits = 64; k.end_bit = 64; k.unique_keys = unique; k.offsets = o;\n"
                   "    k.max_runs = 32; k.num_runs = n;\n"
                   "    red.reduce_by_key(r, k, v, out, stream);\n"
                   "    scan.scan_by_key(r, k, v);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "gl-radix-sort_amd"), str(src)])
    alone = tmp_path / "key_runs_alone.cpp"
    alone.write_text('#include "glu/KeyRuns.hpp"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "gl-radix-sort_amd"), str(alone)])


def test_the_standalone_header_is_generated_and_compiles(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dist.py"), str(tmp_path)])
    assert os.path.exists(tmp_path / "KeyRuns.hpp")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "KeyRuns.hpp"\n#include "Reduce.hpp"\n#include "BlellochScan.hpp"\n'
                  "int main() { return glu::KeyRuns::plan(0).tiles; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", str(tmp_path), str(tu)])
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "$(DIST)/KeyRuns.hpp" in mk


def test_the_library_makefile_and_the_build_know_the_new_unit():
    mk = open(os.path.join(ROOT, "gl-radix-sort_amd", "csrc", "Makefile")).read()
    assert "glu_key_runs" in mk and "key_runs_kernels.hpp" in mk and "glu_key_runs_object.hpp" in mk


def test_every_new_kernel_is_built_for_both_key_widths_without_scratch(built):
    """lib/kernel_resources.log of this build: the two streaming kernels for 4- and 8-byte keys and the scan of the tile counts,
    none with scratch memory."""
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
    for name, want in (("key_runs_count_kernel", 2), ("key_runs_write_kernel", 2), ("key_runs_scan_kernel", 1)):
        mine = {k: v for k, v in kernels.items() if name in k}
        assert len(mine) == want, (name, sorted(mine))
        assert all(v == 0 for v in mine.values()), mine
    for name in ("key_runs_count_kernel", "key_runs_write_kernel"):
        assert {("IjE" in k, "ImE" in k) for k in kernels if name in k} == {(True, False), (False, True)}, name
