"""CPU test of GLU_HIP_SCRATCH_FILL, the test switch of the one place where operator scratch is allocated (csrc/glu_host.hpp:
Scratch::reserve).  The rule that reads the variable is plain C++ in csrc/glu_args.hpp: a host program includes it with its own
fail(), as tests/test_args_layer.py does, and prints what it answers for every spelling; the same program runs once more as a
stand-alone executable under -fsanitize=address,undefined.  And without a device nothing can have been filled: the counter of the
library reads 0.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
MESSAGE = 'GLU_HIP_SCRATCH_FILL must be an integer 0 .. 255 (got "%s")'
GOOD = {"0": 0, "255": 255, "90": 90, "0x5A": 0x5A, "0xff": 255, "0X0": 0, "007": 7, "000255": 255}
BAD = ["256", "-1", "+1", "0x100", "0x", "x5A", "5A", "fill", " 1", "1 ", "1.0", "4294967296", "18446744073709551616", "99999999999999999999999"]

PROGRAM = r"""
#include <cstdarg>
#include <cstdio>
#include <string>
#include "glu_args.hpp"
using namespace glu_hip::host;

static std::string g_text;
glu_status glu_hip::host::fail(glu_status code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_text = buf;
    return code;
}

int main(int argc, char** argv)
{
    int byte = 12345;
    glu_status unset = check_scratch_fill(nullptr, &byte);
    printf("unset %d %d\n", (int) unset, byte);
    byte = 12345;
    unset = check_scratch_fill("", &byte);
    printf("empty %d %d\n", (int) unset, byte);
    for (int i = 1; i < argc; i++)
    {
        g_text.clear();
        byte = 12345;
        const glu_status st = check_scratch_fill(argv[i], &byte);
        printf("value [%s] %d %d [%s]\n", argv[i], (int) st, byte, g_text.c_str());
    }
    return 0;
}
"""


def build_and_run(tmp, name, flags):
    src = tmp / "scratch_fill.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           str(src)])
    return subprocess.run([str(exe), *GOOD, *BAD], capture_output=True, text=True)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("scratch_fill")


@pytest.fixture(scope="module")
def printed(tmp):
    p = build_and_run(tmp, "scratch_fill", [])
    assert p.returncode == 0, p.stderr
    return p.stdout.splitlines()


def test_unset_and_empty_fill_nothing(printed):
    assert printed[:2] == ["unset 0 -1", "empty 0 -1"]


def test_a_byte_in_decimal_or_hexadecimal_is_taken(printed):
    for text, byte in GOOD.items():
        assert "value [%s] 0 %d []" % (text, byte) in printed, text


def test_anything_else_is_an_invalid_argument_with_the_message(printed):
    for text in BAD:
        assert "value [%s] 1 -1 [%s]" % (text, MESSAGE % text) in printed, text
    assert len(printed) == 2 + len(GOOD) + len(BAD)


def test_the_switch_sits_in_the_one_place_scratch_is_allocated():
    """Scratch::reserve asks fill_new_scratch behind its hipMalloc; glu_core.hip reads the variable there with glu_env, at every growth
    (no static), and nowhere else does a unit read it."""
    host = open(os.path.join(CSRC, "glu_host.hpp")).read()
    reserve = host[host.index("glu_status reserve(size_t bytes)"):host.index("void release()")]
    assert reserve.index("hipMalloc(&ptr, bytes)") < reserve.index("fill_new_scratch(ptr, bytes)")
    core = open(os.path.join(CSRC, "glu_core.hip")).read()
    body = core[core.index("glu_status fill_new_scratch("):core.index("Device g_dev;")]
    assert 'glu_env("GLU_HIP_SCRATCH_FILL")' in body and "static" not in body
    assert "hipMemset(ptr, byte, bytes)" in body and body.index("hipMemset(") < body.index("hipDeviceSynchronize()") < body.index("g_scratch_filled +=")
    readers = [n for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".hpp")) and '"GLU_HIP_SCRATCH_FILL"' in open(os.path.join(CSRC, n)).read()]
    assert readers == ["glu_core.hip"], readers


def test_without_a_device_the_counter_reads_zero(built, monkeypatch):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    monkeypatch.setenv("GLU_HIP_SCRATCH_FILL", "255")
    assert built.scratch_filled_bytes() == 0
    with pytest.raises(built.GluError) as e:  # (no object, so no growth: nothing reads the variable, nothing is filled)
        built.KeyRuns()
    assert e.value.status == built.GLU_ERROR_NO_DEVICE
    assert built.scratch_filled_bytes() == 0


def test_the_sanitized_stand_alone_program_runs_clean(tmp, printed):
    """the same program under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly"""
    p = build_and_run(tmp, "scratch_fill_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0 and p.stderr == "", p.stderr
    assert p.stdout.splitlines() == printed


def test_the_harness_of_the_gpu_tests_can_fail(monkeypatch):
    """under_every_fill of tests/test_gpu_scratch_fill.py on a stand-in for the library: it passes a case that grows and tells the same
    under every fill, and fails one that tells something else under one fill, one whose object holds more than was filled, one that
    fills nothing, and an operator without scratch that fills something."""
    import numpy as np

    import test_gpu_scratch_fill as sf

    monkeypatch.setattr(sf.sb, "sync", lambda: None)

    class Library:
        filled = 0

        def scratch_filled_bytes(self):
            return self.filled

    def case_of(lib, grows, held, told_under):
        def case():
            lib.filled += grows
            return held, told_under(int(os.environ[sf.ENV]))
        return case

    same = lambda fill: {"out": np.arange(4, dtype=np.float32), "last": (1, 2)}  # noqa: E731
    lib = Library()
    sf.under_every_fill(lib, monkeypatch, case_of(lib, 64, 64, same))
    sf.under_every_fill(lib, monkeypatch, case_of(lib, 0, 0, same), moves=False)
    sf.under_every_fill(lib, monkeypatch, case_of(lib, 0, 0, same), moves=None)
    nan_where_filled = lambda fill: {"out": np.array([1.0 if fill == 0 else np.nan], dtype=np.float32)}  # noqa: E731
    one_bit = lambda fill: {"out": np.array([0.0 if fill != 0x5A else -0.0], dtype=np.float32)}  # noqa: E731
    report = lambda fill: {"last": {"path": 1, "candidates": fill}}  # noqa: E731
    for told in (nan_where_filled, one_bit, report):
        with pytest.raises(AssertionError, match="differs from what it is after a fill of zeros"):
            sf.under_every_fill(lib, monkeypatch, case_of(lib, 64, 64, told))
    for grows, held, moves in ((32, 64, True), (0, 0, True), (0, 64, None), (4, 0, False)):
        with pytest.raises(AssertionError, match="bytes"):
            sf.under_every_fill(lib, monkeypatch, case_of(lib, grows, held, same), moves=moves)
