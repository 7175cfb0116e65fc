"""The ordering step of the in-LDS pass (gl-radix-sort_amd/csrc/bucket_order.hpp: two sorting networks, an insertion and the walk over
one thread's bucket masks) is plain C++ that compiles for the host: tests/cpp/test_bucket_order.cpp is a stand-alone program that
checks it exhaustively where that is possible (every 0-1 input of the networks, every permutation for 2 .. 4 and 8 words) and against
std::sort elsewhere.  Built and run here plain, and once more with the address and undefined-behaviour sanitizers: the program has
its own main, nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "test_bucket_order.cpp")


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                       "-fno-omit-frame-pointer"])])
def test_bucket_order_host_program(tmp_path, name, flags):
    exe = tmp_path / ("test_bucket_order_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags, "-I", CSRC, "-o", str(exe), SRC])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.strip().endswith(" 0 failed"), p.stdout[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
