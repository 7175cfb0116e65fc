"""CPU tests of top-k's host side: glu_top_k_plan (no device: the digit windows, the tile and tiles of select for the key width, the
default capacity, the scratch bytes, the kernels enqueued for each combination of outputs), the refusals the host makes without a
device, and that the build knows the new unit."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
KEY_BYTES = {"uint32": 4, "int32": 4, "float32": 4, "uint64": 8, "int64": 8, "float64": 8}
STATE_BYTES = 48  # sizeof(TopkState): two 8-byte words and eight 4-byte ones


def test_the_digit_windows_cover_the_key_from_the_top(built):
    for key_type, kb in KEY_BYTES.items():
        p = built.plan_top_k(12345, 7, key_type)
        assert p["rounds"] == (3 if kb == 4 else 6)
        assert [b for _, b in p["digits"]] == ([11, 11, 10] if kb == 4 else [11, 11, 11, 11, 11, 9])
        top = 8 * kb
        for shift, bits in p["digits"]:  # adjacent, from the top bit down to bit 0
            assert shift + bits == top and 1 <= bits <= 11
            top = shift
        assert top == 0


@pytest.mark.parametrize("count", [0, 1, 4095, 4096, 4097, 12289, 2**28, 2**32 - 1])
def test_tile_and_tiles_are_selects_for_the_key_width(built, count):
    for key_type, kb in KEY_BYTES.items():
        stencil = built.SelectStencil_Uint if kb == 4 else built.SelectStencil_Double
        tile, tiles, _ = built.plan_select(count, stencil)
        p = built.plan_top_k(count, min(count, 5), key_type)
        assert (p["tile"], p["tiles"]) == (tile, tiles)
        assert p["tile"] == 256 * 4 * (16 // kb)


def test_the_default_capacity(built):
    for count, want in ((0, 2**16), (1, 2**16), (2**25, 2**16), (2**25 + 1, 2**16 + 1), (2**28, 2**19), (2**32 - 1, 2**23)):
        assert built.plan_top_k(count, 0)["capacity"] == want, count
    assert built.plan_top_k(2**28, 1, cand_capacity=64)["capacity"] == 64


def test_the_kernels_of_every_combination_of_outputs(built):
    A, C, F = built.TopKPath_Auto, built.TopKPath_Candidates, built.TopKPath_Full
    for key_type, kb in KEY_BYTES.items():
        rest = 3 * ((3 if kb == 4 else 6) - 1)  # count, sum, pick for every remaining round over the input
        for path, chain in ((A, 2), (C, 2), (F, 0)):
            base = 3 + chain + rest
            assert built.plan_top_k(10**6, 100, key_type, sorted=False, with_arrays=False, path=path)["kernels"] == base  # out_kth alone
            assert built.plan_top_k(10**6, 100, key_type, sorted=True, with_arrays=False, path=path)["kernels"] == base
            assert built.plan_top_k(10**6, 100, key_type, sorted=False, with_arrays=True, path=path)["kernels"] == base + 4
            assert built.plan_top_k(10**6, 100, key_type, sorted=True, with_arrays=True, path=path)["kernels"] == base + 6
        assert built.plan_top_k(10**6, 0, key_type)["kernels"] == 0
        assert built.plan_top_k(0, 0, key_type)["kernels"] == 0


def test_the_scratch_bytes(built):
    for key_type, kb in KEY_BYTES.items():
        for count, k, cap in ((1, 1, 0), (70001, 1000, 0), (70001, 1000, 8), (2**28, 2**20, 0)):
            p = built.plan_top_k(count, k, key_type, cand_capacity=cap)
            groups = min(p["tiles"], 1024)
            want = STATE_BYTES + 2048 * 4 + groups * 2048 * 4 + p["capacity"] * kb + 2 * (p["tiles"] + 1) * 4 + k * (kb + 4)
            assert p["scratch_bytes"] == want, (key_type, count, k, cap)
        assert built.plan_top_k(0, 0, key_type)["scratch_bytes"] == 0


def test_the_plan_refuses_what_the_host_can_check(built):
    with pytest.raises(built.GluError) as e:
        built.plan_top_k(2**32, 1)
    assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT and "count below 2^32" in e.value.message
    with pytest.raises(built.GluError) as e:
        built.plan_top_k(10, 11)
    assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT and "k must not exceed count" in e.value.message
    with pytest.raises(built.GluError) as e:
        built.plan_top_k(0, 1)
    assert "k must not exceed count" in e.value.message
    with pytest.raises(built.GluError) as e:
        built.plan_top_k(10, 1, path=3)
    assert "path must be" in e.value.message
    with pytest.raises(built.GluError) as e:
        built.plan_top_k(10, 1, cand_capacity=2**30 + 1)
    assert "cand_capacity" in e.value.message
    L = built.lib()
    assert L.glu_top_k_plan(10, 1, 6, 0, 0, 0, 0, *([None] * 8)) == built.GLU_ERROR_INVALID_ARGUMENT
    assert b"Invalid key type" in L.glu_last_error()
    assert L.glu_top_k_plan(10, 1, 0, 0, 0, 0, 0, *([None] * 8)) == built.GLU_OK  # (every pointer may be NULL)


def test_calls_fail_loudly_without_a_device(built):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(built.GluError) as e:
        built.TopK()
    assert e.value.status == built.GLU_ERROR_NO_DEVICE
    L = built.lib()
    assert L.glu_top_k_run_ptr(None, None, 0, 0, 0, 0, 0, None, None, None, None) == built.GLU_ERROR_NO_DEVICE


def test_the_library_makefile_and_the_build_know_the_new_unit():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for name in ("glu_top_k", "topk_kernels.hpp", "topk_pick.hpp", "histogram_walk.hpp", "glu_top_k_object.hpp", "$(DIST)/TopK.hpp"):
        assert name in mk, name
    assert "glu_top_k.hip" in open(os.path.join(CSRC, "glu_host.hpp")).read()


def test_the_top_k_kernels_are_built_without_scratch(built):
    """lib/kernel_resources.log of this build: every top-k kernel, for both key widths, with ScratchSize 0; the counting kernel and
    the candidate rounds hold one table of 2048 counters in LDS."""
    import re

    log = os.path.join(ROOT, "gl-radix-sort_amd", "lib", "kernel_resources.log")
    assert os.path.exists(log), "the library's Makefile writes the log beside the library"
    scratch, lds, cur = {}, {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and cur:
            lds[cur] = int(m.group(1))
    ours = {k: v for k, v in scratch.items() if "topk_" in k}
    for stem in ("topk_count_kernel", "topk_pick_kernel", "topk_collect_kernel", "topk_cand_rounds_kernel", "topk_flag_count_kernel",
                 "topk_write_kernel", "topk_decode_kernel"):
        assert len([k for k in ours if stem in k]) >= 2, stem  # 4- and 8-byte keys
    assert [k for k in ours if "topk_sum_kernel" in k]
    assert all(v == 0 for v in ours.values()), {k: v for k, v in ours.items() if v}
    for name, size in lds.items():
        if "topk_count_kernel" in name:
            assert size == 2048 * 4, (name, size)
        if "topk_cand_rounds_kernel" in name:
            assert 2048 * 4 <= size <= 2048 * 4 + 256, (name, size)


def test_the_dist_header_is_generated_and_compiles(tmp_path):
    import subprocess
    import sys

    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dist.py"), str(tmp_path)])
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "TopK.hpp"\n#include "Select.hpp"\nint main() { return sizeof(glu::TopK::Plan) ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(tmp_path), str(tu)])
