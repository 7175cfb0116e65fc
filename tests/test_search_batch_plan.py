"""CPU tests of the host half of the batched sorted search: the four entry points are declared, exported and bound;
glu_sorted_search_plan_batch (a pure function: no device needed) for both key widths against a restatement of tile_plan
(csrc/tile_span.hpp); the default window and its range; the refusal of a bad window, a bad key type and a needle count of 2^32; the
new path value; the build knows the two new headers and none of the new kernels uses scratch memory."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
SYMBOLS = ["glu_sorted_search_run_batch_ptr", "glu_sorted_search_run_batch_offsets_ptr", "glu_sorted_search_set_batch_window",
           "glu_sorted_search_plan_batch"]
KEY_TYPES = ["uint32", "int32", "float32", "uint64", "int64", "float64"]
LDS_BYTES = 32768  # the staged window at the most
DEFAULT = 0xFFFFFFFF
PACKS = 2  # 16-byte packs of needles per thread and tile


def tile_plan(count, elem_bytes, packs):
    """tile_span.hpp's tile_plan, restated: 256 threads x packs x the elements of 16 bytes; the tiles of `count` elements from an
    aligned base."""
    tile = 256 * packs * (16 // elem_bytes)
    return tile, -(-count // tile)


def test_the_four_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in bound, name
    for method in ("run_batch_ptr", "run_batch_offsets_ptr", "set_batch_window"):
        assert callable(getattr(built.SortedSearch, method))
    assert callable(built.plan_sorted_search_batch)
    assert built.SearchPath_Batch == 3 and re.search(r"GLU_SEARCH_PATH_BATCH\s*=\s*3\b", text)
    assert built.SEARCH_BATCH_WINDOW_DEFAULT == DEFAULT and re.search(r"#define\s+GLU_SEARCH_BATCH_WINDOW_DEFAULT\s+0xFFFFFFFFu", text)
    # the batched kernel walks the single search's tiles
    walk = open(os.path.join(CSRC, "search_batch_walk.hpp")).read()
    assert int(re.search(r"kSearchBatchPacks\s*=\s*(\d+)", walk).group(1)) == built.SortedSearch.NEEDLE_PACKS == PACKS
    assert int(re.search(r"kSearchBatchLdsBytes\s*=\s*(\d+)", walk).group(1)) == LDS_BYTES


@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_the_plan_states_tile_tiles_window_and_kernels(built, key_type):
    kb = 8 if key_type.endswith("64") else 4
    tile = 2048 if kb == 4 else 1024
    most = LDS_BYTES // kb
    assert most == (8192 if kb == 4 else 4096)
    for n in (0, 1, tile - 1, tile, tile + 1, 5 * tile, 5 * tile + 1, 65536 * 128, 2**28, 2**32 - 1):
        want_tile, want_tiles = tile_plan(n, kb, PACKS)
        assert want_tile == tile
        for window, used in ((DEFAULT, most), (0, 0), (16, 16), (17, 17), (most - 1, most - 1), (most, most)):
            assert built.plan_sorted_search_batch(n, key_type, window) == (tile, want_tiles, used, 1 if n else 0), (n, window)
    assert built.plan_sorted_search_batch(100, key_type) == (tile, 1, most, 1)  # the default window is the maximum
    assert built.SortedSearch.needle_tile(key_type) == tile


def refused(built, *args):
    with pytest.raises(built.GluError) as e:
        built.plan_sorted_search_batch(*args)
    assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
    return e.value.message


def test_the_plan_refuses_a_bad_window_key_type_or_count(built):
    for key_type, kb in (("uint32", 4), ("float64", 8)):
        most = LDS_BYTES // kb
        for window in (1, 15, most + 1, 2 * most + 1, 2**31, DEFAULT - 1):
            message = refused(built, 100, key_type, window)
            assert "the batch window must be 0 or lie in [16, %d] for %d-byte keys (got %d)" % (most, kb, window) in message, message
    assert built.plan_sorted_search_batch(100, "uint32", 8192)[2] == 8192  # fine for 4-byte keys, refused for 8-byte keys above
    assert "needle_total must be below 2^32" in refused(built, 2**32, "uint32", 0)
    L = built.lib()
    a = ctypes.c_uint32()
    for bad in (-1, 6, 100):
        assert L.glu_sorted_search_plan_batch(10, bad, 0, ctypes.byref(a), None, None, None) != 0
        assert ("Invalid key type: %d" % bad) in L.glu_last_error().decode()
    assert L.glu_sorted_search_plan_batch(10, 0, 0, None, None, None, None) == 0  # any pointer may be NULL


def test_the_build_knows_the_headers_and_no_batched_kernel_spills():
    make = open(os.path.join(CSRC, "Makefile")).read()
    headers = re.search(r"^KERNEL_HEADERS := (.*?)(?<!\\)\n", make, flags=re.S | re.M).group(1)
    assert "sorted_search_batch_kernels.hpp" in headers.split() and "search_batch_walk.hpp" in headers.split()
    users = [n for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".hpp")) and
             '#include "sorted_search_batch_kernels.hpp"' in open(os.path.join(CSRC, n)).read()]
    assert users == ["glu_sorted_search.hip"]
    log = os.path.join(ROOT, "gl-radix-sort_amd", "lib", "kernel_resources.log")
    assert os.path.exists(log), "the build writes the compiler's resource remarks beside the library"
    kernels, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur and "sorted_search_batch_kernel" in cur:
            kernels[cur] = int(m.group(1))
    assert len(kernels) == 12 and set(kernels.values()) == {0}, kernels  # 2 key widths x 3 bounds x 2 needle forms
