"""CPU tests of the host half of the batched histogram: the seven entry points are declared, exported and bound;
glu_histogram_plan_batch (a pure function: no device needed) against a restatement at every length where the class changes, for both
key widths and both modes; the scratch of a prepared batch stays at or below total / 8 bytes; the argument errors; the C++ header
compiles with the new members; without a device the calls fail loudly; the new kernels use no scratch memory and the LDS that
DESIGN.md 4.22 states."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
SYMBOLS = ["glu_histogram_run_batch_even_ptr", "glu_histogram_run_batch_offsets_even_ptr", "glu_histogram_run_batch_edges_ptr",
           "glu_histogram_run_batch_offsets_edges_ptr", "glu_histogram_prepare_batch", "glu_histogram_plan_batch", "glu_histogram_read_batch"]
WAVE_BYTES, WAVE_BINS, CHUNK_BYTES, PER_BIN, LDS_BINS = 8192, 2048, 1 << 19, 64, 8192
CASES = [(k, m) for m in ("even", "edges") for k in ("uint32", "float32", "uint64", "float64") if not (m == "even" and k == "uint64")]


def restated(count, bins, key_bytes):
    """The header's rule: (path, workgroups, (wave_limit, block_limit), chunk, scratch_bytes_per_chunk)."""
    wave_limit = WAVE_BYTES // key_bytes if bins <= WAVE_BINS else 0
    chunk = max(CHUNK_BYTES // key_bytes, PER_BIN * bins)
    path = 0 if count == 0 else 1 if count <= wave_limit else 2 if count <= chunk else 3
    return path, (0, 1, 1, -(-count // chunk))[path], (wave_limit, chunk), chunk, 4 * bins


def test_the_seven_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glu_hip.h")).read(), flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in bound, name
    for method in ("run_batch_even_ptr", "run_batch_offsets_even_ptr", "run_batch_edges_ptr", "run_batch_offsets_edges_ptr", "prepare_batch",
                   "read_batch"):
        assert callable(getattr(built.Histogram, method))
    assert callable(built.plan_histogram_batch)
    assert re.search(r"\bGLU_HISTOGRAM_PATH_BATCH = 2\b", text) and built.HistogramPath_Batch == 2
    # the constants this file restates are the header's
    src = open(os.path.join(CSRC, "histogram_bins.hpp")).read()
    assert re.search(r"#define GLU_HIST_BATCH_WAVE_BYTES 8192\b", src) and re.search(r"#define GLU_HIST_BATCH_CHUNK_BYTES \(1u << 19\)", src)
    assert re.search(r"#define GLU_HIST_BATCH_BLOCK_BYTES GLU_HIST_BATCH_CHUNK_BYTES\b", src)
    assert int(re.search(r"kHistBatchWaveBins\s*=\s*(\d+)", src).group(1)) == WAVE_BINS
    assert int(re.search(r"kHistBatchChunkPerBin\s*=\s*(\d+)", src).group(1)) == PER_BIN
    assert re.search(r"HIST_PATH_BATCH = 2\b", src)


@pytest.mark.parametrize("key_type,mode", CASES)
def test_the_plan_follows_the_restated_rule_where_the_class_changes(built, key_type, mode):
    key_bytes = 8 if key_type.endswith("64") else 4
    for bins in (1, 64, 256, 2048, 2049, 4096, 8192):
        wave_limit, block_limit, chunk = restated(1, bins, key_bytes)[2] + (restated(1, bins, key_bytes)[3],)
        w = wave_limit if wave_limit else WAVE_BYTES // key_bytes
        counts = [0, 1, w, w + 1, block_limit, block_limit + 1] + [k * chunk + d for k in (2, 3, 1000) for d in (0, 1)] + [2 ** 32 - 1]
        for count in counts:
            assert built.plan_histogram_batch(count, bins, key_type, mode) == restated(count, bins, key_bytes), (count, bins)
    assert built.plan_histogram_batch(WAVE_BYTES // key_bytes, 2048, key_type, mode)[0] == 1
    assert built.plan_histogram_batch(1, 2049, key_type, mode)[:3] == (2, 1, (0, 64 * 2049))  # no wave class beyond 2048 bins
    assert built.plan_histogram_batch(64 * 8192 + 1, 8192, key_type, mode)[:2] == (3, 2)  # the chunk grows with the bins
    assert built.plan_histogram_batch(64 * 8192, 8192, key_type, mode)[:2] == (2, 1)
    built.check(built.lib().glu_histogram_plan_batch(100, 100, built.KEY_TYPES[key_type], built.HISTOGRAM_MODES[mode], None, None, None, None,
                                                     None))  # any pointer may be NULL


def test_the_scratch_of_a_prepared_batch_stays_at_or_below_an_eighth_of_a_byte_per_sample(built):
    for key_type, mode in (("uint32", "even"), ("float64", "edges")):
        for bins in (1, 256, 2048, 2049, 8192):
            _, _, (_, block_limit), chunk, row_bytes = built.plan_histogram_batch(1, bins, key_type, mode)
            assert 16 * row_bytes <= chunk  # a chunk's partial row: at most 1/16 of a byte per sample of the chunk
            for total in (0, 1, chunk, chunk + 1, 2 * chunk + 1, 10 * chunk + 7, 2 ** 28, 2 ** 32 - 1):
                for segments in (1, 2, 1000, 2 ** 24):
                    longs = min(segments, total // (block_limit + 1))
                    chunks = total // chunk + longs if longs else 0  # what glu_histogram_prepare_batch reserves rows for
                    assert row_bytes * chunks <= total // 8, (bins, total, segments)


def test_limits_and_bad_types_are_invalid_arguments(built):
    L = built.lib()
    cases = [
        (lambda: built.plan_histogram_batch(2 ** 32, 10), "fewer than 2^32"),
        (lambda: built.plan_histogram_batch(100, 0), "bins must be 1 .. 8192"),
        (lambda: built.plan_histogram_batch(100, 8193), "bins must be 1 .. 8192"),
        (lambda: built.plan_histogram_batch(100, 8193, "float64", "edges"), "bins must be 1 .. 8192"),
        (lambda: built.plan_histogram_batch(100, 10, "uint64", "even"), "glu_histogram_run_batch_edges_ptr"),
        (lambda: built.plan_histogram_batch(100, 10, "int64", "even"), "has no even bins"),
        (lambda: built.plan_histogram_batch(100, 10, "uint32", 2), "Invalid mode"),
        (lambda: built.check(L.glu_histogram_plan_batch(100, 10, 6, 0, None, None, None, None, None)), "Invalid key type"),
    ]
    for call, message in cases:
        with pytest.raises(built.GluError) as e:
            call()
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert message in e.value.message, e.value.message


def test_the_calls_fail_loudly_without_a_device_or_an_object(built):
    import torch

    want = built.GLU_ERROR_INVALID_ARGUMENT if torch.cuda.is_available() else built.GLU_ERROR_NO_DEVICE
    L = built.lib()
    calls = [
        lambda: L.glu_histogram_run_batch_even_ptr(None, None, 64, 2, 0, None, None, 10, None, 0, None),
        lambda: L.glu_histogram_run_batch_offsets_even_ptr(None, None, 64, None, 2, 0, None, None, 10, None, 0, None),
        lambda: L.glu_histogram_run_batch_edges_ptr(None, None, 64, 2, 0, None, 10, None, 0, None),
        lambda: L.glu_histogram_run_batch_offsets_edges_ptr(None, None, 64, None, 2, 0, None, 10, None, 0, None),
        lambda: L.glu_histogram_prepare_batch(None, 64, 2, 10),
        lambda: L.glu_histogram_read_batch(None, None, None, None),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want and e.value.message


def test_the_cpp_header_compiles_with_the_batched_members(tmp_path):
    src = tmp_path / "histogram_batch_tu.cpp"
    src.write_text('#include "glu/Histogram.hpp"\n'
                   '#include "glu/Reduce.hpp"\n'
                   '#include "glu/KeyRuns.hpp"\n'
                   "void f(glu::Histogram& h, const double* d, const float* x, const int32_t* i, const uint32_t* u, const uint64_t* w,\n"
                   "       const double* de, const uint64_t* we, const uint32_t* offsets, uint32_t* out, void* stream)\n"
                   "{\n"
                   "    h.prepare_batch(70000, 37, 8192);\n"
                   "    h.even_batch(d, 1000, 70, -1.0, 1.0, 100, out, false, stream);\n"
                   "    h.even_batch(i, 1000, 70, -50, 50, 100, out, true);\n"
                   "    h.even_batch_offsets(x, 70000, offsets, 37, 0.0f, 1.0f, 100, out);\n"
                   "    h.edges_batch(d, 1000, 70, de, 8192, out, false, stream);\n"
                   "    h.edges_batch_offsets(w, 70000, offsets, 37, we, 10, out, true, stream);\n"
                   "    h.bincount_batch(u, 1000, 70, 1000, out, false, stream);\n"
                   "    h.bincount_batch_offsets(u, 70000, offsets, 37, 1000, out);\n"
                   "    glu::Histogram::BatchClasses c = h.read_batch();\n"
                   "    (void) c.wave_segments; (void) c.block_segments; (void) c.long_segments;\n"
                   "    static_assert(GLU_HISTOGRAM_PATH_BATCH == 2, \"\");\n"
                   "}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "gl-radix-sort_amd"), str(src)])
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_histogram_batch_api.cpp"))


def test_the_library_makefile_knows_the_new_headers():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for name in ("histogram_batch_kernels.hpp", "histogram_batch_walk.hpp"):
        assert name in mk, name
    assert "histogram_batch_kernels.hpp" in open(os.path.join(CSRC, "glu_host.hpp")).read()


def test_the_batched_kernels_are_built_without_scratch_and_with_the_stated_lds(built):
    """lib/kernel_resources.log of this build, read as test_histogram_plan.py reads it: the wave kernel for the four even types (four
    tables of 2048 counters: 32 KiB) and the six edges types (and 2049 staged edges: 40 and 48 KiB), the block kernel with the table
    and the staged edges of histogram_count_kernel (32, 64 and 96 KiB), binning, clear and sum; none with scratch memory."""
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
    ours = {k: v for k, v in scratch.items() if re.search(r"histogram_batch_(bin|clear|wave|block|sum)_kernel", k)}
    tables, table = 4 * WAVE_BINS * 4, LDS_BINS * 4
    # (Itanium codes: j uint32, i int32, f float, d double, m uint64, l int64)
    for code, rule in (("j", "HistEvenInt"), ("i", "HistEvenInt"), ("f", "HistEvenFloat"), ("d", "HistEvenFloat")):
        name = next((n for n in ours if re.search(r"histogram_batch_wave_kernelI%sNS_\d+%sE" % (code, rule), n)), None)
        assert name and tables <= lds[name] <= tables + 16, (code, rule, name)
        name = next((n for n in ours if re.search(r"histogram_batch_block_kernelI%sNS_\d+%sELj256E" % (code, rule), n)), None)
        assert name and table <= lds[name] <= table + 16, (code, rule, name)
    for code, threads, key_bytes in (("j", 512, 4), ("i", 512, 4), ("f", 512, 4), ("m", 1024, 8), ("l", 1024, 8), ("d", 1024, 8)):
        name = next((n for n in ours if re.search(r"histogram_batch_wave_kernelI%sNS_\d+HistEdgesI%sEE" % (code, code), n)), None)
        want = tables + (WAVE_BINS + 1) * key_bytes
        assert name and want <= lds[name] <= want + 16, (code, name)
        name = next((n for n in ours if re.search(r"histogram_batch_block_kernelI%sNS_\d+HistEdgesI%sEELj%dE" % (code, code, threads), n)), None)
        want = table + (LDS_BINS + 1) * key_bytes
        assert name and want <= lds[name] <= want + 16, (code, name)
    for plain in ("bin", "clear", "sum"):
        assert any("histogram_batch_%s_kernel" % plain in n for n in ours), plain
    assert len(ours) == 10 + 10 + 3 and all(v == 0 for v in ours.values()), ours
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("4.22"):]
    for figure in ("32 KiB", "40 KiB", "48 KiB", "64 KiB", "96 KiB"):
        assert figure in section, figure
