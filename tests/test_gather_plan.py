"""CPU tests of the host half of gather and scatter: the eight entry points are declared, exported and bound; glu_gather_plan (a pure
function: no device needed) against a restatement; the C++ header compiles alone and beside the other ten; the build knows the new
unit, and its kernels use no scratch memory and no LDS; and the arithmetic of csrc/gather_walk.hpp, which is plain C++: a host
program walks whole small arrays through it as gather_kernels.hpp does, for every item size, every alignment of the streaming side
and the counts around a pack and a tile, and runs the batched forms' row, segment and source computation on equal partitions and on
offsets with empty segments, a decreasing pair and an end beyond total, against numpy.  The same program, built with the address and
undefined-behaviour sanitizers, runs the same cases as a stand-alone executable.  No device needed."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
SYMBOLS = ["glu_gather_create", "glu_gather_destroy", "glu_gather_run_ptr", "glu_gather_run_batch_ptr", "glu_gather_run_batch_offsets_ptr",
           "glu_gather_scatter_ptr", "glu_gather_plan", "glu_gather_last"]
ITEM_SIZES = (4, 8, 16, 32)
HEADERS = ["Gather", "TopK", "Expand", "Histogram", "Merge", "SortedSearch", "Select", "KeyRuns", "Reduce", "BlellochScan", "RadixSort"]


def header_packs():
    text = open(os.path.join(CSRC, "gather_walk.hpp")).read()
    assert "return GLU_GATHER_PACKS;" in text
    return int(re.search(r"#define GLU_GATHER_PACKS (\d+)", text).group(1))


def restated_tile(item_bytes):
    """256 threads x PACKS packs of 16 bytes of the streaming side"""
    return 256 * header_packs() * 16 // item_bytes


def restated(count, item_bytes):
    tile = restated_tile(item_bytes)
    return tile, -(-count // tile), 1 if count else 0


def test_the_eight_symbols_are_declared_exported_and_bound(built):
    raw = open(os.path.join(ROOT, "include", "glu_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"GLU_API\s+[\w\s\*]+?\b(glu_\w+)\s*\(", text)
    L = ctypes.CDLL(built.LIB_PATH)
    bound = {n for n, _, _ in built.SYMBOLS}
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in bound, name
        before = raw[:raw.index("GLU_API glu_status %s(" % name)]
        assert before[before.rindex("/*"):].startswith("/* Not in the reference"), name
    for method in ("run_ptr", "run_batch_ptr", "run_batch_offsets_ptr", "scatter_ptr", "last", "destroy"):
        assert callable(getattr(built.Gather, method))
    assert not hasattr(built.Gather, "prepare")  # no scratch: nothing to prepare
    assert callable(built.plan_gather)


def test_the_plan_follows_the_restated_rule(built):
    assert header_packs() == 4
    for item_bytes in ITEM_SIZES:
        T = restated_tile(item_bytes)
        assert T == {4: 4096, 8: 2048, 16: 1024, 32: 512}[item_bytes]
        for count in (0, 1, T - 1, T, T + 1, 3 * T + 5, 2 ** 32 - 1):
            assert built.plan_gather(count, item_bytes) == restated(count, item_bytes), (count, item_bytes)
        assert built.plan_gather(0, item_bytes) == (T, 0, 0)
        assert built.plan_gather(T, item_bytes) == (T, 1, 1) and built.plan_gather(T + 1, item_bytes) == (T, 2, 1)
    built.check(built.lib().glu_gather_plan(100, 8, None, None, None))  # any pointer may be NULL
    for call, message in ((lambda: built.plan_gather(2 ** 32, 4), "count must be below 2^32"), (lambda: built.plan_gather(2 ** 40, 32), "count"),
                          (lambda: built.plan_gather(10, 12), "item_bytes"), (lambda: built.plan_gather(10, 0), "item_bytes"),
                          (lambda: built.plan_gather(10, 64), "item_bytes")):
        with pytest.raises(built.GluError) as e:
            call()
        assert e.value.status == built.GLU_ERROR_INVALID_ARGUMENT
        assert message in e.value.message, e.value.message


def test_the_calls_fail_loudly_without_a_device_or_an_object(built):
    import torch

    want = built.GLU_ERROR_INVALID_ARGUMENT if torch.cuda.is_available() else built.GLU_ERROR_NO_DEVICE
    L = built.lib()
    calls = [
        lambda: L.glu_gather_run_ptr(None, None, 64, 4, None, 64, None, None),
        lambda: L.glu_gather_run_batch_ptr(None, None, 4, 64, 2, None, 3, None, None),
        lambda: L.glu_gather_run_batch_offsets_ptr(None, None, 4, 64, None, 2, None, 3, None, None),
        lambda: L.glu_gather_scatter_ptr(None, None, 4, None, 64, None, 64, None),
        lambda: L.glu_gather_last(None, None, None),
        lambda: L.glu_gather_create(None),
    ]
    for call in calls:
        with pytest.raises(built.GluError) as e:
            built.check(call())
        assert e.value.status == want
        assert e.value.message


def syntax_only(*args):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + list(args))


def test_the_cpp_header_compiles_alone_and_beside_the_other_ten(tmp_path):
    includes = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gl-radix-sort_amd")]
    alone = tmp_path / "gather_alone.cpp"
    alone.write_text('#include "glu/Gather.hpp"\nint main() { return 0; }\n')
    syntax_only(*includes, str(alone))
    assert len(HEADERS) == 11
    src = tmp_path / "gather_tu.cpp"
    src.write_text("".join('#include "glu/%s.hpp"\n' % h for h in HEADERS) +
                   "void f(glu::Gather& g, const double* items, const uint32_t* indices, const uint32_t* offsets, double* out,\n"
                   "       glu::ShaderStorageBuffer& x, glu::ShaderStorageBuffer& y, glu::ShaderStorageBuffer& z, void* stream)\n"
                   "{\n"
                   "    g(items, 1000, 8, indices, 500, out, stream);\n"
                   "    g(items, 1000, 8, indices, 500, out);\n"
                   "    g(x, 1000, 16, y, 500, z);\n"
                   "    g.batch(items, 8, 1000, 37, indices, 17, out, stream);\n"
                   "    g.batch_offsets(items, 8, 37000, offsets, 37, indices, 17, out);\n"
                   "    g.scatter(items, 8, indices, 500, out, 1000, stream);\n"
                   "    glu::Gather::Plan p = glu::Gather::plan(500, 8);\n"
                   "    (void) p.tile; (void) p.tiles; (void) p.kernels;\n"
                   "    glu::Gather::Last l = g.last();\n"
                   "    (void) l.tiles; (void) l.kernels;\n"
                   "}\n"
                   "int main() { return 0; }\n")
    syntax_only(*includes, str(src))


def test_the_standalone_header_is_generated_and_compiles(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dist.py"), str(tmp_path)])
    assert os.path.exists(tmp_path / "Gather.hpp")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "Gather.hpp"\n#include "TopK.hpp"\n#include "Expand.hpp"\n#include "RadixSort.hpp"\n'
                  "int main() { return glu::Gather::plan(0, 4).tiles; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", str(tmp_path), str(tu)])
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(DIST)/Gather.hpp" in mk


def test_the_library_makefile_names_the_unit_and_its_three_headers():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    units = re.search(r"^UNITS := (.*)$", mk, flags=re.M).group(1).split()
    assert "glu_gather" in units
    assert "Twenty-one translation units" in mk and len(units) == 21
    kernel_headers = re.search(r"^KERNEL_HEADERS := ((?:.*\\\n)*.*)$", mk, flags=re.M).group(1)
    host_headers = re.search(r"^HOST_HEADERS := (.*)$", mk, flags=re.M).group(1)
    assert "gather_kernels.hpp" in kernel_headers.split() and "gather_walk.hpp" in kernel_headers.split()
    assert "glu_gather_object.hpp" in host_headers.split()


def test_the_gather_kernels_are_built_without_scratch_or_lds(built):
    """lib/kernel_resources.log of this build: the gather kernel, plain and batched, and the scatter kernel for items of 4, 8, 16
    and 32 bytes: twelve kernels, none with scratch memory, none with LDS."""
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
    ours = {k for k in scratch if re.search(r"glu_hip\d+(gather|scatter)_\w*kernel", k)}
    for item_bytes in ITEM_SIZES:
        for pattern in (r"gather_kernelILj%dELb0EE", r"gather_kernelILj%dELb1EE", r"scatter_kernelILj%dEE"):
            name = next((n for n in ours if re.search(pattern % item_bytes, n)), None)
            assert name, (pattern, item_bytes)
    assert len(ours) == 12, sorted(ours)
    assert all(scratch[n] == 0 and lds[n] == 0 for n in ours), {n: (scratch[n], lds[n]) for n in ours}


# ---- the walk of gather_walk.hpp on the host -------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gather_walk.hpp"
using namespace glu_hip;

static unsigned long long violations = 0;
static FILE* in;
static FILE* out;

template<typename T>
static std::vector<T> get(size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, in) != n) exit(3);
    return v;
}
template<typename T>
static void put(const std::vector<T>& v)
{
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), out) != v.size()) exit(4);
}

template<uint32_t BYTES>
struct alignas(BYTES) PieceOf
{
    unsigned char b[BYTES];
};

// The walk of one call over `count` items whose streaming side starts `shift` bytes behind a 64-byte boundary; skip[j]: entry j
// fails its test.  visits[piece]: how often the piece was reached; moved[piece]: 1 = element by element, 2 = inside a whole pack.
template<uint32_t ITEM_BYTES>
static void walk(uint32_t shift, uint32_t count, const std::vector<unsigned char>& skip)
{
    using Cfg = GatherCfg<ITEM_BYTES>;
    using Piece = PieceOf<Cfg::PIECE_BYTES>;
    static_assert(sizeof(Piece) == Cfg::PIECE_BYTES, "a piece");
    alignas(64) static unsigned char room[256];
    const uint64_t pieces = (uint64_t) count * Cfg::PIECES;
    const TileSpan<Piece> span = tile_span<Piece, Cfg::PACKS>(room + 64 + shift, pieces);
    if ((const unsigned char*) span.base != room + 64 + (shift & ~15u) || span.lo >= Cfg::VEC || span.hi != span.lo + pieces) violations++;
    const GatherPlan plan = gather_plan(count, ITEM_BYTES);
    if (plan.tile != Cfg::TILE / Cfg::PIECES || span.tiles < plan.tiles || span.tiles > plan.tiles + 1u) violations++;
    std::vector<unsigned char> visits(pieces, 0), moved(pieces, 0);
    unsigned long long outside = 0, whole_packs = 0;
    for (uint32_t t = 0; t < span.tiles; t++)
        for (uint32_t wave = 0; wave < kTileWaves; wave++)
            for (uint32_t g = 0; g < Cfg::PACKS; g++)
                for (uint32_t lane = 0; lane < kTileLanes; lane++)
                {
                    const uint64_t first = gather_pack_first<Cfg>(t, wave, g, lane);
                    if (first % Cfg::VEC) violations++; // packs are aligned
                    bool all_inside = true, all_live = true, live[4] = {false, false, false, false};
                    for (uint32_t k = 0; k < Cfg::VEC; k++)
                    {
                        const bool inside = gather_inside(first + k, span.lo, span.hi);
                        all_inside = all_inside && inside;
                        if (!inside)
                        {
                            outside++;
                            all_live = false;
                            continue;
                        }
                        uint32_t item, part;
                        gather_item_of(first + k, span.lo, Cfg::PIECES, &item, &part);
                        const uint64_t piece = (uint64_t) item * Cfg::PIECES + part;
                        if (item >= count || part >= Cfg::PIECES || piece != first + k - span.lo)
                        {
                            violations++;
                            continue;
                        }
                        visits[piece]++;
                        live[k] = !skip[item];
                        all_live = all_live && live[k];
                    }
                    if (gather_pack_inside(first, Cfg::VEC, span.lo, span.hi) != all_inside) violations++;
                    if (gather_tile_inside(t, Cfg::TILE, span.lo, span.hi) && !all_inside) violations++; // (such a tile tests nothing)
                    if (!gather_tile_inside(t, Cfg::TILE, span.lo, span.hi) && t != 0 && t + 1 != span.tiles) violations++;
                    const bool whole = gather_pack_inside(first, Cfg::VEC, span.lo, span.hi) && all_live;
                    whole_packs += whole;
                    for (uint32_t k = 0; k < Cfg::VEC; k++)
                        if (live[k]) moved[first + k - span.lo] = whole ? 2 : 1;
                }
    // every tile lies in front of the next: the last piece of the last tile is at or beyond hi, and without the last tile it is not
    if (count && ((uint64_t) span.tiles * Cfg::TILE < span.hi || (uint64_t) (span.tiles - 1u) * Cfg::TILE >= span.hi)) violations++;
    put(std::vector<uint32_t>{span.tiles, (uint32_t) span.lo});
    put(std::vector<uint64_t>{outside, whole_packs});
    put(visits);
    put(moved);
}

static void batch(uint32_t k, uint32_t num_segments, uint32_t total, uint32_t offsets_form, uint32_t count)
{
    const std::vector<uint32_t> offsets = get<uint32_t>(offsets_form ? num_segments + 1 : 0);
    const uint64_t entries = (uint64_t) num_segments * k;
    const std::vector<uint32_t> indices = get<uint32_t>(entries);
    const GatherRows rows = gather_make_rows(k, count, total, offsets_form != 0);
    std::vector<unsigned char> moves(entries, 0);
    std::vector<uint32_t> source(entries, 0);
    for (uint64_t j = 0; j < entries; j++)
    {
        uint32_t s, col, begin, len;
        gather_row((uint32_t) j, rows, &s, &col);
        if (s != j / k || col != j % k || s >= num_segments)
        {
            violations++;
            continue;
        }
        if (offsets_form)
            gather_offsets_segment(offsets[s], offsets[s + 1], rows, &begin, &len);
        else
            gather_partition_segment(s, rows, &begin, &len);
        if ((uint64_t) begin + len > total && len) violations++;
        moves[j] = gather_batch_source(begin, len, col, indices[j], rows, &source[j]);
        if (moves[j] && source[j] >= total) violations++; // every begin + index stays below total
    }
    put(moves);
    put(source);
}

static void rows_only(uint32_t k)
{
    const std::vector<uint32_t> n = get<uint32_t>(1);
    const std::vector<uint32_t> j = get<uint32_t>(n[0]);
    const GatherRows rows = gather_make_rows(k, 0, 0, false);
    std::vector<uint32_t> s(n[0]), col(n[0]);
    for (uint32_t i = 0; i < n[0]; i++) gather_row(j[i], rows, &s[i], &col[i]);
    put(s);
    put(col);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    in = fopen(argv[1], "rb");
    out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const uint32_t cases = get<uint32_t>(1)[0];
    put(std::vector<uint32_t>{gather_packs(4), gather_tile(4), gather_tile(8), gather_tile(16), gather_tile(32)});
    for (uint32_t c = 0; c < cases; c++)
    {
        const std::vector<uint32_t> h = get<uint32_t>(6); // kind, then its five words
        if (h[0] == 0)
        {
            const std::vector<unsigned char> skip = get<unsigned char>(h[3]);
            switch (h[1])
            {
            case 4: walk<4>(h[2], h[3], skip); break;
            case 8: walk<8>(h[2], h[3], skip); break;
            case 16: walk<16>(h[2], h[3], skip); break;
            case 32: walk<32>(h[2], h[3], skip); break;
            default: return 5;
            }
        }
        else if (h[0] == 1)
            batch(h[1], h[2], h[3], h[4], h[5]);
        else
            rows_only(h[1]);
    }
    put(std::vector<uint64_t>{violations});
    fclose(in);
    fclose(out);
    printf("%u cases, %llu violations\n", cases, violations);
    return violations ? 1 : 0;
}
"""


def walk_cases():
    """[(item_bytes, shift, count, skip)]: every misalignment of the streaming side within 64 bytes, the counts 0 .. 3 packs + 1 and
    tile - 1, tile, tile + 1; nothing skipped, then every third entry, then a run in the middle."""
    cases = []
    for item_bytes in ITEM_SIZES:
        align = min(item_bytes, 16)
        per_pack = max(1, 16 // item_bytes)
        T = restated_tile(item_bytes)
        for shift in range(0, 64, align):
            for count in list(range(0, 3 * per_pack + 2)) + [T - 1, T, T + 1]:
                cases.append((item_bytes, shift, count, np.zeros(count, dtype=np.uint8)))
        for shift in (0, align):
            count = T + 3 * per_pack + 1
            third = (np.arange(count) % 3 == 1).astype(np.uint8)
            run = np.zeros(count, dtype=np.uint8)
            run[count // 2:count // 2 + 5] = 1
            cases += [(item_bytes, shift, count, third), (item_bytes, shift, count, run), (item_bytes, shift, count, np.ones(count, dtype=np.uint8))]
    return cases


def batch_cases():
    """[(k, offsets or None, count, total, indices)]"""
    rng = np.random.default_rng(21)
    cases = []
    for k, count, parts in ((17, 1000, 37), (1, 5, 9), (600, 100, 3), (3, 1, 40), (50, 32768, 4)):
        total = count * parts
        idx = rng.integers(0, count, parts * k, dtype=np.uint32)
        idx[::7] = rng.choice(np.array([count, count + 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32), idx[::7].size)
        cases.append((k, None, count, total, idx))
    lens = np.array([0, 5, 0, 0, 16, 17, 18, 1, 5000, 0, 33, 600, 601, 2, 0], dtype=np.int64)
    good = (np.concatenate([[0], np.cumsum(lens)]) + 3).astype(np.uint32)
    total = int(good[-1]) + 4
    decreasing = good.copy()
    decreasing[6] = decreasing[5] - 9  # segment 5 ends below its begin; segment 6 begins there
    beyond = good.copy()
    beyond[-1] = total + 1  # the last segment ends beyond total
    far = good.copy()
    far[9] = 0xFFFFFFF0  # segment 8 ends far beyond total, segment 9 begins there and decreases
    for k in (1, 17, 600):
        for offsets in (good, decreasing, beyond, far, good[::-1].copy(), rng.integers(0, 2 ** 32, good.size, dtype=np.uint32)):
            idx = rng.integers(0, 700, (offsets.size - 1) * k, dtype=np.uint32)
            idx[::11] = rng.choice(np.array([5000, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32), idx[::11].size)
            cases.append((k, offsets, 0, total, idx))
    return cases


ROW_DIVISORS = [1, 2, 3, 7, 17, 50, 600, 641, 65535, 65536, 65537, 2 ** 24, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1]


def row_probes(k):
    rng = np.random.default_rng(k & 0xFFFF)
    edge = np.array([0, 1, k - 1, k, k + 1, 2 * k - 1, 2 * k, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], dtype=np.uint64)
    mult = (rng.integers(1, 2 ** 32, 200, dtype=np.uint64) // k) * k
    near = np.concatenate([mult - 1, mult, mult + 1])
    j = np.concatenate([edge, near, rng.integers(0, 2 ** 32, 500, dtype=np.uint64)])
    return (j[j < 2 ** 32]).astype(np.uint32)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gather_walk")
    src = tmp / "gather_walk.cpp"
    src.write_text(PROGRAM)
    walks, batches = walk_cases(), batch_cases()
    infile = tmp / "cases.bin"
    u32 = lambda *v: np.array(v, dtype=np.uint32).tobytes()
    with open(infile, "wb") as f:
        f.write(u32(len(walks) + len(batches) + len(ROW_DIVISORS)))
        for item_bytes, shift, count, skip in walks:
            f.write(u32(0, item_bytes, shift, count, 0, 0))
            f.write(skip.tobytes())
        for k, offsets, count, total, idx in batches:
            n = idx.size // k
            f.write(u32(1, k, n, total, 0 if offsets is None else 1, count))
            if offsets is not None:
                f.write(offsets.tobytes())
            f.write(idx.tobytes())
        for k in ROW_DIVISORS:
            j = row_probes(k)
            f.write(u32(2, k, 0, 0, 0, 0))
            f.write(u32(j.size))
            f.write(j.tobytes())
    return tmp, src, walks, batches, infile


def build_and_run(tmp, src, infile, name, flags):
    exe, outfile = tmp / name, tmp / (name + ".out")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           str(src)])
    p = subprocess.run([str(exe), str(infile), str(outfile)], capture_output=True, text=True, timeout=600)
    return p, outfile


@pytest.fixture(scope="module")
def results(setup):
    tmp, src, walks, batches, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "gather_walk", [])
    raw = open(outfile, "rb").read()
    pos = 0

    def take(dtype, n):
        nonlocal pos
        v = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += v.nbytes
        return v

    head = take(np.uint32, 5)
    w, b, r = [], [], []
    for item_bytes, shift, count, skip in walks:
        pieces = count * (2 if item_bytes == 32 else 1)
        tiles, lo = (int(x) for x in take(np.uint32, 2))
        outside, whole = (int(x) for x in take(np.uint64, 2))
        w.append({"tiles": tiles, "lo": lo, "outside": outside, "whole": whole, "visits": take(np.uint8, pieces), "moved": take(np.uint8, pieces)})
    for k, offsets, count, total, idx in batches:
        b.append({"moves": take(np.uint8, idx.size), "source": take(np.uint32, idx.size)})
    for k in ROW_DIVISORS:
        n = row_probes(k).size
        r.append({"s": take(np.uint32, n), "col": take(np.uint32, n)})
    violations = int(take(np.uint64, 1)[0])
    assert pos == len(raw)
    return {"head": head, "walks": w, "batches": b, "rows": r, "violations": violations, "returncode": p.returncode, "stdout": p.stdout,
            "stderr": p.stderr}


def test_the_header_states_the_tiles_and_no_index_leaves_its_bound(results):
    assert results["violations"] == 0 and results["returncode"] == 0, results["stdout"]
    assert results["head"].tolist() == [header_packs()] + [restated_tile(b) for b in ITEM_SIZES]


def test_every_position_is_visited_once_and_nothing_outside(setup, results):
    """Whatever the alignment: every piece of [0, count) once; the pieces of the walk that lie outside the array are exactly the rest
    of the tiles; tiles is the plan's or one more; a pack is whole only where all of its pieces lie inside and none is skipped, and
    every piece that is not skipped moves, whole or element by element."""
    _, _, walks, _, _ = setup
    seen_extra_tile = False
    for (item_bytes, shift, count, skip), r in zip(walks, results["walks"]):
        case = (item_bytes, shift, count, int(skip.sum()))
        pieces_per = 2 if item_bytes == 32 else 1
        vec = max(1, 16 // item_bytes)
        tile_pieces = restated_tile(item_bytes) * pieces_per
        pieces = count * pieces_per
        lo = (shift % 16) // min(item_bytes, 16)
        assert r["lo"] == lo, case
        plan_tiles = -(-count // restated_tile(item_bytes))
        assert r["tiles"] == (-(-(lo + pieces) // tile_pieces) if count else 0), case
        assert plan_tiles <= r["tiles"] <= plan_tiles + 1, case
        seen_extra_tile |= r["tiles"] == plan_tiles + 1
        assert (r["visits"] == 1).all(), case
        assert r["outside"] == r["tiles"] * tile_pieces - pieces, case
        live = np.repeat(skip == 0, pieces_per)
        assert ((r["moved"] > 0) == live).all(), case
        # the packs as numpy sees them: pack q holds the pieces [q * vec - lo, (q + 1) * vec - lo)
        at = np.arange(pieces) + lo
        padded = np.zeros((-(-(lo + pieces) // vec)) * vec, dtype=bool)
        padded[at] = live
        whole = padded.reshape(-1, vec).all(axis=1)
        assert r["whole"] == int(whole.sum()), case
        assert ((r["moved"] == 2) == np.repeat(whole, vec)[at]).all(), case
    assert seen_extra_tile


def test_the_batched_forms_against_numpy(setup, results):
    _, _, _, batches, _ = setup
    forms = set()
    for (k, offsets, count, total, idx), r in zip(batches, results["batches"]):
        n = idx.size // k
        if offsets is None:
            begin, end = np.arange(n, dtype=np.int64) * count, (np.arange(n, dtype=np.int64) + 1) * count
        else:
            begin, end = offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)
            end = np.where((end < begin) | (end > total), begin, end)  # such a segment is empty
        forms.add((offsets is None, bool((end == begin).any()), bool((end - begin < k).any())))
        length = end - begin
        col = np.tile(np.arange(k), n)
        seg = np.repeat(np.arange(n), k)
        moves = (col < np.minimum(k, length)[seg]) & (idx.astype(np.int64) < length[seg])
        case = (k, n, count, total)
        assert (r["moves"].astype(bool) == moves).all(), case
        source = begin[seg] + idx.astype(np.int64)
        assert (r["source"][moves] == source[moves]).all(), case
        assert (source[moves] < total).all(), case
        assert moves.any() or offsets is not None, case
    assert {f[0] for f in forms} == {True, False} and any(f[1] for f in forms) and any(f[2] for f in forms)


def test_the_row_of_an_entry_is_the_exact_quotient(results):
    for k, r in zip(ROW_DIVISORS, results["rows"]):
        j = row_probes(k).astype(np.uint64)
        assert (r["s"] == j // k).all() and (r["col"] == j % k).all(), k


def test_the_sanitized_stand_alone_program_runs_clean(setup, results):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly; the
    same output, nothing on stderr."""
    tmp, src, _, _, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "gather_walk_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert p.stderr == "", p.stderr[-4000:]
    assert p.stdout == results["stdout"]
    assert open(outfile, "rb").read() == open(tmp / "gather_walk.out", "rb").read()


def test_the_binding_states_the_headers_tile(built):
    for item_bytes in ITEM_SIZES:
        assert built.plan_gather(1, item_bytes)[0] == restated_tile(item_bytes)
