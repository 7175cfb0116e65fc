"""CPU test of the arithmetic of merge (csrc/merge_path.hpp): the split of a diagonal, the ranges of a tile with their clamps, the
split of a tile among its threads and a thread's serial merge.  The header is plain C++: a host program merges whole arrays through
its functions alone, tile by tile and thread by thread as merge_kernels.hpp does (its staging buffer stands in for LDS), and reports
the splits, the ranges, the merged keys, where each came from, how often each output was written and whether any index left its
array.  Sorted inputs are held against numpy's stable argsort of the concatenation; shuffled inputs only against the promise that
every range lies inside its array and the outputs tile [0, total) exactly.  The same program, built with the address and
undefined-behaviour sanitizers, runs the same cases as a stand-alone executable.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
THREADS = 256
ITEMS = {4: 11, 8: 7}  # (merge_path.hpp: merge_items)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "merge_path.hpp"
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
// element i of v; an index outside is counted and not read
template<typename T>
static T at(const std::vector<T>& v, uint64_t i)
{
    if (i >= v.size())
    {
        violations++;
        return (T) 0;
    }
    return v[i];
}

template<typename K>
static void one_case(uint32_t na, uint32_t nb)
{
    constexpr uint32_t ITEMS = merge_items(sizeof(K), true), TILE = merge_tile(sizeof(K), true);
    static_assert(TILE == kMergeThreads * ITEMS && ITEMS % 2 == 1, "a tile is 256 threads of an odd number of outputs");
    const std::vector<K> a = get<K>(na), b = get<K>(nb);
    const uint32_t total = na + nb, tiles = (total + TILE - 1) / TILE;
    // the partition kernel
    std::vector<uint32_t> split(tiles + 1);
    const uint32_t steps = merge_steps(na < nb ? na : nb);
    for (uint32_t t = 0; t <= tiles; t++)
    {
        const uint64_t d64 = (uint64_t) t * TILE;
        const uint32_t d = d64 < total ? (uint32_t) d64 : total;
        split[t] = merge_diag_split(
            d, na, nb, steps, [&](uint32_t i, bool any) { return any ? at(a, i) : (K) 0; },
            [&](uint32_t j, bool any) { return any ? at(b, j) : (K) 0; });
    }
    // the tile kernel
    std::vector<uint32_t> ranges(4 * (size_t) tiles), from(total), written(total, 0);
    std::vector<K> merged(total);
    for (uint32_t t = 0; t < tiles; t++)
    {
        const uint32_t d0 = t * TILE, count = total - d0 < TILE ? total - d0 : TILE;
        const MergeRanges r = merge_tile_ranges(split[t], split[t + 1], d0, d0 + count);
        ranges[4 * t] = r.a0, ranges[4 * t + 1] = r.a1, ranges[4 * t + 2] = r.b0, ranges[4 * t + 3] = r.b1;
        if (r.a0 > r.a1 || r.a1 > na || r.b0 > r.b1 || r.b1 > nb || (r.a1 - r.a0) + (r.b1 - r.b0) != count)
        {
            violations++;
            continue;
        }
        const uint32_t ta = r.a1 - r.a0, tb = r.b1 - r.b0;
        std::vector<K> lds(count);
        for (uint32_t x = 0; x < count; x++) lds[x] = x < ta ? at(a, (uint64_t) r.a0 + x) : at(b, (uint64_t) r.b0 + (x - ta));
        const uint32_t tile_steps = merge_steps(ta < tb ? ta : tb);
        for (uint32_t tid = 0; tid < kMergeThreads; tid++)
        {
            const uint32_t diag = merge_thread_diag(tid, ITEMS, count);
            const uint32_t todo = count - diag < ITEMS ? count - diag : ITEMS;
            const uint32_t i0 = merge_diag_split(
                diag, ta, tb, tile_steps, [&](uint32_t i, bool any) { return any ? at(lds, i) : (K) 0; },
                [&](uint32_t j, bool any) { return any ? at(lds, (uint64_t) ta + j) : (K) 0; });
            if (i0 > ta || diag - i0 > tb)
            {
                violations++;
                continue;
            }
            merge_serial<ITEMS, K>(
                i0, diag - i0, ta, tb, todo, [&](uint32_t x, bool any) { return any ? at(lds, x) : (K) 0; },
                [&](uint32_t s, uint32_t x, K key, bool live) {
                    if (!live) return;
                    const uint64_t o = (uint64_t) d0 + diag + s;
                    if (o >= total || x >= count)
                    {
                        violations++;
                        return;
                    }
                    merged[o] = key;
                    from[o] = x < ta ? r.a0 + x : na + r.b0 + (x - ta); // as an element of A || B
                    written[o]++;
                });
        }
    }
    put(std::vector<uint32_t>{tiles});
    put(split);
    put(ranges);
    put(merged);
    put(from);
    put(written);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    in = fopen(argv[1], "rb");
    out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const uint32_t cases = get<uint32_t>(1)[0];
    for (uint32_t c = 0; c < cases; c++)
    {
        const std::vector<uint32_t> h = get<uint32_t>(3); // key bytes, na, nb
        if (h[0] == 8)
            one_case<uint64_t>(h[1], h[2]);
        else
            one_case<uint32_t>(h[1], h[2]);
    }
    put(std::vector<uint64_t>{violations});
    fclose(in);
    fclose(out);
    return violations ? 1 : 0;
}
"""


def tile(key_bytes):
    return THREADS * ITEMS[key_bytes]


def counts(key_bytes):
    T = tile(key_bytes)
    return [0, 1, 5, T - 1, T, 3 * T + 17]


def make_cases():
    """[(kind, key_bytes, A, B)]: every pair of counts; sorted with heavy ties (an alphabet of 3), sorted without ties, shuffled.
    The keys are the encoded ones (unsigned)."""
    rng = np.random.default_rng(14)
    cases = []
    for key_bytes in (4, 8):
        u = np.uint32 if key_bytes == 4 else np.uint64
        for na in counts(key_bytes):
            for nb in counts(key_bytes):
                if key_bytes == 8 and (na + nb) % 2 == 0 and na not in (0, tile(8)):  # (a lighter grid for the second width)
                    continue
                ties = [np.sort(rng.integers(0, 3, n)).astype(u) * u(0x40000001) for n in (na, nb)]
                distinct = rng.permutation(na + nb).astype(u) * u(3 if key_bytes == 4 else 3 << 33)
                unique = [np.sort(distinct[:na]), np.sort(distinct[na:])]
                shuffled = [rng.integers(0, 1 << 31, n).astype(u) for n in (na, nb)]
                half = [np.sort(shuffled[0]), shuffled[1][::-1].copy()]  # (one side sorted, the other anything)
                for kind, (a, b) in (("ties", ties), ("unique", unique), ("shuffled", shuffled), ("shuffled", half)):
                    cases.append((kind, key_bytes, a, b))
    return cases


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The program's source, the cases and their file."""
    tmp = tmp_path_factory.mktemp("merge_path")
    src = tmp / "merge_path.cpp"
    src.write_text(PROGRAM)
    cases = make_cases()
    infile = tmp / "cases.bin"
    with open(infile, "wb") as f:
        f.write(np.array([len(cases)], dtype=np.uint32).tobytes())
        for _, key_bytes, a, b in cases:
            f.write(np.array([key_bytes, a.size, b.size], dtype=np.uint32).tobytes())
            f.write(a.tobytes())
            f.write(b.tobytes())
    return tmp, src, cases, infile


def build_and_run(tmp, src, infile, name, flags):
    exe, outfile = tmp / name, tmp / (name + ".out")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    p = subprocess.run([str(exe), str(infile), str(outfile)], capture_output=True, text=True, timeout=600)
    return p, outfile


@pytest.fixture(scope="module")
def results(setup):
    """[{tiles, split, ranges, merged, from, written}] per case, and the program's count of indices that left their arrays."""
    tmp, src, cases, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "merge_path", [])
    raw = open(outfile, "rb").read()
    pos, out = 0, []

    def take(dtype, n):
        nonlocal pos
        v = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += v.nbytes
        return v

    for _, key_bytes, a, b in cases:
        total = a.size + b.size
        tiles = int(take(np.uint32, 1)[0])
        out.append({"tiles": tiles, "split": take(np.uint32, tiles + 1), "ranges": take(np.uint32, 4 * tiles).reshape(tiles, 4),
                    "merged": take(a.dtype, total), "from": take(np.uint32, total), "written": take(np.uint32, total)})
    violations = int(take(np.uint64, 1)[0])
    assert pos == len(raw)
    return out, violations, p.returncode


def test_no_index_leaves_its_array_sorted_or_not(results):
    _, violations, returncode = results
    assert violations == 0 and returncode == 0


def test_sorted_inputs_split_and_merge_as_the_stable_sort_of_the_concatenation(setup, results):
    """(a) split[t] = the elements of A among the first d of numpy's stable order, at every tile boundary; the whole merge, keys and
    origins, is that order: A first on ties, each side in its own order."""
    _, _, cases, _ = setup
    out, _, _ = results
    seen = 0
    for (kind, key_bytes, a, b), r in zip(cases, out):
        if kind == "shuffled":
            continue
        seen += 1
        T, total = tile(key_bytes), a.size + b.size
        both = np.concatenate([a, b])
        order = np.argsort(both, kind="stable")
        a_in_front = np.concatenate([[0], np.cumsum(order < a.size)])
        case = (kind, key_bytes, a.size, b.size)
        assert r["tiles"] == -(-total // T), case
        want_split = [int(a_in_front[min(t * T, total)]) for t in range(r["tiles"] + 1)]
        assert r["split"].tolist() == want_split, case
        assert (r["merged"] == both[order]).all(), case
        assert (r["from"] == order).all(), case
        assert (r["written"] == 1).all(), case
        if kind == "ties" and a.size >= T and b.size >= T:  # (the ties do straddle tile boundaries)
            assert any(0 < t * T < total and both[order][t * T - 1] == both[order][t * T] for t in range(r["tiles"])), case
    assert seen >= 2 * 36


def test_shuffled_inputs_keep_every_range_inside_and_tile_the_output_exactly(setup, results):
    """(b) whatever the keys hold: max(0, d - nb) <= split <= min(d, na); 0 <= a0 <= a1 <= na and 0 <= b0 <= b1 <= nb; a tile's ranges
    hold exactly its outputs; every output is written once and comes from inside its tile's ranges."""
    _, _, cases, _ = setup
    out, _, _ = results
    seen = 0
    for (kind, key_bytes, a, b), r in zip(cases, out):
        T, total, na, nb = tile(key_bytes), a.size + b.size, a.size, b.size
        case = (kind, key_bytes, na, nb)
        seen += kind == "shuffled"
        for t in range(r["tiles"] + 1):
            d = min(t * T, total)
            assert max(0, d - nb) <= r["split"][t] <= min(d, na), case
        for t in range(r["tiles"]):
            d0, d1 = t * T, min(t * T + T, total)
            a0, a1, b0, b1 = (int(x) for x in r["ranges"][t])
            assert 0 <= a0 <= a1 <= na and 0 <= b0 <= b1 <= nb, (case, t)
            assert a0 == r["split"][t] and b0 == d0 - a0 and (a1 - a0) + (b1 - b0) == d1 - d0, (case, t)
            src = r["from"][d0:d1]
            inside = ((src >= a0) & (src < a1)) | ((src >= na + b0) & (src < na + b1))
            assert inside.all(), (case, t)
        assert (r["written"] == 1).all(), case
        both = np.concatenate([a, b])
        assert (r["merged"] == both[r["from"]]).all(), case
    assert seen >= 2 * 36


def test_the_sanitized_stand_alone_program_runs_clean(setup):
    """(c) the same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly."""
    tmp, src, _, infile = setup
    p, _ = build_and_run(tmp, src, infile, "merge_path_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


def test_the_binding_states_the_headers_tile(built):
    for key_type, key_bytes in (("uint32", 4), ("float32", 4), ("uint64", 8), ("int64", 8)):
        for with_vals in (True, False):
            assert built.plan_merge(1, 1, key_type, with_vals)[0] == tile(key_bytes)
