"""CPU test of the arithmetic of expand (csrc/expand_path.hpp over merge_path.hpp): the cut of the merged sequence at every tile
boundary, the ranges of a tile with their clamps, the slots of the tile's slice of offsets, the marks, and the bound on the segment a
gather uses.  The header is plain C++: a host program expands whole arrays through its functions alone, tile by tile as
expand_kernels.hpp does (two vectors stand in for LDS, a running maximum for the scan), and reports the splits, the ranges, the three
outputs, how often each position was written and whether any index left its array.  Sorted offsets are held against
numpy.searchsorted; shuffled and out-of-range offsets only against the promise that every index stays inside its bound and the tiles
cut [0, M) exactly.  The same program, built with the address and undefined-behaviour sanitizers, runs the same cases as a
stand-alone executable.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
POISON = 0xA5A5A5A5

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "expand_path.hpp"
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
// element i of v; an index outside is counted and not used
template<typename T>
static T& at(std::vector<T>& v, uint64_t i)
{
    static T sink;
    if (i >= v.size())
    {
        violations++;
        sink = (T) 0;
        return sink;
    }
    return v[i];
}

static void one_case(uint32_t num_segments, uint32_t total)
{
    const uint32_t na = num_segments + 1, nb = total, merged = na + nb;
    std::vector<uint32_t> offsets = get<uint32_t>(na), items(num_segments);
    for (uint32_t s = 0; s < num_segments; s++) items[s] = s * 2654435761u + 17u;
    const uint32_t tiles = (merged + kExpandTile - 1) / kExpandTile;
    // the partition kernel
    std::vector<uint32_t> split(tiles + 1);
    for (uint32_t t = 0; t <= tiles; t++)
        split[t] = expand_split(expand_diag(t, merged), na, nb, [&](uint32_t i, bool any) { return any ? at(offsets, i) : 0u; });
    // the tile kernel
    std::vector<uint32_t> ranges(4 * (size_t) tiles), seg(total, 0xA5A5A5A5u), rank(total, 0xA5A5A5A5u), item(total, 0xA5A5A5A5u), written(total, 0);
    for (uint32_t t = 0; t < tiles; t++)
    {
        const MergeRanges r = expand_tile_ranges(split[t], split[t + 1], t, merged);
        ranges[4 * t] = r.a0, ranges[4 * t + 1] = r.a1, ranges[4 * t + 2] = r.b0, ranges[4 * t + 3] = r.b1;
        if (r.a0 > r.a1 || r.a1 > na || r.b0 > r.b1 || r.b1 > nb || (r.a1 - r.a0) + (r.b1 - r.b0) > kExpandTile)
        {
            violations++;
            continue;
        }
        const uint32_t na_t = r.a1 - r.a0, nb_t = r.b1 - r.b0;
        if (!nb_t) continue;
        std::vector<uint32_t> slice(kExpandTile + 1, 0xDEADBEEFu), marks(kExpandTile, 0u);
        for (uint32_t k = 0; k <= na_t; k++)
        {
            bool has;
            const uint32_t src = expand_slice_source(r.a0, k, &has);
            if (has && src >= r.a1) violations++; // (inside the tile's offsets and the one in front)
            at(slice, k) = has ? at(offsets, src) : 0u;
        }
        for (uint32_t k = 1; k <= na_t; k++)
        {
            uint32_t i;
            if (expand_marks(k, na_t, at(slice, k), k < na_t ? at(slice, k + 1) : 0u, r.b0, nb_t, &i))
            {
                if (i >= nb_t) violations++;
                at(marks, i) = k;
            }
        }
        uint32_t run = 0;
        for (uint32_t i = 0; i < kExpandTile; i++) // the inclusive max-scan
        {
            run = run > marks[i] ? run : marks[i];
            marks[i] = run;
        }
        for (uint32_t i = 0; i < nb_t; i++)
        {
            const uint32_t slot = at(marks, i);
            uint32_t s;
            if (slot > na_t) violations++;
            if (!expand_segment(r.a0, slot, num_segments, &s)) continue;
            const uint64_t j = (uint64_t) r.b0 + i;
            if (s >= num_segments || j >= total)
            {
                violations++;
                continue;
            }
            seg[j] = s;
            rank[j] = (uint32_t) j - at(slice, slot);
            item[j] = at(items, s);
            written[j]++;
        }
    }
    put(std::vector<uint32_t>{tiles});
    put(split);
    put(ranges);
    put(seg);
    put(rank);
    put(item);
    put(written);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    in = fopen(argv[1], "rb");
    out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const uint32_t cases = get<uint32_t>(1)[0];
    put(std::vector<uint32_t>{kExpandTile});
    for (uint32_t c = 0; c < cases; c++)
    {
        const std::vector<uint32_t> h = get<uint32_t>(2); // num_segments, total
        one_case(h[0], h[1]);
    }
    put(std::vector<uint64_t>{violations});
    fclose(in);
    fclose(out);
    return violations ? 1 : 0;
}
"""


def header_tile():
    import re

    text = open(os.path.join(CSRC, "expand_path.hpp")).read()
    threads = int(re.search(r"kExpandThreads = (\d+);", text).group(1))
    items = int(re.search(r"kExpandItems = (\d+);", text).group(1))
    return threads * items


def offsets_from_lengths(lens, first=0):
    return (np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]) + first).astype(np.uint32)


def make_cases():
    """[(kind, offsets, total)]: kind "sorted" (held against numpy) or "malformed" (bounds only)."""
    T = header_tile()
    rng = np.random.default_rng(16)
    cases = []
    for total in (1, 2, 63, 64, 65):
        for n in sorted({1, 2, total}):
            lens = rng.multinomial(total, np.ones(n) / n)
            cases.append(("sorted", offsets_from_lengths(lens), total))
    for M in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 1):
        for mean in (1, 3, 1000):
            n = max(1, (M - 1) // (mean + 1))
            total = M - n - 1
            lens = rng.multinomial(total, np.ones(n) / n)
            cases.append(("sorted", offsets_from_lengths(lens), total))
    cases.append(("sorted", np.array([0, 3 * T + 7], dtype=np.uint32), 3 * T + 7))  # one segment
    cases.append(("sorted", np.arange(2 * T + 10, dtype=np.uint32), 2 * T + 9))  # every segment of length 1
    for run in (1, T - 1, T, T + 1, 3 * T + 5):  # empty segments: leading, interior (from a tile boundary of the merged sequence), trailing
        a = [0] * run + [5, 9]
        cases.append(("sorted", offsets_from_lengths(a), 14))
        cases.append(("sorted", offsets_from_lengths([5, 9] + [0] * run), 14))
        # interior: T - 2 positions and 2 offsets fill the first tile exactly, then `run` equal offsets
        cases.append(("sorted", offsets_from_lengths([T - 2] + [0] * run + [T + 3]), 2 * T + 1))
    # partial cover: head and tail uncovered; offsets[n] beyond total
    cases.append(("sorted", offsets_from_lengths([4, 0, T, 7], first=5), T + 40))
    cases.append(("sorted", offsets_from_lengths([4, 0, T, 700], first=5), T + 40))
    cases.append(("sorted", offsets_from_lengths([1, 2, 3], first=2 * T), T))  # nothing covered
    lens = rng.geometric(1 / 37.0, 4000) - 1
    cases.append(("sorted", offsets_from_lengths(lens), int(lens.sum())))
    # malformed
    for base in (offsets_from_lengths(rng.multinomial(3 * T, np.ones(500) / 500)), offsets_from_lengths(lens)):
        total = int(base[-1])
        cases.append(("malformed", rng.permutation(base).astype(np.uint32), total))
        beyond = base.copy()
        beyond[base.size // 2:] += np.uint32(2 * T)
        cases.append(("malformed", beyond, total))
        beyond = base.copy()
        beyond[3] = np.uint32(0xFFFFFFFF)
        beyond[-1] = np.uint32(0xFFFFFFF0)
        cases.append(("malformed", beyond, total))
        pair = base.copy()
        pair[[10, 11]] = pair[[11, 10]] + np.uint32([7, 0])
        cases.append(("malformed", pair, total))
        cases.append(("malformed", base[::-1].copy(), total))
        cases.append(("malformed", rng.integers(0, 2**32, base.size, dtype=np.uint32), total))
    return cases


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("expand_path")
    src = tmp / "expand_path.cpp"
    src.write_text(PROGRAM)
    cases = make_cases()
    infile = tmp / "cases.bin"
    with open(infile, "wb") as f:
        f.write(np.array([len(cases)], dtype=np.uint32).tobytes())
        for _, offsets, total in cases:
            f.write(np.array([offsets.size - 1, total], dtype=np.uint32).tobytes())
            f.write(offsets.tobytes())
    return tmp, src, cases, infile


def build_and_run(tmp, src, infile, name, flags):
    exe, outfile = tmp / name, tmp / (name + ".out")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    p = subprocess.run([str(exe), str(infile), str(outfile)], capture_output=True, text=True, timeout=600)
    return p, outfile


@pytest.fixture(scope="module")
def results(setup):
    tmp, src, cases, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "expand_path", [])
    raw = open(outfile, "rb").read()
    pos, out = 0, []

    def take(dtype, n):
        nonlocal pos
        v = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += v.nbytes
        return v

    tile = int(take(np.uint32, 1)[0])
    for _, offsets, total in cases:
        tiles = int(take(np.uint32, 1)[0])
        out.append({"tiles": tiles, "split": take(np.uint32, tiles + 1), "ranges": take(np.uint32, 4 * tiles).reshape(tiles, 4),
                    "seg": take(np.uint32, total), "rank": take(np.uint32, total), "item": take(np.uint32, total),
                    "written": take(np.uint32, total)})
    violations = int(take(np.uint64, 1)[0])
    assert pos == len(raw)
    return out, violations, p.returncode, tile


def oracle(offsets, total):
    n = offsets.size - 1
    s = np.searchsorted(offsets, np.arange(total), side="right") - 1
    return s, (s >= 0) & (s < n)


def test_no_index_leaves_its_bound_sorted_or_not(results):
    _, violations, returncode, tile = results
    assert violations == 0 and returncode == 0
    assert tile == header_tile()


def test_the_tile_ranges_cut_the_merged_sequence_exactly(setup, results):
    """Whatever the offsets hold: tile t's ranges start where tile t - 1's end, lie inside both sides and hold exactly its share of
    [0, M); no position is written twice."""
    _, _, cases, _ = setup
    out, _, _, T = results
    for (kind, offsets, total), r in zip(cases, out):
        na, M = offsets.size, offsets.size + total
        case = (kind, na - 1, total)
        assert r["tiles"] == -(-M // T), case
        assert r["split"][0] == 0 and r["split"][-1] == na, case
        end_a = end_b = 0
        for t in range(r["tiles"]):
            a0, a1, b0, b1 = (int(x) for x in r["ranges"][t])
            assert 0 <= a0 <= a1 <= na and 0 <= b0 <= b1 <= total, (case, t)
            assert (a1 - a0) + (b1 - b0) == min(T, M - t * T) and a0 + b0 == t * T, (case, t)
            if kind == "sorted":  # (malformed offsets: the clamp may let consecutive tiles disagree, never leave the arrays)
                assert a0 == end_a and b0 == end_b, (case, t)
            end_a, end_b = a1, b1
        if kind == "sorted":
            assert end_a == na and end_b == total, case
        assert (r["written"] <= 1).all(), case


def test_sorted_offsets_expand_as_numpy_searchsorted(setup, results):
    _, _, cases, _ = setup
    out, _, _, _ = results
    seen = 0
    for (kind, offsets, total), r in zip(cases, out):
        if kind != "sorted":
            continue
        seen += 1
        n = offsets.size - 1
        case = (n, total, offsets[:4].tolist())
        s, covered = oracle(offsets, total)
        assert (r["written"] == covered).all(), case
        sc = s[covered]
        assert (r["seg"][covered] == sc).all(), case
        assert (r["rank"][covered] == np.arange(total)[covered] - offsets[sc]).all(), case
        items = (np.arange(n, dtype=np.uint64) * 2654435761 + 17).astype(np.uint32)
        assert (r["item"][covered] == items[sc]).all(), case
        for name in ("seg", "rank", "item"):
            assert (r[name][~covered] == POISON).all(), (case, name)
    assert seen >= 50


def test_malformed_offsets_write_only_segments_below_n(setup, results):
    _, _, cases, _ = setup
    out, _, _, _ = results
    seen = 0
    for (kind, offsets, total), r in zip(cases, out):
        if kind != "malformed":
            continue
        seen += 1
        w = r["written"] == 1
        assert (r["seg"][w] < offsets.size - 1).all()
        assert (r["seg"][~w] == POISON).all() and (r["item"][~w] == POISON).all()
    assert seen == 12


def test_the_sanitized_stand_alone_program_runs_clean(setup):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly."""
    tmp, src, _, infile = setup
    p, _ = build_and_run(tmp, src, infile, "expand_path_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


def test_the_binding_states_the_headers_tile(built):
    assert built.plan_expand(1000, 10)[0] == header_tile()
    assert built.plan_expand(1, 1)[0] == header_tile()
