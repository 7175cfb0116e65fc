"""CPU test of the arithmetic of the batched sorted search (csrc/search_batch_walk.hpp): the needles of a tile, the tile's first and
last segment, the segment of a needle between them, the cover rule, the window decision, the clamps of a needle's haystack on both
paths and the equal-rows quotient.  The header is plain C++: a host program performs whole calls through its functions alone, tile by
tile as sorted_search_batch_kernels.hpp does (a vector of `window` keys stands in for LDS), at tile = 16 and window = 32 as well as at
the real sizes, and reports both outputs, how often each needle was written, how many tiles were staged and whether any index left its
array or the LDS vector.  Well-formed offsets are held against numpy.searchsorted per segment; shuffled, decreasing and out-of-range
offsets only against the promise that every index stays inside its array and every written position inside [0, hay_total].  The
same program, built with the address and undefined-behaviour sanitizers, runs the same cases as a stand-alone executable.  No device
needed."""
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
#include "search_batch_walk.hpp"
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

struct Header
{
    uint32_t num_segments, hay_total, needle_total, tile, window, lo, hay_form, needle_form, hay_count, needle_row;
};

static void one_case(const Header& h)
{
    const uint32_t S = h.num_segments;
    std::vector<uint32_t> hoff = get<uint32_t>(h.hay_form ? S + 1 : 0), noff = get<uint32_t>(h.needle_form ? S + 1 : 0);
    std::vector<uint64_t> hay = get<uint64_t>(h.hay_total), needles = get<uint64_t>(h.needle_total);
    std::vector<uint32_t> lower(h.needle_total, 0xA5A5A5A5u), upper(h.needle_total, 0xA5A5A5A5u), written(h.needle_total, 0);
    const SearchBatchRows rows = search_batch_make_rows(h.needle_row, h.hay_count);
    const uint64_t lo = h.lo, hi = (uint64_t) h.lo + h.needle_total;
    const uint32_t tiles = h.needle_total ? (uint32_t) ((hi + h.tile - 1) / h.tile) : 0u;
    uint32_t staged_tiles = 0, seen = 0;
    for (uint32_t t = 0; t < tiles && S; t++)
    {
        uint32_t j0, j1;
        if (!search_batch_tile_needles(t, h.tile, lo, hi, &j0, &j1)) continue;
        if (j0 >= j1 || j1 > h.needle_total) violations++;
        seen += j1 - j0;
        uint32_t s_first, s_last;
        if (h.needle_form)
        {
            const auto offset_at = [&](uint32_t i) { return at(noff, i); };
            s_first = search_batch_end_segment(j0, S, offset_at);
            s_last = search_batch_last_segment(s_first, search_batch_end_segment(j1 - 1u, S, offset_at));
        }
        else
        {
            s_first = search_batch_row(j0, rows, S);
            s_last = search_batch_row(j1 - 1u, rows, S);
        }
        if (s_first > s_last || s_last >= S)
        {
            violations++;
            continue;
        }
        const uint32_t w0 = h.hay_form ? at(hoff, s_first) : s_first * rows.hay_count;
        const uint32_t w1 = h.hay_form ? at(hoff, s_last + 1u) : (s_last + 1u) * rows.hay_count;
        const bool staged = search_batch_staged(w0, w1, h.hay_total, h.window);
        std::vector<uint64_t> lds(h.window, 0xDEADBEEFDEADBEEFull);
        if (staged)
        {
            staged_tiles++;
            for (uint32_t i = 0; i < w1 - w0; i++) at(lds, i) = at(hay, (uint64_t) w0 + i);
        }
        // every needle's range first, then the bounds with the trips of the longest range (the kernel: of the wave's longest)
        std::vector<uint32_t> base(j1 - j0), len(j1 - j0), live(j1 - j0);
        uint32_t longest = 0;
        for (uint32_t j = j0; j < j1; j++)
        {
            uint32_t seg;
            bool covered = true;
            if (h.needle_form)
            {
                const uint32_t c = search_batch_upper_bound(j, search_batch_inner_base(s_first), search_batch_inner_len(s_first, s_last),
                                                            search_batch_inner_steps(s_first, s_last), [&](uint32_t i) { return at(noff, i); });
                seg = search_batch_inner_segment(s_first, s_last, c);
                covered = search_batch_covered(j, at(noff, seg), at(noff, seg + 1u));
            }
            else
                seg = search_batch_row(j, rows, S);
            if (seg < s_first || seg > s_last) violations++;
            uint32_t begin = seg * rows.hay_count, count = rows.hay_count;
            if (h.hay_form) search_batch_offsets_segment(covered ? at(hoff, seg) : 0u, covered ? at(hoff, seg + 1u) : 0u, h.hay_total, &begin, &count);
            if (!covered) count = 0;
            uint32_t b, l;
            if (staged)
            {
                search_batch_window_range(begin, count, w0, w1, &b, &l);
                if ((uint64_t) b + l > w1 - w0) violations++;
            }
            else
            {
                search_batch_global_range(begin, count, h.hay_total, &b, &l);
                if ((uint64_t) b + l > h.hay_total) violations++;
            }
            base[j - j0] = b, len[j - j0] = l, live[j - j0] = covered;
            longest |= l;
        }
        const uint32_t steps = hist_steps(longest);
        for (uint32_t j = j0; j < j1; j++)
        {
            if (!live[j - j0]) continue;
            const auto key_at = [&](uint32_t i) { return staged ? at(lds, i) : at(hay, i); };
            const uint64_t x = at(needles, j);
            at(lower, j) = search_batch_bound<false, uint64_t>(x, base[j - j0], len[j - j0], steps, key_at);
            at(upper, j) = search_batch_bound<true, uint64_t>(x, base[j - j0], len[j - j0], steps, key_at);
            at(written, j)++;
        }
    }
    if (S && seen != h.needle_total) violations++; // the tiles hold every needle once
    put(lower);
    put(upper);
    put(written);
    put(std::vector<uint32_t>{tiles, staged_tiles});
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    in = fopen(argv[1], "rb");
    out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const uint32_t cases = get<uint32_t>(1)[0];
    put(std::vector<uint32_t>{search_batch_tile(4), search_batch_tile(8), search_batch_max_window(4), search_batch_max_window(8)});
    for (uint32_t c = 0; c < cases; c++)
    {
        const std::vector<uint32_t> w = get<uint32_t>(10);
        one_case(Header{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9]});
    }
    put(std::vector<uint64_t>{violations});
    fclose(in);
    fclose(out);
    printf("cases %u violations %llu\n", cases, violations);
    return violations ? 1 : 0;
}
"""

SIZES = ((16, 32), (2048, 8192), (1024, 4096))  # (tile, window): small, the real ones of 4-byte and of 8-byte keys


def offsets_from_lengths(lens, first=0):
    return (np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]) + first).astype(np.uint32)


def sorted_rows(rng, offsets, total, span):
    """`total` keys, sorted inside every segment of `offsets`, all from the same small range (so that a probe that leaks into a
    neighbouring segment changes the answer)."""
    hay = rng.integers(0, span, total, dtype=np.uint64)
    for b, e in zip(offsets[:-1], offsets[1:]):
        hay[b:e].sort()
    return hay


class Case:
    def __init__(self, kind, tile, window, lo, hay, needles, hay_offsets=None, needle_offsets=None, num_segments=None, hay_count=0,
                 needle_row=0):
        self.kind, self.tile, self.window, self.lo = kind, tile, window, lo
        self.hay, self.needles = np.asarray(hay, dtype=np.uint64), np.asarray(needles, dtype=np.uint64)
        self.hay_offsets, self.needle_offsets = hay_offsets, needle_offsets
        self.S = num_segments if num_segments is not None else (hay_offsets if hay_offsets is not None else needle_offsets).size - 1
        self.hay_count, self.needle_row = hay_count, needle_row

    def header(self):
        return np.array([self.S, self.hay.size, self.needles.size, self.tile, self.window, self.lo, self.hay_offsets is not None,
                         self.needle_offsets is not None, self.hay_count, self.needle_row], dtype=np.uint32)

    def segments(self):
        """[(hb, he, nb, ne)] of a well-formed case"""
        ho = self.hay_offsets if self.hay_offsets is not None else np.arange(self.S + 1, dtype=np.int64) * self.hay_count
        no = self.needle_offsets if self.needle_offsets is not None else np.arange(self.S + 1, dtype=np.int64) * self.needle_row
        return [(int(ho[s]), int(ho[s + 1]), int(no[s]), int(no[s + 1])) for s in range(self.S)]


LENGTHS = np.array([0, 1, 2, 15, 16, 17, 31, 32, 33, 100])


def make_cases():
    rng = np.random.default_rng(21)
    cases = []
    for tile, window in SIZES:
        scale = tile // 16
        for lo in (0, 1, 3):
            # equal partitions: rows of the same key range; the window holds a tile's rows, exactly, or not
            for S, n, m in ((7, 5, 3), (5, 2 * scale, 16 * scale), (3, window, tile), (3, window + 1, tile), (4, 3 * window, 2 * tile + 5),
                            (40, 0, 3), (1, 50, 2 * tile + 1)):
                ho = np.arange(S + 1, dtype=np.int64) * n
                hay = sorted_rows(rng, ho, S * n, 64)
                cases.append(Case("sorted", tile, window, lo, hay, rng.integers(0, 66, S * m, dtype=np.uint64), num_segments=S, hay_count=n,
                                  needle_row=m))
            # ragged, both offsets: lengths around the tile and the window, runs of empty segments, partial cover
            for trial in range(3):
                S = 60
                hl, nl = rng.choice(LENGTHS * scale, S), rng.choice(LENGTHS * scale, S)
                nl[20:45] = 0  # a run of segments without needles inside a tile
                hl[50:55] = 0  # needles with an empty haystack
                ho, no = offsets_from_lengths(hl), offsets_from_lengths(nl, first=(0, 5, 0)[trial])
                total_n = int(no[-1]) + (0, 9, 0)[trial]
                hay = sorted_rows(rng, ho, int(ho[-1]), 48)
                cases.append(Case("sorted", tile, window, lo, hay, rng.integers(0, 50, total_n, dtype=np.uint64), ho, no))
            # needle_offsets NULL over ragged haystacks; one segment; many empty segments around one needle each
            hl = rng.choice(LENGTHS * scale, 9)
            ho = offsets_from_lengths(hl)
            hay = sorted_rows(rng, ho, int(ho[-1]), 48)
            cases.append(Case("sorted", tile, window, lo, hay, rng.integers(0, 50, 9 * 37, dtype=np.uint64), ho, None, needle_row=37))
            cases.append(Case("sorted", tile, window, lo, np.sort(rng.integers(0, 90, 3 * tile + 1, dtype=np.uint64)),
                              rng.integers(0, 92, 2 * tile + 3, dtype=np.uint64), np.array([0, 3 * tile + 1], dtype=np.uint32),
                              np.array([0, 2 * tile + 3], dtype=np.uint32)))
            nl = np.zeros(3 * tile + 2, dtype=np.int64)
            nl[[0, tile + 1, 3 * tile + 1]] = (1, 2, 1)
            ho = offsets_from_lengths(np.full(nl.size, 2))
            cases.append(Case("sorted", tile, window, lo, sorted_rows(rng, ho, int(ho[-1]), 8), rng.integers(0, 9, 4, dtype=np.uint64), ho,
                              offsets_from_lengths(nl)))
        # malformed offsets on either side
        S = 80
        hl, nl = rng.choice(LENGTHS * scale, S), rng.choice(LENGTHS * scale, S)
        ho, no = offsets_from_lengths(hl), offsets_from_lengths(nl)
        hay = sorted_rows(rng, ho, int(ho[-1]), 48)
        needles = rng.integers(0, 50, int(no[-1]), dtype=np.uint64)

        def broken(o):
            yield rng.permutation(o).astype(np.uint32)
            yield o[::-1].copy()
            beyond = o.copy()
            beyond[S // 2:] += np.uint32(3 * tile)
            yield beyond
            wild = o.copy()
            wild[3] = np.uint32(0xFFFFFFFF)
            wild[-1] = np.uint32(0xFFFFFFF0)
            yield wild
            yield rng.integers(0, 2**32, o.size, dtype=np.uint32)
            yield np.full(o.size, 0xFFFFFFFF, dtype=np.uint32)

        for bad in broken(ho):
            cases.append(Case("malformed", tile, window, 1, hay, needles, bad, no))
        for bad in broken(no):
            cases.append(Case("malformed", tile, window, 2, hay, needles, ho, bad))
        for bad_h, bad_n in zip(broken(ho), broken(no)):
            cases.append(Case("malformed", tile, window, 0, hay, needles, bad_h, bad_n))
        for bad in broken(ho):  # equal needle rows over malformed haystack offsets
            cases.append(Case("malformed", tile, window, 3, hay, needles[:S * 4], bad, None, needle_row=4))
    return cases


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("search_batch_walk")
    src = tmp / "search_batch_walk.cpp"
    src.write_text(PROGRAM)
    cases = make_cases()
    infile = tmp / "cases.bin"
    with open(infile, "wb") as f:
        f.write(np.array([len(cases)], dtype=np.uint32).tobytes())
        for c in cases:
            f.write(c.header().tobytes())
            for a in (c.hay_offsets, c.needle_offsets, c.hay, c.needles):
                if a is not None:
                    f.write(a.tobytes())
    return tmp, src, cases, infile


def build_and_run(tmp, src, infile, name, flags):
    exe, outfile = tmp / name, tmp / (name + ".out")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    p = subprocess.run([str(exe), str(infile), str(outfile)], capture_output=True, text=True, timeout=600)
    return p, outfile


@pytest.fixture(scope="module")
def results(setup):
    tmp, src, cases, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "search_batch_walk", [])
    raw = open(outfile, "rb").read()
    pos, out = 0, []

    def take(dtype, n):
        nonlocal pos
        v = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += v.nbytes
        return v

    sizes = take(np.uint32, 4).tolist()
    for c in cases:
        n = c.needles.size
        r = {"lower": take(np.uint32, n), "upper": take(np.uint32, n), "written": take(np.uint32, n)}
        r["tiles"], r["staged"] = (int(v) for v in take(np.uint32, 2))
        out.append(r)
    violations = int(take(np.uint64, 1)[0])
    assert pos == len(raw)
    return out, violations, p, sizes


def test_no_index_leaves_its_array_or_the_window_sorted_or_not(setup, results):
    _, _, cases, _ = setup
    _, violations, p, sizes = results
    assert violations == 0 and p.returncode == 0 and p.stderr == ""
    assert p.stdout == "cases %d violations 0\n" % len(cases)
    assert sizes == [2048, 1024, 8192, 4096]
    assert sorted({(c.tile, c.window) for c in cases}) == sorted(SIZES)


def test_well_formed_offsets_search_as_numpy_per_segment(setup, results):
    _, _, cases, _ = setup
    out, _, _, _ = results
    seen = staged = unstaged = 0
    for c, r in zip(cases, out):
        if c.kind != "sorted":
            continue
        seen += 1
        name = (c.tile, c.window, c.lo, c.S, c.hay.size, c.needles.size)
        lower, upper = np.full(c.needles.size, POISON, dtype=np.uint32), np.full(c.needles.size, POISON, dtype=np.uint32)
        covered = np.zeros(c.needles.size, dtype=np.uint32)
        for hb, he, nb, ne in c.segments():
            lower[nb:ne] = np.searchsorted(c.hay[hb:he], c.needles[nb:ne], side="left")
            upper[nb:ne] = np.searchsorted(c.hay[hb:he], c.needles[nb:ne], side="right")
            covered[nb:ne] += 1
        assert (r["written"] == covered).all() and covered.max(initial=0) <= 1, name  # every covered needle once, the others never
        assert (r["lower"] == lower).all(), name
        assert (r["upper"] == upper).all(), name
        assert r["tiles"] == -(-(c.lo + c.needles.size) // c.tile), name
        staged += r["staged"]
        unstaged += r["tiles"] - r["staged"]
    assert seen >= 100 and staged > 100 and unstaged > 50  # both paths at every size


def test_the_window_decision_is_exact_at_its_edge(setup, results):
    """Rows of exactly `window` keys with one tile of needles each are staged; one key more and none is."""
    _, _, cases, _ = setup
    out, _, _, _ = results
    full = over = 0
    for c, r in zip(cases, out):
        if c.kind == "sorted" and c.hay_offsets is None and c.needle_row == c.tile and c.lo == 0:
            if c.hay_count == c.window:
                assert r["staged"] == r["tiles"] == c.S
                full += 1
            if c.hay_count == c.window + 1:
                assert r["staged"] == 0
                over += 1
    assert full == len(SIZES) and over == len(SIZES)


def test_malformed_offsets_write_positions_inside_the_haystack_at_most_once(setup, results):
    _, _, cases, _ = setup
    out, _, _, _ = results
    seen = 0
    for c, r in zip(cases, out):
        if c.kind != "malformed":
            continue
        seen += 1
        w = r["written"] == 1
        assert (r["written"] <= 1).all()
        assert (r["lower"][w] <= c.hay.size).all() and (r["upper"][w] <= c.hay.size).all()
        assert (r["lower"][~w] == POISON).all() and (r["upper"][~w] == POISON).all()
    assert seen == 24 * len(SIZES)


def test_the_sanitized_stand_alone_program_runs_clean(setup, results):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly; it
    prints the same line and leaves stderr empty."""
    tmp, src, _, infile = setup
    _, _, plain, _ = results
    p, outfile = build_and_run(tmp, src, infile, "search_batch_walk_san",
                               ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert p.stderr == "" and p.stdout == plain.stdout
    assert open(outfile, "rb").read() == open(tmp / "search_batch_walk.out", "rb").read()


def test_the_binding_states_the_headers_tile_and_window(built):
    assert built.plan_sorted_search_batch(5000, "uint32")[:3] == (2048, 3, 8192)
    assert built.plan_sorted_search_batch(5000, "float64")[:3] == (1024, 5, 4096)
