"""CPU test of the host arithmetic of the segmented sort (csrc/seg_plan.hpp): the sub-block descriptors of a pass (seg_build_image),
the pieces ordered by segment and the segment starts, the check that the pieces tile the input, and which arrays each pass reads and
writes.  The header is plain C++: a host program runs the functions on cases from a file and writes what they returned.  The expected
values come from a restatement of the rules written out here, and the structure of every image is asserted on its own.  The same
program, built with the address and undefined-behaviour sanitizers, runs the same cases as a stand-alone executable.  No device needed."""
import bisect
import itertools
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
M32 = 0xFFFFFFFF

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "seg_plan.hpp"
using namespace glu_hip;

static FILE* in;
static FILE* out;
static unsigned long long get()
{
    unsigned long long v = 0;
    if (fscanf(in, "%llu", &v) != 1) exit(3);
    return v;
}
// (on the heap, exactly as long as the list: the sanitizers see an access past its end)
static std::vector<SegPiece> get_pieces(size_t n)
{
    std::vector<SegPiece> pieces(n);
    for (SegPiece& pc : pieces)
    {
        pc.begin = get(), pc.len = get();
        pc.seg = (uint32_t) get();
    }
    pieces.shrink_to_fit();
    return pieces;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    in = fopen(argv[1], "r");
    out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    const unsigned long long cases = get();
    for (unsigned long long c = 0; c < cases; c++)
    {
        const unsigned kind = (unsigned) get();
        if (kind == 0) // an image: nwg nseg total npieces, the pieces (ordered by segment), seg_start[nseg + 1]
        {
            const uint32_t nwg = (uint32_t) get(), nseg = (uint32_t) get();
            const uint64_t total = get();
            const std::vector<SegPiece> pieces = get_pieces((size_t) get());
            std::vector<uint64_t> start((size_t) nseg + 1);
            for (uint64_t& s : start) s = get();
            SegImage img;
            seg_build_image(pieces.data(), pieces.size(), nseg, start.data(), total, nwg, img);
            fprintf(out, "%u %u %u %u %zu %zu %zu %zu", img.nsb, img.nwg, img.nseg, img.max_subs_per_wg, img.off_first, img.off_list, img.off_start,
                    img.words.size());
            for (uint32_t w : img.words) fprintf(out, " %u", w);
            fprintf(out, "\n");
        }
        else if (kind == 1) // the order and the starts: nseg origin npieces, the pieces
        {
            const uint32_t nseg = (uint32_t) get();
            const uint64_t origin = get();
            std::vector<SegPiece> pieces = get_pieces((size_t) get());
            std::vector<uint64_t> start;
            seg_order_pieces(pieces, nseg, origin, start);
            fprintf(out, "%zu %zu", pieces.size(), start.size());
            for (const SegPiece& pc : pieces) fprintf(out, " %llu %llu %u", (unsigned long long) pc.begin, (unsigned long long) pc.len, pc.seg);
            for (uint64_t s : start) fprintf(out, " %llu", (unsigned long long) s);
            fprintf(out, "\n");
        }
        else if (kind == 2) // do the pieces tile?  npieces, the pieces
        {
            const std::vector<SegPiece> pieces = get_pieces((size_t) get());
            const SegTiling t = seg_pieces_tile(pieces);
            fprintf(out, "%d %llu %d\n", t.tiles ? 1 : 0, (unsigned long long) t.element, t.twice ? 1 : 0);
        }
        else // the arrays of every pass: passes
        {
            const uint32_t passes = (uint32_t) get();
            for (uint32_t p = 0; p < passes; p++)
            {
                const SegPassArrays a = seg_pass_arrays(passes, p);
                fprintf(out, "%s%d %d", p ? " " : "", (int) a.src, (int) a.dst);
            }
            fprintf(out, "\n");
        }
    }
    fclose(in);
    fclose(out);
    return 0;
}
"""

# ---- the restatement -----------------------------------------------------------------------------------------------------------


def by_segment(pieces):
    """Pieces (begin, len, seg) in segment order; the caller's order among the pieces of a segment."""
    return [pc for g in sorted({pc[2] for pc in pieces}) for pc in pieces if pc[2] == g]


def starts(pieces, nseg, origin=0):
    out = [origin]
    for g in range(nseg):
        out.append(out[-1] + sum(l for _, l, s in pieces if s == g))
    return out


def image_words(pieces, nseg, seg_start, total, nwg):
    """The rules: the pieces laid end to end are dealt to the workgroups in shares of ceil(total / nwg) elements (at least 1); a sub-block
    is the part of one piece inside one share.  Words: the sub-blocks as (begin, end), the first sub-block of every workgroup and the
    end, the first sub-block of every segment and the end, the segment starts; all as 32-bit words, padded to an even count."""
    share = max(1, -(-total // nwg))
    subs, per_wg, pos = [], [0] * nwg, 0
    for begin, length, seg in pieces:
        lo = pos
        while lo < pos + length:
            hi = min(pos + length, (lo // share + 1) * share)
            subs.append((begin + lo - pos, begin + hi - pos, seg))
            per_wg[min(lo // share, nwg - 1)] += 1
            lo = hi
        pos += length
    wg_first = [0] + list(itertools.accumulate(per_wg))
    sub_segs = [s[2] for s in subs]  # (ascending: the pieces come ordered by segment)
    seg_first = [bisect.bisect_left(sub_segs, g) for g in range(nseg + 1)]  # how many sub-blocks belong to lower segments
    words = [x & M32 for b, e, _ in subs for x in (b, e)] + wg_first + seg_first + [s & M32 for s in seg_start[:nseg]]
    return words + [0] * (len(words) % 2), len(subs), max(per_wg), subs


def first_bad_element(pieces):
    """None: every element below the end of the pieces lies in exactly one; else (element, in more than one?)."""
    end = max([b + l for b, l, _ in pieces if l] + [0])
    cover = [0] * end
    for b, l, _ in pieces:
        for e in range(b, b + l):
            cover[e] += 1
    for e, c in enumerate(cover):
        if c != 1:
            return e, c > 1
    return None


# ---- the cases -----------------------------------------------------------------------------------------------------------------


def tiled(lens_and_segs, rng=None):
    """Pieces of these (len, seg) that tile [0, total) -- in address order, or dealt to addresses in a shuffled order."""
    order = list(range(len(lens_and_segs)))
    if rng:
        rng.shuffle(order)
    begin, at = {}, 0
    for i in order:
        begin[i] = at
        at += lens_and_segs[i][0]
    return [(begin[i], l, s) for i, (l, s) in enumerate(lens_and_segs)]


def image_case(pieces, nseg, nwg, origin=0):
    pieces = by_segment(pieces)
    return (pieces, nseg, starts(pieces, nseg, origin), sum(l for _, l, _ in pieces), nwg)


IMAGE_CASES = {
    "no pieces": image_case([], 3, 4),
    "all lengths zero": image_case([(0, 0, 0), (5, 0, 2), (9, 0, 2)], 3, 4),
    "total < nwg": image_case(tiled([(2, 0), (1, 1), (2, 1)]), 2, 7),
    "nwg = 1": image_case(tiled([(100, 0), (0, 1), (250, 1), (3, 2)]), 3, 1),
    "one piece spanning every workgroup": image_case([(0, 1_000_003, 0)], 1, 256),
    "a segment with no piece between two that have some": image_case(tiled([(700, 0), (900, 2), (50, 0), (1, 2)]), 3, 3),
    "a piece whose begin + len is 0xFFFF0000": image_case([(0xFFFF0000 - 4000, 4000, 1), (0, 3000, 0), (3000, 1234, 1)], 2, 7),
    "nseg = 1": image_case(tiled([(1500, 0), (1, 0), (4999, 0)]), 1, 3),
    "nseg = 40": image_case(tiled([(37 * (g % 5) + g, (g * 7) % 40) for g in range(40)]), 40, 7),
    "the later passes of a plan with an origin: whole segments": image_case([(5000, 300, 0), (5300, 0, 1), (5300, 4100, 2)], 3, 2, origin=5000),
    "an exact multiple of the share": image_case(tiled([(512, 0), (512, 1), (1024, 2)]), 3, 4),
}
RANDOM_IMAGES = 2000


def random_image_case(seed):
    rng = random.Random(seed)
    nwg, nseg = rng.choice([1, 2, 3, 7, 256]), rng.randint(1, 40)
    top = rng.choice([0, 1, 40, 5000, 5000])  # (short pieces too: shares of a few elements, many pieces in one share)
    shape = [(rng.randint(0, top), rng.randrange(nseg)) for _ in range(rng.randint(0, 200))]
    return image_case(tiled(shape, rng), nseg, nwg)


ORDER_CASES = {
    # (distinct begins: the order of equal-segment pieces shows)
    "equal-segment pieces keep the caller's order": ([(40, 5, 2), (30, 7, 0), (20, 1, 2), (10, 9, 0), (0, 3, 2), (50, 0, 1)], 3, 0),
    "a non-zero origin": ([(40, 5, 2), (30, 7, 0), (20, 1, 2), (10, 9, 0), (0, 3, 3)], 5, 1_000_000),
    "an origin past 2^32": ([(7, 11, 1), (0, 7, 0)], 2, (1 << 33) + 5),
    "no pieces": ([], 4, 17),
    "no segments": ([], 0, 3),
}

TILING_CASES = {
    "an exact tiling in shuffled order": tiled([(5, 0), (1, 1), (300, 0), (17, 2), (2, 1)], random.Random(4)),
    "an exact tiling in address order": tiled([(5, 0), (1, 1), (300, 0)]),
    "a gap": [(0, 5, 0), (7, 3, 0), (10, 4, 1)],
    "a gap at the front": [(2, 5, 0), (7, 3, 0)],
    "an overlap": [(6, 4, 1), (0, 5, 0), (3, 3, 0)],
    "one piece inside another": [(0, 10, 0), (4, 2, 1), (10, 5, 0)],
    "the same piece twice": [(0, 4, 0), (4, 4, 0), (4, 4, 1)],
    "an overlap before a gap": [(0, 5, 0), (4, 2, 0), (9, 1, 0)],
    "a gap before an overlap": [(0, 5, 0), (6, 4, 0), (8, 1, 0)],
    "zero-length pieces anywhere": [(0, 0, 0), (0, 5, 0), (3, 0, 1), (5, 4, 1), (9, 0, 0), (1000, 0, 2)],
    "zero-length pieces around a gap": [(0, 5, 0), (5, 0, 1), (6, 0, 1), (6, 2, 1)],
    "only zero-length pieces": [(3, 0, 0), (9, 0, 1)],
    "no pieces": [],
}

PASS_COUNTS = (1, 2, 3, 4)
IN, OUT, SCRATCH = 0, 1, 2


def case_lines():
    def pieces_text(pieces):
        return " ".join("%d %d %d" % pc for pc in pieces)

    images = list(IMAGE_CASES.values()) + [random_image_case(seed) for seed in range(RANDOM_IMAGES)]
    lines = []
    for pieces, nseg, seg_start, total, nwg in images:
        lines.append("0 %d %d %d %d %s %s" % (nwg, nseg, total, len(pieces), pieces_text(pieces), " ".join(str(s) for s in seg_start)))
    for pieces, nseg, origin in ORDER_CASES.values():
        lines.append("1 %d %d %d %s" % (nseg, origin, len(pieces), pieces_text(pieces)))
    for pieces in TILING_CASES.values():
        lines.append("2 %d %s" % (len(pieces), pieces_text(pieces)))
    for passes in PASS_COUNTS:
        lines.append("3 %d" % passes)
    return images, lines


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("seg_plan")
    src = tmp / "seg_plan.cpp"
    src.write_text(PROGRAM)
    images, lines = case_lines()
    infile = tmp / "cases.txt"
    infile.write_text("%d\n" % len(lines) + "\n".join(lines) + "\n")
    return tmp, src, infile, images


def build_and_run(tmp, src, infile, name, flags):
    exe, outfile = tmp / name, tmp / (name + ".out")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    p = subprocess.run([str(exe), str(infile), str(outfile)], capture_output=True, text=True, timeout=600)
    return p, outfile


@pytest.fixture(scope="module")
def results(setup):
    """The program's output: one row of numbers per case, in the order of the case file."""
    tmp, src, infile, images = setup
    p, outfile = build_and_run(tmp, src, infile, "seg_plan", [])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rows = [[int(x) for x in line.split()] for line in open(outfile).read().splitlines()]
    assert len(rows) == len(images) + len(ORDER_CASES) + len(TILING_CASES) + len(PASS_COUNTS)
    return rows


def check_image(case, row):
    pieces, nseg, seg_start, total, nwg = case
    nsb, got_nwg, got_nseg, max_subs, off_first, off_list, off_start, nwords = row[:8]
    words = row[8:]
    # word for word against the restatement
    want_words, want_nsb, want_max, want_subs = image_words(pieces, nseg, seg_start, total, nwg)
    assert (nsb, got_nwg, got_nseg, max_subs) == (want_nsb, nwg, nseg, want_max)
    assert (off_first, off_list, off_start) == (2 * nsb, 2 * nsb + nwg + 1, 2 * nsb + nwg + 1 + nseg + 1)
    assert nwords == len(words) and words == want_words
    # the structure itself
    assert nwords % 2 == 0 and nwords - (off_start + nseg) in (0, 1)
    subs = [(words[2 * i], words[2 * i + 1]) for i in range(nsb)]
    wg_first, seg_first = words[off_first:off_list], words[off_list:off_start]
    share = max(1, -(-total // nwg))
    at, pos, sub_seg = 0, 0, []
    for begin, length, seg in pieces:  # the sub-blocks of a piece partition it in order
        here = begin
        while here < begin + length:
            b, e = subs[at]
            assert b == here & M32 and 0 < e - b <= begin + length - here, (at, b, e, here)
            lo, hi = pos + here - begin, pos + here - begin + (e - b)  # (in the pieces laid end to end)
            assert lo // share == (hi - 1) // share, "a sub-block crosses a multiple of the share"
            sub_seg.append(seg)
            here += e - b
            at += 1
        pos += length
    assert at == nsb and pos == total
    assert wg_first[0] == 0 and wg_first[nwg] == nsb and all(a <= b for a, b in zip(wg_first, wg_first[1:]))
    assert max_subs == max(b - a for a, b in zip(wg_first, wg_first[1:]))
    assert seg_first[nseg] == nsb
    assert all(a <= b for a, b in zip(sub_seg, sub_seg[1:]))
    for g in range(nseg):  # the first sub-block of segment g: the one before it belongs to a lower segment, the one there does not
        f = seg_first[g]
        assert (f == 0 or sub_seg[f - 1] < g) and (f == nsb or sub_seg[f] >= g), (g, f)
    assert words[off_start:off_start + nseg] == [s & M32 for s in seg_start[:nseg]]


@pytest.mark.parametrize("name", list(IMAGE_CASES))
def test_image_of_a_hand_written_case(setup, results, name):
    index = list(IMAGE_CASES).index(name)
    check_image(setup[3][index], results[index])


def test_images_of_seeded_random_cases(setup, results):
    images = setup[3]
    assert len(images) - len(IMAGE_CASES) >= 2000
    seen_nwg = set()
    for index in range(len(IMAGE_CASES), len(images)):
        check_image(images[index], results[index])
        seen_nwg.add(images[index][4])
    assert seen_nwg == {1, 2, 3, 7, 256}


def test_the_hand_written_images_are_the_cases_they_name(setup, results):
    """(what the names promise, so that a case cannot quietly stop reaching its edge)"""
    rows = dict(zip(IMAGE_CASES, results))
    cases = dict(zip(IMAGE_CASES, setup[3]))
    assert rows["no pieces"][0] == 0 and rows["all lengths zero"][0] == 0
    assert cases["total < nwg"][3] < cases["total < nwg"][4]
    assert rows["one piece spanning every workgroup"][0] == 256 and rows["one piece spanning every workgroup"][3] == 1
    seg_first = rows["a segment with no piece between two that have some"]
    off_list = seg_first[5]
    assert seg_first[8 + off_list + 1] == seg_first[8 + off_list + 2] != seg_first[8 + off_list]  # segment 1 is empty, 0 is not
    far = rows["a piece whose begin + len is 0xFFFF0000"]
    assert 0xFFFF0000 in far[8:8 + 2 * far[0]]
    assert rows["nseg = 1"][2] == 1 and rows["nseg = 40"][2] == 40


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_order_and_starts(setup, results, name):
    pieces, nseg, origin = ORDER_CASES[name]
    row = results[len(setup[3]) + list(ORDER_CASES).index(name)]
    assert row[:2] == [len(pieces), nseg + 1]
    got = [tuple(row[2 + 3 * i:5 + 3 * i]) for i in range(len(pieces))]
    assert got == by_segment(pieces), name
    assert row[2 + 3 * len(pieces):] == starts(pieces, nseg, origin), name
    assert row[2 + 3 * len(pieces)] == origin


def test_the_order_cases_have_something_to_keep():
    pieces, _, _ = ORDER_CASES["equal-segment pieces keep the caller's order"]
    assert by_segment(pieces) != sorted(pieces, key=lambda pc: (pc[2], pc[0])) and by_segment(pieces) != pieces


@pytest.mark.parametrize("name", list(TILING_CASES))
def test_tiling_check(setup, results, name):
    pieces = TILING_CASES[name]
    row = results[len(setup[3]) + len(ORDER_CASES) + list(TILING_CASES).index(name)]
    bad = first_bad_element(pieces)
    if bad is None:
        assert row == [1, 0, 0], name
    else:
        assert row == [0, bad[0], 1 if bad[1] else 0], name
    want = {"a gap": (5, False), "a gap at the front": (0, False), "an overlap": (3, True), "one piece inside another": (4, True),
            "the same piece twice": (4, True), "an overlap before a gap": (4, True), "a gap before an overlap": (5, False),
            "zero-length pieces around a gap": (5, False)}.get(name)
    assert bad == want, name


@pytest.mark.parametrize("passes", PASS_COUNTS)
def test_pass_arrays(setup, results, passes):
    row = results[len(setup[3]) + len(ORDER_CASES) + len(TILING_CASES) + PASS_COUNTS.index(passes)]
    arrays = [(row[2 * p], row[2 * p + 1]) for p in range(passes)]
    assert len(row) == 2 * passes
    assert arrays[0][0] == IN and arrays[-1][1] == OUT
    assert all(src != dst for src, dst in arrays)
    assert all(arrays[p][0] == arrays[p - 1][1] for p in range(1, passes))
    used = {a for pair in arrays for a in pair}
    assert (SCRATCH in used) == (passes % 2 == 0)
    assert arrays == {1: [(IN, OUT)], 2: [(IN, SCRATCH), (SCRATCH, OUT)], 3: [(IN, OUT), (OUT, IN), (IN, OUT)],
                      4: [(IN, SCRATCH), (SCRATCH, IN), (IN, SCRATCH), (SCRATCH, OUT)]}[passes]


def test_the_sanitized_stand_alone_program_runs_clean(setup, results):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly; it
    writes what the plain build wrote."""
    tmp, src, infile, _ = setup
    p, outfile = build_and_run(tmp, src, infile, "seg_plan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert [[int(x) for x in line.split()] for line in open(outfile).read().splitlines()] == results
