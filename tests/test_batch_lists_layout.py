"""CPU test of the segment lists the three batched operators share (csrc/batch_lists.hpp): where the lists of a call with device
offsets lie and how many entries each holds.  batch_lists_layout is plain C++: a host program prints it for the three operators'
class tables over a grid of sizes, and the rule stated in the header is recomputed here.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")

TOTALS = [0, 1, 2, 511, 512, 513, 16384, 65536, 65537, 1 << 20, (1 << 32) - 1]
SEGMENTS = [1, 7, 1 << 24]
LONG, CHUNKS = 4, 5


def tables():
    """(operator, element or key bytes) -> (shortest listed length, the four class limits, chunk, wide): what classes_of() of
    glu_sort_batch.hip, glu_reduce_batch.hip and glu_scan_batch.hip return, in elements."""
    t = {}
    for kb in (4, 8):
        t["sort", kb] = (2, [512, 1024, 4096, 16384 if kb == 4 else 8192], 0, False)
    for es in (4, 8, 16, 32):
        t["reduce", es] = (1, [16, 64, 4096 // es, (256 << 10) // es], (256 << 10) // es, True)
        t["scan", es] = (1, [128 // es, 512 // es, 2048 // es, (64 << 10) // es], (32 << 10) // es, True)
    return t


def expected(table, total, num_segments):
    """The rule of batch_lists.hpp: list c holds min(num_segments, total / shortest length of its class) entries; the lists lie back
    to back, an 8-byte list from an even word on; the chunk list holds total / chunk + long capacity entries, none when the long
    list holds none."""
    shortest, limit, chunk, wide = table
    at, start, capacity = 0, [], []
    for c in range(LONG + 1):
        entry_words = 2 if c == LONG and wide else 1
        at = (at + entry_words - 1) // entry_words * entry_words
        start.append(at)
        capacity.append(min(num_segments, total // (shortest if c == 0 else limit[c - 1] + 1)))
        at += entry_words * capacity[c]
    start.append(at)
    capacity.append(total // chunk + capacity[LONG] if chunk and capacity[LONG] else 0)
    return start, capacity, list(limit), chunk, at + 2 * capacity[CHUNKS]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{(operator, bytes, total, num_segments): (start, capacity, limit, chunk, words)} as the header computes them."""
    tmp = tmp_path_factory.mktemp("batch_lists")
    rows = ["    {%d, {%d, {%s}, %d, %s}}," % (i, t[0], ", ".join(map(str, t[1])), t[2], "true" if t[3] else "false")
            for i, t in enumerate(tables().values())]
    src = tmp / "layout.cpp"
    src.write_text('#include <cstdio>\n'
                   '#include "batch_lists.hpp"\n'
                   "using namespace glu_hip;\n"
                   "struct Row { int id; BatchClasses classes; };\n"
                   "static const Row rows[] = {\n" + "\n".join(rows) + "\n};\n"
                   "static const size_t totals[] = {%s};\n" % ", ".join("%dull" % v for v in TOTALS) +
                   "static const size_t segments[] = {%s};\n" % ", ".join("%dull" % v for v in SEGMENTS) +
                   "int main()\n"
                   "{\n"
                   "    static_assert(sizeof(size_t) == 8, \"the layout counts words in 64 bits\");\n"
                   "    for (const Row& r : rows)\n"
                   "        for (size_t total : totals)\n"
                   "            for (size_t n : segments)\n"
                   "            {\n"
                   "                size_t words;\n"
                   "                const BatchListsLayout l = batch_lists_layout(r.classes, total, n, words);\n"
                   '                printf("%d %zu %zu", r.id, total, n);\n'
                   '                for (int c = 0; c < BATCH_LISTS; c++) printf(" %u", l.start[c]);\n'
                   '                for (int c = 0; c < BATCH_LISTS; c++) printf(" %u", l.capacity[c]);\n'
                   '                for (int c = 0; c < 4; c++) printf(" %u", l.limit[c]);\n'
                   '                printf(" %u %zu\\n", l.chunk, words);\n'
                   "            }\n"
                   "    return 0;\n"
                   "}\n")
    exe = tmp / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    keys = list(tables())
    out = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        v = [int(x) for x in line.split()]
        out[keys[v[0]] + (v[1], v[2])] = (v[3:9], v[9:15], v[15:19], v[19], v[20])
    return out


def test_every_layout_follows_the_rule_of_the_header(printed):
    assert len(printed) == len(tables()) * len(TOTALS) * len(SEGMENTS)
    for (op, nbytes, total, n), got in printed.items():
        want = expected(tables()[op, nbytes], total, n)
        assert got == want, (op, nbytes, total, n, got, want)


def test_no_two_lists_overlap_and_the_sizes_fit_their_types(printed):
    for (op, nbytes, total, n), (start, capacity, _, _, words) in printed.items():
        wide = tables()[op, nbytes][3]
        end = 0
        for c in range(CHUNKS + 1):
            entry_words = 2 if wide and c >= LONG else 1
            assert start[c] >= end and start[c] % entry_words == 0, (op, nbytes, total, n, c)
            end = start[c] + entry_words * capacity[c]
        assert end == words and words * 4 < 1 << 64, (op, nbytes, total, n)
        # (equal to the unbounded numbers of expected(): nothing was cut to 32 bits on the way)
        assert all(v < 1 << 32 for v in start + capacity), (op, nbytes, total, n)
    assert ("reduce", 4, (1 << 32) - 1, 1 << 24) in printed and ("sort", 8, (1 << 32) - 1, 1 << 24) in printed


def test_the_tables_are_the_operators_class_limits(built):
    """The limits above against the pure plan functions of the library: the last length of a class and the first of the next."""
    t = tables()
    for kb in (4, 8):
        limit = t["sort", kb][1]
        assert built.plan_batch(1, kb)[0] == 0 and built.plan_batch(2, kb)[0] == 1  # (shorter segments are in no list)
        assert built.plan_batch(limit[0], kb) == (1, limit[0]) and built.plan_batch(limit[0] + 1, kb) == (2, limit[1])
        for c in (1, 2):
            assert built.plan_batch(limit[c], kb) == (2, limit[c]) and built.plan_batch(limit[c] + 1, kb) == (2, limit[c + 1])
        assert built.plan_batch(limit[3], kb) == (2, limit[3]) and built.plan_batch(limit[3] + 1, kb)[0] == 3
    for op, plan in (("reduce", built.plan_reduce_batch), ("scan", built.plan_scan_batch)):
        for es in (4, 8, 16, 32):
            _, limit, chunk, _ = t[op, es]
            assert limit[0] < limit[1] < limit[2] < limit[3]
            assert plan(0, es)[0] == 0 and plan(1, es)[0] == 1
            assert plan(limit[2], es) == (1, 1) and plan(limit[2] + 1, es) == (2, 1)
            assert plan(limit[3], es) == (2, 1) and plan(limit[3] + 1, es) == (3, -(-(limit[3] + 1) // chunk))
            assert plan(7 * chunk + 1, es) == (3, 8)
