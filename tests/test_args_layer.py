"""CPU test of the argument rules the entry points share (csrc/glu_args.hpp).  The header is plain C++: a host program includes it,
supplies its own fail() that keeps the text, and holds (a) overlaps() and check_disjoint() against a brute-force intersection of byte
sets over every small (pointer or NULL, start, length), adjacent and empty arrays among them, in each of the three orders of
reporting; (b) check_aligned() against `%` for alignments 1, 4, 8 and 16; and prints what the other helpers answer, which is asserted
here.  The same program runs once more as a stand-alone executable under -fsanitize=address,undefined.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")

PROGRAM = r"""
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "glu_args.hpp"
using namespace glu_hip::host;

static std::string g_text;
static int g_fails = 0;
glu_status glu_hip::host::fail(glu_status code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_text = buf;
    g_fails++;
    return code;
}

static const uintptr_t kBase = 0x7F0000001000ull; // nothing is read through it
struct Small { bool null; unsigned start, len; };

static Array array_of(const Small& s, const char* name) { return Array{s.null ? nullptr : (const void*) (kBase + s.start), s.len, name}; }
// the bytes of an array as a bit set; a NULL array has none
static unsigned long long bytes_of(const Small& s) { return s.null ? 0ull : ((1ull << s.len) - 1) << s.start; }
static bool meet(const Small& a, const Small& b) { return (bytes_of(a) & bytes_of(b)) != 0; }

static std::string expected(const Small* o, const char* const* on, int no, const Small* in, const char* const* inn, int ni, OutputPairs pairs)
{
    for (int a = 0; a < no; a++)
    {
        if (pairs == kOutputsBeforeInputs)
            for (int b = a + 1; b < no; b++)
                if (meet(o[a], o[b])) return std::string(on[a]) + " overlaps " + on[b];
        for (int i = 0; i < ni; i++)
            if (meet(o[a], in[i])) return std::string(on[a]) + " overlaps " + inn[i];
    }
    if (pairs == kOutputsAfterInputs)
        for (int b = 0; b < no; b++)
            for (int a = 0; a < b; a++)
                if (meet(o[b], o[a])) return std::string(on[b]) + " overlaps " + on[a];
    return "";
}

int main()
{
    std::vector<Small> all;
    all.push_back(Small{true, 0, 3}); // NULL with a length: not given
    for (unsigned start = 0; start < 5; start++)
        for (unsigned len = 0; len < 4; len++) all.push_back(Small{false, start, len});
    // (a) two arrays
    unsigned long long pairs = 0, wrong = 0, adjacent = 0;
    for (const Small& a : all)
        for (const Small& b : all)
        {
            pairs++;
            if (overlaps(array_of(a, "a"), array_of(b, "b")) != meet(a, b)) wrong++;
            if (!a.null && !b.null && overlaps((const void*) (kBase + a.start), a.len, (const void*) (kBase + b.start), b.len) != meet(a, b)) wrong++;
            if (!a.null && !b.null && a.len && b.len && a.start + a.len == b.start)
            {
                adjacent++;
                if (overlaps(array_of(a, "a"), array_of(b, "b")) || overlaps(array_of(b, "b"), array_of(a, "a"))) wrong++;
            }
        }
    printf("pairs %llu adjacent %llu wrong %llu\n", pairs, adjacent, wrong);
    // two outputs against two inputs, every combination, in the three orders
    const char* on[2] = {"o0", "o1"};
    const char* inn[2] = {"i0", "i1"};
    unsigned long long calls = 0, refused = 0;
    wrong = 0;
    for (int mode = kOutputsMayOverlap; mode <= kOutputsBeforeInputs; mode++)
        for (const Small& o0 : all)
            for (const Small& o1 : all)
                for (const Small& i0 : all)
                    for (const Small& i1 : all)
                    {
                        const Small o[2] = {o0, o1}, in[2] = {i0, i1};
                        const std::string want = expected(o, on, 2, in, inn, 2, (OutputPairs) mode);
                        g_text.clear();
                        const int before = g_fails;
                        const glu_status st = check_disjoint({array_of(o0, on[0]), array_of(o1, on[1])}, {array_of(i0, inn[0]), array_of(i1, inn[1])},
                                                             (OutputPairs) mode);
                        calls++;
                        refused += st != GLU_OK;
                        if ((st == GLU_OK) != want.empty() || (st != GLU_OK && st != GLU_ERROR_INVALID_ARGUMENT) || g_text != want ||
                            g_fails - before != (want.empty() ? 0 : 1))
                            wrong++;
                    }
    printf("disjoint %llu refused %llu wrong %llu\n", calls, refused, wrong);
    // the order, spelled out: every array is the same eight bytes, so every pair overlaps and the first one is named
    const Array o0{(const void*) kBase, 8, "o0"}, o1{(const void*) kBase, 8, "o1"}, o2{(const void*) kBase, 8, "o2"}, i0{(const void*) kBase, 8, "i0"},
        i1{(const void*) kBase, 8, "i1"}, none{nullptr, 8, "none"}, empty{(const void*) kBase, 0, "empty"};
    const char* modes[3] = {"may_overlap", "after_inputs", "before_inputs"};
    for (int mode = 0; mode < 3; mode++)
    {
        const OutputPairs m = (OutputPairs) mode;
        g_text = "accepted";
        (void) check_disjoint({o0, o1, o2}, {i0, i1}, m);
        printf("order %s all: %s\n", modes[mode], g_text.c_str());
        g_text = "accepted";
        (void) check_disjoint({o0, o1, o2}, {none, empty}, m);
        printf("order %s outputs_only: %s\n", modes[mode], g_text.c_str());
        g_text = "accepted";
        (void) check_disjoint({none, o1, o2}, {empty, i1}, m);
        printf("order %s first_output_null: %s\n", modes[mode], g_text.c_str());
        g_text = "accepted";
        (void) check_disjoint({empty, none, o2}, {none, empty}, m);
        printf("order %s one_array: %s\n", modes[mode], g_text.c_str());
    }
    // (b) alignment
    calls = wrong = 0;
    for (size_t align : {1, 4, 8, 16})
        for (uintptr_t address = kBase; address < kBase + 40; address++)
        {
            g_text.clear();
            const glu_status st = check_aligned((const void*) address, align, "p", "the rule");
            calls++;
            if ((st != GLU_OK) != (address % align != 0) || (st != GLU_OK && (st != GLU_ERROR_INVALID_ARGUMENT || g_text != "p is not aligned to the rule")))
                wrong++;
            if (align == 4 && (check_aligned_4((const void*) address, "p") != GLU_OK) != (address % 4 != 0)) wrong++;
        }
    for (size_t align : {1, 4, 8, 16})
        if (check_aligned(nullptr, align, "p", "the rule") != GLU_OK) wrong++;
    printf("aligned %llu wrong %llu\n", calls, wrong);
    g_text.clear();
    (void) check_aligned_4((const void*) (kBase + 2), "out_vals");
    printf("text %s\n", g_text.c_str());
    g_text.clear();
    (void) check_items_aligned((const void*) (kBase + 8), (const void*) kBase, 32, bytes_text(item_align(32)));
    printf("text %s\n", g_text.c_str());
    g_text.clear();
    (void) check_items_aligned((const void*) kBase, (const void*) (kBase + 4), 8, "min(item_bytes, 16)");
    printf("text %s\n", g_text.c_str());
    printf("items_null %d\n", (int) check_items_aligned(nullptr, (const void*) (kBase + 1), 0, "unused"));
    // key types, items, limits, pointers, out-parameters
    for (int t = -1; t <= 6; t++)
    {
        g_text.clear();
        const glu_status st = check_key_type(t);
        printf("key %d %d %u %u [%s]\n", t, (int) st, key_bytes_of(t), key_xf_of(t), g_text.c_str());
    }
    for (uint32_t b : {0u, 1u, 4u, 8u, 12u, 16u, 32u, 64u})
    {
        g_text.clear();
        const glu_status st = check_item_bytes(b);
        printf("item %u %d %u [%s]\n", b, (int) st, item_align(b), g_text.c_str());
    }
    printf("bytes_text %s|%s|%s\n", bytes_text(4), bytes_text(8), bytes_text(16));
    for (size_t v : {(size_t) 0, ((size_t) 1 << 32) - 1, (size_t) 1 << 32})
    {
        g_text.clear();
        const glu_status a = check_below_2_32(v, "max_out");
        const std::string first = g_text;
        g_text.clear();
        const glu_status b = check_tile_count(v, "select takes a count below 2^32");
        printf("limit %zu %d [%s] %d [%s]\n", v, (int) a, first.c_str(), (int) b, g_text.c_str());
    }
    g_text.clear();
    printf("null %d %d [%s]\n", (int) check_not_null(&g_text, "merge"), (int) check_not_null(nullptr, "merge"), g_text.c_str());
    // several pointers under the caller's whole sentence: any NULL among them refuses, once, with that sentence and nothing added
    const void* const here = &g_text;
    const char* const sentence = "100%s / name is NULL"; // (not a format)
    int before = g_fails;
    const int none_null[5] = {(int) check_none_null({here}, sentence), (int) check_none_null({here, here, here}, sentence), (int) check_none_null({}, sentence),
                              (int) check_none_null({(const void*) nullptr}, sentence), g_fails - before};
    printf("none_null accepted %d %d %d refused %d fails %d [%s]\n", none_null[0], none_null[1], none_null[2], none_null[3], none_null[4], g_text.c_str());
    for (int at = 0; at < 3; at++)
    {
        g_text.clear();
        before = g_fails;
        const glu_status st = check_none_null({at == 0 ? nullptr : here, at == 1 ? nullptr : here, at == 2 ? nullptr : here}, "NULL array");
        printf("none_null at %d %d fails %d [%s]\n", at, (int) st, g_fails - before, g_text.c_str());
    }
    g_text.clear();
    before = g_fails;
    const glu_status all_null = check_none_null({nullptr, nullptr}, "NULL argument"); // (one refusal, not two)
    printf("none_null all %d fails %d [%s]\n", (int) all_null, g_fails - before, g_text.c_str());
    uint32_t word = 7;
    size_t wide = 7;
    store(&word, (size_t) 9);
    store(&wide, 11u);
    store((uint32_t*) nullptr, 13);
    printf("store %u %zu\n", word, wide);
    return 0;
}
"""


def build_and_run(tmp, name, flags):
    src = tmp / "args_layer.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           str(src)])
    return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("args_layer")


@pytest.fixture(scope="module")
def printed(tmp):
    p = build_and_run(tmp, "args_layer", [])
    assert p.returncode == 0, p.stderr
    return p.stdout.splitlines()


def lines(printed, kind):
    return [ln[len(kind) + 1:] for ln in printed if ln.startswith(kind + " ")]


def test_the_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "glu_args.hpp")).read()
    assert "hip/" not in text and "hip_runtime" not in text
    assert '#include "glu_args.hpp"' in open(os.path.join(CSRC, "glu_host.hpp")).read()


def test_overlap_is_the_intersection_of_the_byte_sets(printed):
    (pairs,) = lines(printed, "pairs")
    n = 1 + 5 * 4  # NULL, and five starts by four lengths
    count, _, adjacent, _, wrong = pairs.split()
    assert int(count) == n * n and int(adjacent) > 0 and int(wrong) == 0
    (disjoint,) = lines(printed, "disjoint")
    calls, _, refused, _, wrong = disjoint.split()
    assert int(calls) == 3 * n ** 4 and int(wrong) == 0 and 0 < int(refused) < int(calls)


def test_the_first_pair_is_reported_in_each_callers_order(printed):
    got = dict(ln.split(": ") for ln in lines(printed, "order"))
    # every output against every input comes first, outputs outermost -- except where an output looks at the outputs behind it first
    assert got["may_overlap all"] == got["after_inputs all"] == "o0 overlaps i0"
    assert got["before_inputs all"] == "o0 overlaps o1"
    # with no input in the way: nothing / the later output names the earlier (merge: "out_vals overlaps out_keys") / the earlier
    # names the later (expand: "out_segments overlaps out_ranks")
    assert got["may_overlap outputs_only"] == "accepted"
    assert got["after_inputs outputs_only"] == "o1 overlaps o0"
    assert got["before_inputs outputs_only"] == "o0 overlaps o1"
    # NULL and empty arrays are skipped
    assert got["may_overlap first_output_null"] == got["after_inputs first_output_null"] == "o1 overlaps i1"
    assert got["before_inputs first_output_null"] == "o1 overlaps o2"
    assert all(got[m + " one_array"] == "accepted" for m in ("may_overlap", "after_inputs", "before_inputs"))


def test_alignment_is_the_remainder(printed):
    (aligned,) = lines(printed, "aligned")
    assert aligned.split() == [str(4 * 40), "wrong", "0"]
    assert lines(printed, "text") == ["out_vals is not aligned to 4 bytes", "items is not aligned to 16 bytes",
                                      "out_items is not aligned to min(item_bytes, 16)"]
    assert lines(printed, "items_null") == ["0"]


def test_key_types_items_limits_and_out_parameters(printed):
    keys = lines(printed, "key")
    assert keys == ["-1 1 4 0 [Invalid key type: -1]", "0 0 4 0 []", "1 0 4 1 []", "2 0 4 2 []", "3 0 8 0 []", "4 0 8 1 []", "5 0 8 2 []",
                    "6 1 8 0 [Invalid key type: 6]"]
    items = lines(printed, "item")
    assert items == ["%d %d %d [%s]" % (b, 0 if b in (4, 8, 16, 32) else 1, min(b, 16),
                                        "" if b in (4, 8, 16, 32) else "item_bytes must be 4, 8, 16 or 32 (got %d)" % b)
                     for b in (0, 1, 4, 8, 12, 16, 32, 64)]
    assert lines(printed, "bytes_text") == ["4 bytes|8 bytes|16 bytes"]
    assert lines(printed, "limit") == ["0 0 [] 0 []", "4294967295 0 [] 0 []",
                                       "4294967296 1 [max_out must be below 2^32 (got 4294967296)] 1 [select takes a count below 2^32 (got 4294967296)]"]
    assert lines(printed, "null") == ["0 1 [merge is NULL]"]
    assert lines(printed, "none_null") == ["accepted 0 0 0 refused 1 fails 1 [100%s / name is NULL]", "at 0 1 fails 1 [NULL array]",
                                           "at 1 1 fails 1 [NULL array]", "at 2 1 fails 1 [NULL array]", "all 1 fails 1 [NULL argument]"]
    assert lines(printed, "store") == ["9 11"]


def test_each_rule_has_one_definition():
    """No unit keeps a private copy of what the layer provides."""
    array = "size_t bytes;\n    const char* name;"  # the {ptr, bytes, name} of the overlap tables
    found = {"key_bytes_of(": [], array: [], "check_key_type(int": [], "is not aligned to": []}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, name)).read().replace("        const char* name;", "    const char* name;")
            for needle in found:
                found[needle] += [name] * text.count(needle)
    assert found["check_key_type(int"] == ["glu_args.hpp"] and found[array] == ["glu_args.hpp"]
    assert [n for n in found["key_bytes_of("] if n == "glu_args.hpp"] == ["glu_args.hpp"]  # (one definition; the units only call it)
    assert not any("key_bytes_of(int" in open(os.path.join(CSRC, n)).read() or "key_bytes_of(glu_key_type" in open(os.path.join(CSRC, n)).read()
                   for n in set(found["key_bytes_of("]) - {"glu_args.hpp"})
    assert set(found["is not aligned to"]) <= {"glu_args.hpp", "glu_hip.hip"}, found["is not aligned to"]


def test_the_sanitized_stand_alone_program_runs_clean(tmp, printed):
    """the same program under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly"""
    p = build_and_run(tmp, "args_layer_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0 and p.stderr == "", p.stderr
    assert p.stdout.splitlines() == printed
