"""CPU tests of the plan of batched top-k (csrc/topk_batch_plan.hpp).  The header is plain C++: a host program runs whole selects over
segments through its digit windows at both widths (8 bits: the wave class; 11 bits: the workgroup classes, where it must agree with
topk_pick.hpp's own functions), vectors standing in for the counters in LDS, compacts as the kernels do, pads a row of pairs and
orders it with a stable sort as the sorted stage does.  Held against numpy.argsort(code, kind="stable")[:min(k, len)].  After every
round 1 <= need <= count[d], at the end less + need == k_s.  The same program, built with the address and undefined-behaviour
sanitizers, runs the same cases as a stand-alone executable.  Through ctypes: glu_top_k_plan_batch's classes, paths, kernel counts and
refusals; the list layout of the top-k classes never overflows for non-decreasing offsets.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

from test_top_k_pick import key_code, make_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>
#include "topk_batch_plan.hpp"
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

template<typename K>
static void one_case(uint32_t n, uint32_t k, uint32_t width)
{
    const std::vector<K> code = get<K>(n);
    const uint32_t kb = sizeof(K), rounds = topk_rounds_w(kb, width), k_s = k < n ? k : n;
    if (width == kTopkDigitBits && rounds != topk_rounds(kb)) violations++;
    TopkState s = topk_begin(n, k_s);
    uint32_t covered = 0;
    for (uint32_t r = 0; r < rounds; r++)
    {
        const uint32_t shift = topk_shift_w(kb, width, r), bits = topk_bits_w(kb, width, r);
        if (bits == 0 || bits > width || shift + bits + covered != 8 * kb) violations++; // the windows tile the word from the top
        covered += bits;
        if (width == kTopkDigitBits && (shift != topk_shift(kb, r) || bits != topk_bits(kb, r))) violations++;
        std::vector<uint32_t> table(1u << width, 0);
        for (K c : code)
            if (topk_matches(s, c)) table[topk_digit(c, shift, bits)]++;
        uint32_t before = 0;
        const uint32_t d = topk_find_digit(1u << width, s.need, [&](uint32_t i) { return table[i]; }, &before);
        uint32_t crossing = 0, run = 0; // every counter at once, as the device asks: exactly the one crossing
        for (uint32_t i = 0; i < (1u << width); i++)
        {
            if (topk_crosses(run, table[i], s.need))
            {
                crossing++;
                if (i != d || run != before) violations++;
            }
            run += table[i];
        }
        if (crossing != 1) violations++;
        topk_advance_w(s, kb, width, r, d, before, table[d]);
        if (s.need < 1 || s.need > s.bucket) violations++; // 1 <= need <= count[d]
    }
    if (covered != 8 * kb || s.less + s.need != k_s) violations++;
    if (s.mask != (kb == 4 ? 0xFFFFFFFFull : ~0ull)) violations++;
    // the compaction into a row of k pairs: every word below the threshold and the first `need` equal to it, at
    // less_before + min(ties_before, need); the pads behind k_s
    std::vector<K> row_code(k, (K) 0x5A);
    std::vector<uint32_t> row_index(k, 0xA5A5A5A5u), written(k_s, 0);
    uint32_t less_before = 0, ties_before = 0;
    for (uint32_t i = 0; i < n; i++)
    {
        const bool is_less = code[i] < (K) s.prefix, is_tie = code[i] == (K) s.prefix;
        const uint32_t rank = less_before + (ties_before < s.need ? ties_before : s.need);
        if (is_less || (is_tie && ties_before < s.need))
        {
            if (rank >= k_s)
                violations++;
            else
            {
                row_code[rank] = code[i];
                row_index[rank] = i;
                written[rank]++;
            }
        }
        less_before += is_less;
        ties_before += is_tie;
    }
    for (uint32_t w : written)
        if (w != 1) violations++;
    for (uint32_t j = k_s; j < k; j++)
    {
        row_code[j] = (K) ~(K) 0;
        row_index[j] = j;
    }
    // the sorted stage: a stable sort by the code word keeps the pads behind the real entries, real all-ones codes among them
    std::vector<uint32_t> order(k);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return row_code[a] < row_code[b]; });
    std::vector<uint32_t> sorted_index(k);
    for (uint32_t j = 0; j < k; j++)
    {
        sorted_index[j] = row_index[order[j]];
        if ((j < k_s) != (order[j] < k_s)) violations++;
    }
    put(std::vector<uint64_t>{s.prefix});
    put(std::vector<uint32_t>{s.less, s.need, s.bucket});
    put(row_index);
    put(sorted_index);
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
        const std::vector<uint32_t> h = get<uint32_t>(4); // key_bytes, n, k, width
        if (h[0] == 4) one_case<uint32_t>(h[1], h[2], h[3]);
        else one_case<uint64_t>(h[1], h[2], h[3]);
    }
    // the classes: every length has one, the limits are its last members, 8-byte tiles hold half the keys
    for (uint32_t kb = 4; kb <= 8; kb += 4)
        for (int c = 0; c < BATCH_LIST_LONG; c++)
        {
            const uint32_t limit = topk_batch_limit(c, kb);
            if (topk_batch_class(limit, kb) != c || topk_batch_class((uint64_t) limit + 1, kb) != c + 1) violations++;
            if (c > 0 && (limit <= topk_batch_limit(c - 1, kb) || topk_batch_limit(c, 8) * 2 != topk_batch_limit(c, 4))) violations++;
        }
    if (topk_batch_class(1, 4) != 0 || topk_batch_classes(4).shortest != 1 || kTopkBatchWaveTile != 64 * kTopkBatchWaveKpt) violations++;
    put(std::vector<uint64_t>{violations});
    fclose(in);
    fclose(out);
    return violations ? 1 : 0;
}
"""

LAYOUT_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "topk_batch_plan.hpp"
using namespace glu_hip;

// random batches with non-decreasing offsets: no list of the top-k classes receives more segments than it holds, the lists lie back
// to back inside `words`
int main()
{
    std::mt19937_64 rng(7);
    unsigned long long violations = 0;
    for (uint32_t kb = 4; kb <= 8; kb += 4)
        for (int trial = 0; trial < 400; trial++)
        {
            const BatchClasses cls = topk_batch_classes(kb);
            const size_t nseg = 1 + rng() % 3000;
            const uint32_t scale = trial % 4 == 0 ? 4 * cls.limit[3] : trial % 4 == 1 ? 3 : trial % 4 == 2 ? cls.limit[1] : cls.limit[0];
            std::vector<size_t> len(nseg);
            size_t total = 0;
            for (size_t& n : len)
            {
                n = rng() % 5 == 0 ? 0 : (size_t) (rng() % scale);
                if (rng() % 50 == 0) n = cls.limit[rng() % 4] + rng() % 2;
                total += n;
            }
            total += rng() % 3;
            size_t words = 0;
            const BatchListsLayout l = batch_lists_layout(cls, total, nseg, words);
            size_t in_list[BATCH_LIST_LONG + 1] = {};
            for (size_t n : len)
                if (n >= cls.shortest) in_list[topk_batch_class(n, kb)]++;
            size_t at = 0;
            for (int c = 0; c <= BATCH_LIST_LONG; c++)
            {
                if (in_list[c] > l.capacity[c] || l.start[c] != at) violations++;
                at += l.capacity[c];
            }
            if (at != words || l.capacity[BATCH_LIST_CHUNKS] != 0) violations++;
        }
    printf("%llu\n", violations);
    return violations ? 1 : 0;
}
"""


def make_cases(limits_by_width):
    """[(dtype, largest, kind, n, k, width, code)]: the wave class at both widths, the workgroup classes and the long one at 11 bits."""
    rng = np.random.default_rng(23)
    cases = []
    for dtype in ("uint32", "float32", "int64", "float64"):
        kb = np.dtype(dtype).itemsize
        limits = limits_by_width[kb]
        lengths = {1, 2, 63, 64, 65}
        for limit in limits:
            lengths |= {limit - 1, limit, limit + 1}
        for n in sorted(lengths):
            widths = (8, 11) if n <= limits[0] + 1 else (11,)
            kinds = ("random", "equal", "three") if n > limits[1] + 1 else ("random", "equal", "three", "low_digit", "top_digit")
            for kind in kinds:
                for largest in (False, True):
                    keys = make_keys(kind, dtype, n, rng)
                    code = key_code(keys, largest)
                    if kind == "three" and n > 4:  # a real all-ones code among the words: it sorts in front of the pads
                        code = code.copy()
                        code[rng.integers(0, n)] = np.iinfo(code.dtype).max
                    ks = sorted({1, 2, n // 2, n - 1, n, n + 3} - {0})
                    if n > limits[1] + 1:
                        ks = [ks[0], n // 2, n + 3]
                    for k in ks:
                        for width in widths:
                            cases.append((dtype, largest, kind, n, k, width, code))
    # ties cut at the threshold: more words equal to the threshold than are taken
    for n, k in ((300, 100), (513, 257), (5000, 64)):
        code = np.full(n, 0x50000000, dtype=np.uint32)
        code[rng.choice(n, k // 3, replace=False)] = rng.integers(0, 1000, k // 3)
        for width in (8, 11):
            cases.append(("uint32", False, "ties", n, k, width, code))
    return cases


@pytest.fixture(scope="module")
def setup(tmp_path_factory, built):
    tmp = tmp_path_factory.mktemp("top_k_batch_plan")
    src = tmp / "top_k_batch_plan.cpp"
    src.write_text(PROGRAM)
    cases = make_cases({4: built.plan_top_k_batch(1, 1, 1, "uint32")["limits"], 8: built.plan_top_k_batch(1, 1, 1, "uint64")["limits"]})
    infile = tmp / "cases.bin"
    with open(infile, "wb") as f:
        f.write(np.array([len(cases)], dtype=np.uint32).tobytes())
        for dtype, _, _, n, k, width, code in cases:
            f.write(np.array([code.dtype.itemsize, n, k, width], dtype=np.uint32).tobytes())
            f.write(code.tobytes())
    return tmp, src, cases, infile


def build_and_run(tmp, src, name, flags, args):
    exe = tmp / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    return subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def results(setup):
    tmp, src, cases, infile = setup
    outfile = tmp / "plain.out"
    p = build_and_run(tmp, src, "top_k_batch_plan", [], [str(infile), str(outfile)])
    raw = open(outfile, "rb").read()
    pos, out = 0, []

    def take(dtype, n):
        nonlocal pos
        v = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += v.nbytes
        return v

    for case in cases:
        threshold = int(take(np.uint64, 1)[0])
        less, need, bucket = (int(x) for x in take(np.uint32, 3))
        out.append({"threshold": threshold, "less": less, "need": need, "bucket": bucket, "index": take(np.uint32, case[4]),
                    "sorted_index": take(np.uint32, case[4])})
    violations = int(take(np.uint64, 1)[0])
    assert pos == len(raw)
    return out, violations, p.returncode


def test_the_invariants_hold_after_every_round_at_both_widths(results):
    _, violations, returncode = results
    assert violations == 0 and returncode == 0


def test_every_class_selects_the_head_of_numpys_stable_argsort(setup, results):
    _, _, cases, _ = setup
    out, _, _ = results
    assert len(cases) >= 1000 and {c[5] for c in cases} == {8, 11}
    for (dtype, largest, kind, n, k, width, code), r in zip(cases, out):
        case = (dtype, largest, kind, n, k, width)
        ks = min(k, n)
        head = np.argsort(code, kind="stable")[:ks]
        assert (r["index"][:ks] == np.sort(head)).all(), case
        assert (r["index"][ks:] == np.arange(ks, k)).all(), case  # the pads
        assert (r["sorted_index"][:ks] == head).all(), case  # the stable sort of the row: best first, pads behind
        assert r["threshold"] == int(code[head[-1]]), case
        assert r["less"] == int((code < code[head[-1]]).sum()) and r["less"] + r["need"] == ks, case
        assert r["bucket"] == int((code == code[head[-1]]).sum()) and 1 <= r["need"] <= r["bucket"], case


def test_the_sanitized_stand_alone_program_runs_clean(setup):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly."""
    tmp, src, _, infile = setup
    p = build_and_run(tmp, src, "top_k_batch_plan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
                      [str(infile), str(tmp / "san.out")])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


def test_the_lists_of_the_top_k_classes_never_overflow(setup):
    tmp = setup[0]
    src = tmp / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    p = build_and_run(tmp, src, "layout", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], [])
    assert p.returncode == 0 and p.stdout.strip() == "0", (p.stdout, p.stderr[-2000:])


# ------------------------------------------------------------------------------------------------------------------ glu_top_k_plan_batch


@pytest.mark.parametrize("dtype", ("uint32", "int64"))
def test_class_boundaries_are_monotone_and_the_loop_starts_at_loop_min(built, dtype):
    G = built
    base = G.plan_top_k_batch(1, 1, 1, dtype)
    limits = base["limits"]
    assert limits == sorted(set(limits)) and base["wave_digit_bits"] in (8, 11) and base["cand_room"] > 0
    assert G.plan_top_k_batch(1, 1, 1, "uint64")["limits"][1:] == [n // 2 for n in G.plan_top_k_batch(1, 1, 1, "uint32")["limits"][1:]]
    assert base["loop_min"] > limits[3]  # the default (provisional) lies in the long class
    order = {G.TopKBatch_Wave: 0, G.TopKBatch_Block: 1, G.TopKBatch_Long: 2, G.TopKBatch_Loop: 3}
    seen, previous = set(), (0, 0)
    counts = sorted({1, 2} | {n + d for n in limits for d in (-1, 0, 1)} | {base["loop_min"] - 1, base["loop_min"], 4 * limits[3]})
    for count in counts:
        p = G.plan_top_k_batch(count, 5, 1, dtype)
        assert (order[p["path"]], p["tile"] or 1 << 31) >= previous, count
        previous = (order[p["path"]], p["tile"] or 1 << 31)
        assert (p["path"] == G.TopKBatch_Loop) == (count >= base["loop_min"]), count
        if p["path"] in (G.TopKBatch_Wave, G.TopKBatch_Block):
            assert p["tile"] == min(n for n in limits if count <= n) and p["kernels"] == 1 + 2
        seen.add(p["path"])
    assert seen == set(order)
    for loop_min in (1, 100, limits[3] + 1):
        for count in (loop_min - 1, loop_min, loop_min + 1):
            if count:
                p = G.plan_top_k_batch(count, 3, 1, dtype, loop_min=loop_min)
                assert (p["path"] == G.TopKBatch_Loop) == (count >= loop_min) and p["loop_min"] == loop_min
                if p["path"] == G.TopKBatch_Loop:
                    for sorted_, arrays in ((True, True), (False, True), (False, False)):
                        assert G.plan_top_k_batch(count, 3, 1, dtype, sorted=sorted_, with_arrays=arrays, loop_min=loop_min)["kernels"] == \
                            3 * G.plan_top_k(count, 1, dtype, sorted=sorted_, with_arrays=arrays)["kernels"]


def test_kernel_counts_and_nothing_to_do(built):
    G = built
    for kwargs in (dict(count=100, num_segments=0, k=3), dict(count=100, num_segments=4, k=0), dict(count=0, num_segments=4, k=0),
                   dict(count=0, num_segments=4, k=3, offsets_form=True), dict(count=100, num_segments=0, k=3, offsets_form=True)):
        p = G.plan_top_k_batch(**kwargs)
        assert p["path"] == G.TopKBatch_None and p["kernels"] == 0 and p["scratch_bytes"] == 0, kwargs
    limits = G.plan_top_k_batch(1, 1, 1)["limits"]
    # device offsets: the binning kernel and one kernel per list that can hold a segment of `total` keys
    for total, lists in ((1, 1), (limits[0], 1), (limits[0] + 1, 2), (limits[2] + 1, 4), (limits[3] + 1, 5), (1 << 20, 5)):
        p = G.plan_top_k_batch(total, 9, 4, offsets_form=True, sorted=False)
        assert p["path"] == G.TopKBatch_Binned and p["kernels"] == 1 + lists, (total, p)
        assert G.plan_top_k_batch(total, 9, 4, offsets_form=True, sorted=True)["kernels"] == 1 + lists + 2
        assert G.plan_top_k_batch(total, 9, 4, offsets_form=True, sorted=True, with_arrays=False)["kernels"] == 1 + lists
    # the rows of pairs of the sorted stage
    assert G.plan_top_k_batch(1000, 7, 10, "uint64")["scratch_bytes"] == 7 * 10 * 12
    assert G.plan_top_k_batch(1000, 7, 10, "uint64", sorted=False)["scratch_bytes"] == 0


def test_refusals_name_the_argument(built):
    G = built
    for words, kwargs in ((["k must not exceed count"], dict(count=10, num_segments=2, k=11)),
                          (["num_segments", "2^24"], dict(count=10, num_segments=(1 << 24) + 1, k=1)),
                          (["2^32"], dict(count=1 << 16, num_segments=1 << 16, k=1)),
                          (["2^32"], dict(count=1 << 32, num_segments=5, k=1, offsets_form=True)),
                          (["num_segments * k"], dict(count=1 << 20, num_segments=1 << 20, k=1 << 12, offsets_form=True)),
                          (["loop_min"], dict(count=10, num_segments=2, k=1, loop_min=1 << 32))):
        with pytest.raises(G.GluError) as e:
            G.plan_top_k_batch(**kwargs)
        assert all(w in str(e.value) for w in words), (words, str(e.value))
    with pytest.raises(KeyError):
        G.plan_top_k_batch(10, 2, 1, "float16")
