"""CPU test of the arithmetic of top-k (csrc/topk_pick.hpp): the digit windows per key width, the crossing digit, the update of the
state after a round, the choice between the two paths.  The header is plain C++: a host program runs whole selects through its
functions alone, round after round as topk_kernels.hpp does (vectors stand in for the tables in LDS and for the candidate buffer),
then compacts as the write kernel does, and reports the path, the state and the k indices.  It works on code words, which numpy
makes from the keys of all six types as the sort's key code does (complemented for `largest`), and is held against
numpy.argsort(code, kind="stable")[:k].  After every round it holds 1 <= need <= count[d], at the end less + need == k.  The same
program, built with the address and undefined-behaviour sanitizers, runs the same cases as a stand-alone executable.  No device
needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "topk_pick.hpp"
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

// one round over `words`: the table of the round's digit among the words that match the prefix, the pick, the update
template<typename K>
static void one_round(const std::vector<K>& words, uint32_t round, TopkState& s)
{
    const uint32_t kb = sizeof(K), shift = topk_shift(kb, round), bits = topk_bits(kb, round);
    if (bits == 0 || bits > kTopkDigitBits || shift + bits > 8 * kb) violations++;
    std::vector<uint32_t> table(kTopkBins, 0);
    for (K c : words)
        if (topk_matches(s, c))
        {
            const uint32_t d = topk_digit(c, shift, bits);
            if (d >= (1u << bits)) violations++;
            table[d]++;
        }
    uint32_t before = 0;
    const uint32_t d = topk_find_digit(kTopkBins, s.need, [&](uint32_t i) { return table[i]; }, &before);
    // every digit at once, as the device asks: exactly the one crossing
    uint32_t crossing = 0, run = 0;
    for (uint32_t i = 0; i < kTopkBins; i++)
    {
        if (topk_crosses(run, table[i], s.need))
        {
            crossing++;
            if (i != d || run != before) violations++;
        }
        run += table[i];
    }
    if (crossing != 1) violations++;
    topk_advance(s, kb, round, d, before, table[d]);
    if (s.need < 1 || s.need > s.bucket) violations++; // 1 <= need <= count[d]
}

template<typename K>
static void one_case(uint32_t n, uint32_t k, uint32_t option, uint32_t capacity)
{
    const std::vector<K> code = get<K>(n);
    const uint32_t kb = sizeof(K), rounds = topk_rounds(kb);
    TopkState s = topk_begin(n, k);
    one_round(code, 0, s);
    s.path = topk_choose_path(option, s.bucket, capacity);
    if (s.path == (uint32_t) TOPK_PATH_CANDIDATES)
    {
        std::vector<K> cand;
        for (K c : code)
            if (topk_matches(s, c)) cand.push_back(c);
        s.cand = (uint32_t) cand.size();
        if (cand.size() > capacity || cand.size() != s.bucket) violations++;
        for (uint32_t r = 1; r < rounds; r++) one_round(cand, r, s);
    }
    else
        for (uint32_t r = 1; r < rounds; r++) one_round(code, r, s);
    if (s.less + s.need != k) violations++;
    if (s.mask != (kb == 4 ? 0xFFFFFFFFull : ~0ull)) violations++;
    // the compaction: every word below the threshold and the first `need` equal to it, at less_before + min(ties_before, need)
    std::vector<uint32_t> index(k, 0xA5A5A5A5u), written(k, 0);
    uint32_t less_before = 0, ties_before = 0;
    for (uint32_t i = 0; i < n; i++)
    {
        const bool is_less = code[i] < (K) s.prefix, is_tie = code[i] == (K) s.prefix;
        const uint32_t rank = less_before + (ties_before < s.need ? ties_before : s.need);
        if (is_less || (is_tie && ties_before < s.need))
        {
            if (rank >= k)
                violations++;
            else
            {
                index[rank] = i;
                written[rank]++;
            }
        }
        less_before += is_less;
        ties_before += is_tie;
    }
    for (uint32_t w : written)
        if (w != 1) violations++;
    put(std::vector<uint64_t>{s.prefix});
    put(std::vector<uint32_t>{s.path, s.less, s.need, s.bucket, s.cand});
    put(index);
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
        const std::vector<uint32_t> h = get<uint32_t>(5); // key_bytes, n, k, option, capacity
        if (h[0] == 4) one_case<uint32_t>(h[1], h[2], h[3], h[4]);
        else one_case<uint64_t>(h[1], h[2], h[3], h[4]);
    }
    put(std::vector<uint64_t>{violations});
    fclose(in);
    fclose(out);
    return violations ? 1 : 0;
}
"""

AUTO, CANDIDATES, FULL = 0, 1, 2
DTYPES = ("uint32", "int32", "float32", "uint64", "int64", "float64")


def key_code(keys, largest):
    """The sort's key code (KeyCodec::encode), complemented for `largest`: an unsigned word whose order is the order of the keys."""
    dt = keys.dtype
    u = np.dtype("uint%d" % (8 * dt.itemsize))
    bits = keys.view(u)
    sign = u.type(1) << u.type(8 * dt.itemsize - 1)
    if dt.kind == "u":
        code = bits.copy()
    elif dt.kind == "i":
        code = bits ^ sign
    else:
        code = np.where(bits & sign, ~bits, bits ^ sign)
    return ~code if largest else code


def make_keys(kind, dtype, n, rng):
    dt = np.dtype(dtype)
    u = np.dtype("uint%d" % (8 * dt.itemsize))
    width = 8 * dt.itemsize
    if kind == "random":
        return rng.integers(0, 2**width, n, dtype=u).view(dt)  # (floats: every bit pattern, NaNs of both signs among them)
    if kind == "equal":
        return np.full(n, 0x3F8C0FFE, dtype=u).view(dt)
    if kind == "three":
        return rng.choice(np.array([5, 0x40000000, (1 << (width - 1)) + 77], dtype=u), n).view(dt)
    if kind == "low_digit":  # the keys differ only in the lowest digit (10 bits of a 4-byte key, 9 of an 8-byte one)
        return (u.type(0x12345600 << (width - 32)) ^ rng.integers(0, 2**9, n, dtype=u)).view(dt)
    if kind == "top_digit":  # only in the top digit
        return (u.type(0x000ABCDE) | (rng.integers(0, 2**11, n, dtype=u) << u.type(width - 11))).view(dt)
    if kind == "above_32":
        return (u.type(0x89ABCDEF) | (rng.integers(0, 2**32, n, dtype=u) << u.type(32))).view(dt)
    if kind == "below_32":
        return ((u.type(0x01234567) << u.type(32)) | rng.integers(0, 2**32, n, dtype=u)).view(dt)
    raise ValueError(kind)


def make_cases():
    """[(dtype, largest, kind, n, k, option, capacity, code)]"""
    rng = np.random.default_rng(17)
    cases = []
    for dtype in DTYPES:
        wide = np.dtype(dtype).itemsize == 8
        kinds = ["random", "equal", "three", "low_digit", "top_digit"] + (["above_32", "below_32"] if wide else [])
        for largest in (False, True):
            for n in (1, 63, 64, 65, 4097, 70001):
                for kind in kinds:
                    if n == 70001 and kind not in ("random", "equal", "three"):
                        continue
                    keys = make_keys(kind, dtype, n, rng)
                    code = key_code(keys, largest)
                    for k in sorted({1, 2, n // 2, n - 1, n} & set(range(1, n + 1))):
                        cases.append((dtype, largest, kind, n, k, AUTO, 1 << 16, code))
    # both paths at n = 70001 uniform uint32 keys and k = 1000: the largest top-digit bucket holds about 55 keys
    keys = rng.integers(0, 2**32, 70001, dtype=np.uint32)
    for largest in (False, True):
        code = key_code(keys, largest)
        for option, capacity in ((AUTO, 64), (CANDIDATES, 64), (AUTO, 8), (CANDIDATES, 8), (FULL, 64)):
            cases.append(("uint32", largest, "paths", 70001, 1000, option, capacity, code))
    return cases


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("top_k_pick")
    src = tmp / "top_k_pick.cpp"
    src.write_text(PROGRAM)
    cases = make_cases()
    infile = tmp / "cases.bin"
    with open(infile, "wb") as f:
        f.write(np.array([len(cases)], dtype=np.uint32).tobytes())
        for dtype, _, _, n, k, option, capacity, code in cases:
            f.write(np.array([code.dtype.itemsize, n, k, option, capacity], dtype=np.uint32).tobytes())
            f.write(code.tobytes())
    return tmp, src, cases, infile


def build_and_run(tmp, src, infile, name, flags):
    exe, outfile = tmp / name, tmp / (name + ".out")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    p = subprocess.run([str(exe), str(infile), str(outfile)], capture_output=True, text=True, timeout=600)
    return p, outfile


@pytest.fixture(scope="module")
def results(setup):
    tmp, src, cases, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "top_k_pick", [])
    raw = open(outfile, "rb").read()
    pos, out = 0, []

    def take(dtype, n):
        nonlocal pos
        v = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += v.nbytes
        return v

    for case in cases:
        threshold = int(take(np.uint64, 1)[0])
        path, less, need, bucket, cand = (int(x) for x in take(np.uint32, 5))
        out.append({"threshold": threshold, "path": path, "less": less, "need": need, "bucket": bucket, "cand": cand,
                    "index": take(np.uint32, case[4])})
    violations = int(take(np.uint64, 1)[0])
    assert pos == len(raw)
    return out, violations, p.returncode


def test_the_invariants_hold_after_every_round(results):
    _, violations, returncode = results
    assert violations == 0 and returncode == 0


def test_the_select_is_the_head_of_numpys_stable_argsort(setup, results):
    _, _, cases, _ = setup
    out, _, _ = results
    assert len(cases) >= 700
    for (dtype, largest, kind, n, k, option, capacity, code), r in zip(cases, out):
        case = (dtype, largest, kind, n, k, option, capacity)
        head = np.argsort(code, kind="stable")[:k]
        assert (r["index"] == np.sort(head)).all(), case
        assert r["threshold"] == int(code[head[-1]]), case
        assert r["less"] == int((code < code[head[-1]]).sum()) and r["less"] + r["need"] == k, case
        assert r["bucket"] == int((code == code[head[-1]]).sum()) and 1 <= r["need"] <= r["bucket"], case
        # ordered by (code, index), which is what the stable sort of the pairs in index order gives, they are the head itself
        picked = r["index"].astype(np.int64)
        assert (picked[np.argsort(code[picked], kind="stable")] == head).all(), case


def test_the_capacity_decides_the_path(setup, results):
    _, _, cases, _ = setup
    out, _, _ = results
    seen = set()
    for (dtype, largest, kind, n, k, option, capacity, code), r in zip(cases, out):
        if kind != "paths":
            continue
        top = np.bincount((code >> np.uint32(21)).astype(np.int64), minlength=2048)
        crossing = int(np.searchsorted(np.cumsum(top), k))
        fits = top[crossing] <= capacity
        assert 8 < top[crossing] <= 64, top[crossing]
        want = CANDIDATES if fits and option != FULL else FULL
        assert r["path"] == want, (option, capacity, r["path"])
        assert r["cand"] == (top[crossing] if want == CANDIDATES else 0)
        seen.add((option, capacity, want))
    assert (CANDIDATES, 8, FULL) in seen and (AUTO, 64, CANDIDATES) in seen and (FULL, 64, FULL) in seen


def test_the_sanitized_stand_alone_program_runs_clean(setup):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly."""
    tmp, src, _, infile = setup
    p, _ = build_and_run(tmp, src, infile, "top_k_pick_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


def test_the_binding_states_the_headers_windows(built):
    assert built.plan_top_k(1000, 10, "uint32")["digits"] == [(21, 11), (10, 11), (0, 10)]
    assert built.plan_top_k(1000, 10, "float64")["digits"] == [(53, 11), (42, 11), (31, 11), (20, 11), (9, 11), (0, 9)]
