"""CPU test of the arithmetic of histogram (csrc/histogram_bins.hpp): the three rules that give a sample its bin, and the plan.  The
header is plain C++: a host program with its own main reads cases, folds lo, hi and bins as glu_histogram.hip does, and writes the
bin of every sample; numpy restates each rule and every comparison is ==.
  even integers  (x.astype(int64) - lo) // W, at x = lo + k*W - 1, lo + k*W, lo + k*W + 1: where a reciprocal would be one off
  even floats    minimum(((x.astype(float64) - lo) * scale).astype(int64), bins - 1), NaN dropped
  edges          searchsorted(edges, x, side="right") - 1, NaN dropped
The same program, built with the address and undefined-behaviour sanitizers, runs the same cases as a stand-alone executable.  No
device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
NO_BIN = 0xFFFFFFFF
EVEN_INT, EVEN_FLOAT, EDGES, PLAN = 0, 1, 2, 3
TYPES = ["uint32", "int32", "float32", "uint64", "int64", "float64"]  # (glu_key_type)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "histogram_bins.hpp"
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

template<typename T>
static void even_int(uint32_t n, uint32_t bins)
{
    const std::vector<int64_t> bounds = get<int64_t>(2);
    const std::vector<T> x = get<T>(n);
    HistEvenInt r = {};
    const bool ok = hist_make_even_int(bounds[0], bounds[1], bins, &r);
    put(std::vector<uint32_t>{ok ? 1u : 0u});
    std::vector<uint32_t> bin(n, kHistNoBin);
    if (ok)
        for (uint32_t i = 0; i < n; i++)
        {
            bin[i] = hist_even_int_bin(r, x[i]);
            if (bin[i] != kHistNoBin && bin[i] >= bins) violations++;
        }
    put(bin);
}

template<typename T>
static void even_float(uint32_t n, uint32_t bins)
{
    const std::vector<T> bounds = get<T>(2);
    const std::vector<T> x = get<T>(n);
    HistEvenFloat r = {};
    const bool ok = hist_make_even_float((double) bounds[0], (double) bounds[1], bins, &r);
    put(std::vector<uint32_t>{ok ? 1u : 0u});
    std::vector<uint32_t> bin(n, kHistNoBin);
    if (ok)
        for (uint32_t i = 0; i < n; i++)
        {
            bin[i] = hist_even_float_bin(r, x[i]);
            if (bin[i] != kHistNoBin && bin[i] >= bins) violations++;
        }
    put(bin);
}

// (the edges of a case may be unsorted or hold NaNs: every probe is counted against the table's length)
template<typename T>
static void edges(uint32_t n, uint32_t bins)
{
    const std::vector<T> e = get<T>((size_t) bins + 1);
    const std::vector<T> x = get<T>(n);
    const uint32_t n_edges = bins + 1, steps = hist_steps(n_edges);
    std::vector<uint32_t> bin(n);
    for (uint32_t i = 0; i < n; i++)
    {
        bin[i] = hist_edges_bin(x[i], n_edges, steps, [&](uint32_t at) {
            if (at >= e.size())
            {
                violations++;
                return (T) 0;
            }
            return e[at];
        });
        if (bin[i] != kHistNoBin && bin[i] >= bins) violations++;
    }
    put(std::vector<uint32_t>{1u});
    put(bin);
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
        const std::vector<uint32_t> h = get<uint32_t>(4); // rule, key type, samples, bins
        const uint32_t rule = h[0], type = h[1], n = h[2], bins = h[3];
        if (rule == 0)
            type == 0 ? even_int<uint32_t>(n, bins) : even_int<int32_t>(n, bins);
        else if (rule == 1)
            type == 2 ? even_float<float>(n, bins) : even_float<double>(n, bins);
        else if (rule == 2)
            switch (type)
            {
            case 0: edges<uint32_t>(n, bins); break;
            case 1: edges<int32_t>(n, bins); break;
            case 2: edges<float>(n, bins); break;
            case 3: edges<uint64_t>(n, bins); break;
            case 4: edges<int64_t>(n, bins); break;
            default: edges<double>(n, bins); break;
            }
        else
        {
            // the plan: n = count's low word, then its high word, key bytes, mode, accumulate
            const std::vector<uint32_t> more = get<uint32_t>(4);
            const uint64_t count = (uint64_t) n | ((uint64_t) more[0] << 32);
            const HistPlan p = hist_plan(count, bins, more[1], (int) more[2], more[3] != 0);
            put(std::vector<uint64_t>{p.path, p.threads, p.tile, p.tiles, p.groups, p.kernels, (uint64_t) p.scratch_bytes});
        }
    }
    put(std::vector<uint64_t>{violations});
    fclose(in);
    fclose(out);
    return violations ? 1 : 0;
}
"""


def around_multiples(lo, w, bins, dtype, rng):
    """x = lo + k*W - 1, lo + k*W, lo + k*W + 1 for k = 0, 1, 2, the last ones, bins (= hi) and a spread between, as far as the type holds
    them; and the ends of the type."""
    info = np.iinfo(dtype)
    ks = {0, 1, 2, bins - 2, bins - 1, bins}
    ks.update(int(k) for k in rng.integers(0, bins + 1, 400))
    ks.update(range(0, min(bins, 300) + 1))
    xs = [info.min, info.min + 1, info.max - 1, info.max]
    for k in ks:
        if k < 0:
            continue
        for d in (-1, 0, 1):
            x = lo + k * w + d
            if info.min <= x <= info.max:
                xs.append(x)
    return np.array(xs, dtype=np.int64).astype(dtype)


def make_cases():
    """[(rule, key_type, bins, bounds or edges, samples)]"""
    rng = np.random.default_rng(15)
    cases = []
    # even bins over integers: the four widths of the issue, on both types where the type holds the range
    for dtype, lo, w, bins in ((np.uint32, 0, 1, 1000), (np.int32, -500, 1, 1000), (np.uint32, 7, 3, 4097), (np.int32, -6000, 3, 4097),
                               (np.int32, -2 ** 31, 65537, 65535), (np.uint32, 0, 65537, 65535), (np.uint32, 0, 1431655765, 3),
                               (np.int32, -2 ** 31, 1431655765, 3), (np.uint32, 0, 1, 2 ** 24), (np.uint32, 0, 255, 2 ** 24),
                               (np.uint32, 1, 2 ** 32 - 2, 1), (np.int32, -2 ** 31, 2 ** 32 - 1, 1), (np.uint32, 5, 641, 6700417 // 641)):
        hi = lo + w * bins
        x = np.concatenate([around_multiples(lo, w, bins, dtype, rng),
                            rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max, 2000, dtype=np.int64, endpoint=True).astype(dtype)])
        cases.append((EVEN_INT, np.dtype(dtype).name, bins, (lo, hi), x))
    # ... and the widths that are refused: not whole, below one, hi <= lo
    for lo, hi, bins in ((0, 10, 3), (0, 5, 10), (10, 10, 1), (10, 3, 1), (0, 2 ** 32 - 1, 2)):
        cases.append((EVEN_INT, "uint32", bins, (lo, hi), np.arange(4, dtype=np.uint32)))
    # even bins over floats
    specials32 = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, -np.nan, np.nextafter(np.float32(1), np.float32(-np.inf)), 1.0,
                           np.nextafter(np.float32(0), np.float32(-1)), np.finfo(np.float32).tiny, 0.5], dtype=np.float32)
    for dtype in (np.float32, np.float64):
        specials = specials32.astype(dtype)
        specials[6] = np.nextafter(dtype(1), dtype(-np.inf))
        specials[8] = np.nextafter(dtype(0), dtype(-1))
        for bins in (49, 2 ** 24, 1, 8192):
            lo, hi = dtype(0), dtype(1)
            scale = bins / (float(hi) - float(lo))
            k = rng.integers(0, bins + 1, 3000)
            at_edges = (k / scale).astype(dtype)  # (samples at and beside where a bin ends in the sample's type)
            x = np.concatenate([specials, at_edges, np.nextafter(at_edges, dtype(-np.inf)), np.nextafter(at_edges, dtype(np.inf)),
                                rng.random(3000).astype(dtype), (rng.random(500) * 3 - 1).astype(dtype)])
            cases.append((EVEN_FLOAT, np.dtype(dtype).name, bins, (lo, hi), x))
        lo, hi = dtype(-3.25), dtype(1e6 + 0.5)
        x = np.concatenate([specials, (rng.random(4000) * 1.2e6 - 1e5).astype(dtype), np.array([lo, hi, np.nextafter(hi, dtype(-np.inf))], dtype=dtype)])
        cases.append((EVEN_FLOAT, np.dtype(dtype).name, 1000003, (lo, hi), x))
        big = np.finfo(dtype).max
        for lo, hi in ((dtype(0), dtype(np.inf)), (dtype(np.nan), dtype(1)), (dtype(1), dtype(1)), (dtype(2), dtype(1)), (-big, big)):
            if dtype == np.float32 and lo == -big:
                continue  # (the range of float32 is finite in double)
            cases.append((EVEN_FLOAT, np.dtype(dtype).name, 10, (lo, hi), np.zeros(4, dtype=dtype)))
    # edges: duplicates, one bin, 8192 bins, every type
    for name in TYPES:
        dtype = np.dtype(name).type
        is_float = name.startswith("float")
        for bins in (1, 2, 7, 100, 8191, 8192):
            if is_float:
                e = np.sort((rng.random(bins + 1) * 200 - 100).astype(dtype))
                if bins >= 7:
                    e[2] = -0.0
                    e[3] = 0.0
                    e = np.sort(e)
            elif name.endswith("64"):
                e = np.sort(rng.integers(0 if name[0] == "u" else -2 ** 62, 2 ** 62, bins + 1).astype(dtype))
            else:
                info = np.iinfo(dtype)
                e = np.sort(rng.integers(info.min // 2, info.max // 2, bins + 1).astype(dtype))
            if bins >= 7:
                e[bins // 2:bins // 2 + 3] = e[bins // 2]  # (repeated edges: empty bins)
                e[:2] = e[0]
                e[-2:] = e[-1]
            pick = e[rng.integers(0, bins + 1, 2000)]
            if is_float:
                x = np.concatenate([pick, np.nextafter(pick, dtype(-np.inf)), np.nextafter(pick, dtype(np.inf)),
                                    (rng.random(2000) * 240 - 120).astype(dtype),
                                    np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=dtype)])
            else:
                info = np.iinfo(dtype)
                wide = pick.astype(object)
                x = np.concatenate([pick, np.array([max(v - 1, info.min) for v in wide], dtype=dtype),
                                    np.array([min(v + 1, info.max) for v in wide], dtype=dtype),
                                    np.array([info.min, info.max, 0], dtype=dtype)])
            cases.append((EDGES, name, bins, e, x))
    # edges that break the contract: only the promise that nothing leaves the table (the program counts every probe)
    bad = rng.permutation(8193).astype(np.float32)
    bad[::7] = np.nan
    cases.append((EDGES, "float32", 8192, bad, rng.permutation(9000).astype(np.float32)))
    cases.append((EDGES, "uint64", 100, rng.permutation(101).astype(np.uint64), rng.permutation(300).astype(np.uint64)))
    return cases


PLAN_CASES = [(count, bins, key_bytes, mode, acc)
              for count in (0, 1, 4095, 4096, 4097, 2048 * 1024 + 1, 8192 * 512 + 1, 2 ** 28, 2 ** 32 - 1)
              for bins in (1, 8192, 8193, 2 ** 24)
              for key_bytes in (4, 8)
              for mode in (0, 1)
              for acc in (0, 1)
              if not (mode == 1 and bins > 8192)]


def restated_plan(count, bins, key_bytes, mode, acc):
    """The header's rule, with the kernels under accumulate."""
    threads = 256 if mode == 0 else 512 if key_bytes == 4 else 1024
    groups_max = 1024 if mode == 0 else 512 if key_bytes == 4 else 256
    tile = threads * 4 * (16 // key_bytes)
    tiles = -(-count // tile)
    groups = min(tiles, groups_max)
    if bins <= 8192:
        kernels = (1 if count else 0) + (1 if count or not acc else 0)
        return [0, threads, tile, tiles, groups, kernels, groups * bins * 4]
    return [1, threads, tile, tiles, groups, (0 if acc else 1) + (1 if count else 0), 0]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("histogram_bins")
    src = tmp / "histogram_bins.cpp"
    src.write_text(PROGRAM)
    cases = make_cases()
    infile = tmp / "cases.bin"
    with open(infile, "wb") as f:
        f.write(np.array([len(cases) + len(PLAN_CASES)], dtype=np.uint32).tobytes())
        for rule, name, bins, bounds, x in cases:
            f.write(np.array([rule, TYPES.index(name), x.size, bins], dtype=np.uint32).tobytes())
            if rule == EVEN_INT:
                f.write(np.array(bounds, dtype=np.int64).tobytes())
            elif rule == EVEN_FLOAT:
                f.write(np.array(bounds, dtype=x.dtype).tobytes())
            else:
                assert bounds.dtype == x.dtype and bounds.size == bins + 1
                f.write(bounds.tobytes())
            f.write(x.tobytes())
        for count, bins, key_bytes, mode, acc in PLAN_CASES:
            f.write(np.array([PLAN, 0, count & 0xFFFFFFFF, bins, count >> 32, key_bytes, mode, acc], dtype=np.uint32).tobytes())
    return tmp, src, cases, infile


def build_and_run(tmp, src, infile, name, flags):
    exe, outfile = tmp / name, tmp / (name + ".out")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    p = subprocess.run([str(exe), str(infile), str(outfile)], capture_output=True, text=True, timeout=600)
    return p, outfile


@pytest.fixture(scope="module")
def results(setup):
    """[(accepted, bins of the samples)] per case, the plans, and the program's count of probes and bins outside their tables."""
    tmp, src, cases, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "histogram_bins", [])
    raw = open(outfile, "rb").read()
    pos, out = 0, []

    def take(dtype, n):
        nonlocal pos
        v = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += v.nbytes
        return v

    for _, _, _, _, x in cases:
        accepted = int(take(np.uint32, 1)[0])
        out.append((accepted, take(np.uint32, x.size)))
    plans = [take(np.uint64, 7).tolist() for _ in PLAN_CASES]
    violations = int(take(np.uint64, 1)[0])
    assert pos == len(raw)
    return out, plans, violations, p.returncode


def want_even_int(x, lo, hi, bins):
    w = (hi - lo) // bins
    wide = x.astype(np.int64)
    q = (wide - lo) // w
    return np.where((wide >= lo) & (wide < hi), q, NO_BIN).astype(np.uint32)


def want_even_float(x, lo, hi, bins):
    d = x.astype(np.float64)
    lo, hi = np.float64(lo), np.float64(hi)
    scale = np.float64(bins) / (hi - lo)
    inside = (d >= lo) & (d < hi)  # (a NaN fails both)
    b = np.minimum(((np.where(inside, d, lo) - lo) * scale).astype(np.int64), bins - 1)
    return np.where(inside, b, NO_BIN).astype(np.uint32)


def want_edges(x, e):
    bins = e.size - 1
    keep = ~np.isnan(x) if x.dtype.kind == "f" else np.ones(x.size, dtype=bool)
    b = np.full(x.size, -1, dtype=np.int64)
    b[keep] = np.searchsorted(e, x[keep], side="right") - 1
    return np.where((b >= 0) & (b < bins), b, NO_BIN).astype(np.uint32)


def test_no_probe_and_no_bin_leaves_its_table(results):
    _, _, violations, returncode = results
    assert violations == 0 and returncode == 0


def test_integer_even_bins_are_the_exact_quotient_beside_every_multiple_of_the_width(setup, results):
    _, _, cases, _ = setup
    out, _, _, _ = results
    widths = set()
    for (rule, name, bins, bounds, x), (accepted, got) in zip(cases, out):
        if rule != EVEN_INT:
            continue
        lo, hi = bounds
        valid = hi > lo and (hi - lo) % bins == 0
        assert accepted == (1 if valid else 0), (name, lo, hi, bins)
        if not valid:
            continue
        widths.add((hi - lo) // bins)
        want = want_even_int(x, lo, hi, bins)
        assert (got == want).all(), (name, lo, hi, bins, x[got != want][:5], got[got != want][:5], want[got != want][:5])
        assert (want != NO_BIN).sum() > 100 or bins < 4
    assert {1, 3, 65537, 1431655765} <= widths


def test_float_even_bins_are_one_subtraction_and_one_multiplication_in_double(setup, results):
    _, _, cases, _ = setup
    out, _, _, _ = results
    seen = set()
    for (rule, name, bins, bounds, x), (accepted, got) in zip(cases, out):
        if rule != EVEN_FLOAT:
            continue
        lo, hi = float(bounds[0]), float(bounds[1])
        valid = bool(np.isfinite(lo) and np.isfinite(hi) and lo < hi and np.isfinite(hi - lo))
        assert accepted == (1 if valid else 0), (name, lo, hi, bins)
        if not valid:
            continue
        seen.add((name, bins))
        want = want_even_float(x, bounds[0], bounds[1], bins)
        assert (got == want).all(), (name, lo, hi, bins, x[got != want][:5], got[got != want][:5], want[got != want][:5])
        if (lo, hi) == (0.0, 1.0):
            # nextafter(hi, -inf) is the last bin's; hi is nobody's; both zeros are bin 0; infinities and NaNs are dropped
            assert got[6] == bins - 1 and got[7] == NO_BIN and got[0] == 0 and got[1] == 0
            assert (got[2:6] == NO_BIN).all() and got[8] == NO_BIN
    assert {("float32", 49), ("float32", 2 ** 24), ("float64", 49), ("float64", 2 ** 24)} <= seen


def test_edges_are_numpys_right_sided_searchsorted_minus_one(setup, results):
    _, _, cases, _ = setup
    out, _, _, _ = results
    seen = set()
    for (rule, name, bins, e, x), (_, got) in zip(cases, out):
        if rule != EDGES:
            continue
        if e.dtype.kind == "f" and np.isnan(e).any() or (np.diff(e.astype(np.float64)) < 0).any():
            assert ((got == NO_BIN) | (got < bins)).all()  # (unspecified counts, nothing outside)
            continue
        seen.add((name, bins))
        want = want_edges(x, e)
        assert (got == want).all(), (name, bins, x[got != want][:5], got[got != want][:5], want[got != want][:5])
        assert not np.isin(got, np.flatnonzero(e[:-1] == e[1:])).any()  # (a repeated edge: an empty bin)
    assert {(t, b) for t in TYPES for b in (1, 8192)} <= seen


def test_the_plan_is_the_restated_rule_with_and_without_accumulate(results):
    _, plans, _, _ = results
    for case, got in zip(PLAN_CASES, plans):
        assert got == restated_plan(*case), case


def test_the_sanitized_stand_alone_program_runs_clean(setup):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly."""
    tmp, src, _, infile = setup
    p, _ = build_and_run(tmp, src, infile, "histogram_bins_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
