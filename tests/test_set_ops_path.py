"""CPU test of the arithmetic of the set operations (csrc/set_ops_path.hpp on top of csrc/merge_path.hpp): the bounds of a tile
boundary, and which outputs of the merged order a thread keeps for each of the four operations.  The headers are plain C++: a host
program runs whole calls through their functions alone, boundary by boundary, tile by tile and thread by thread as
set_ops_kernels.hpp does (its staging buffer stands in for LDS), and reports the bounds, for every output of the merged order the
side and index it came from and whether each operation keeps it, the tile counts, the length each call would report and a count of
indices that left their array or their staged range.  Sorted inputs are held against the numpy oracle of the rank rule (elements and
order); shuffled inputs only against the promise: no index outside, a tile's kept count at most its outputs, the reported length at
most the operation's bound.  The same program, built with the address and undefined-behaviour sanitizers, runs the same cases as a
stand-alone executable.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
THREADS = 256
ITEMS = {4: 11, 8: 7}  # (merge_path.hpp: merge_items)
OPS = ("union", "intersection", "difference", "symmetric_difference")  # (glu_set_op's order)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "merge_path.hpp"
#include "set_ops_path.hpp"
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
    const std::vector<K> a = get<K>(na), b = get<K>(nb);
    const uint32_t total = na + nb, tiles = (total + TILE - 1) / TILE;
    // the bounds kernel
    std::vector<SetBounds> bounds(tiles + 1);
    std::vector<uint32_t> bounds_words;
    for (uint32_t t = 0; t <= tiles; t++)
    {
        const uint64_t d64 = (uint64_t) t * TILE;
        const uint32_t d = d64 < total ? (uint32_t) d64 : total;
        bounds[t] = set_ops_boundary<K>(
            d, na, nb, merge_steps(na < nb ? na : nb), merge_steps(na), merge_steps(nb),
            [&](uint32_t i, bool any) { return any ? at(a, i) : (K) 0; }, [&](uint32_t j, bool any) { return any ? at(b, j) : (K) 0; });
        if (bounds[t].start_a > na || bounds[t].start_b > nb) violations++;
        bounds_words.insert(bounds_words.end(), {bounds[t].split, bounds[t].start_a, bounds[t].start_b});
    }
    put(std::vector<uint32_t>{tiles});
    put(bounds_words);
    // the count kernel (the write kernel walks the same way), once per operation
    for (uint32_t op = 0; op < kSetOpCount; op++)
    {
        std::vector<uint32_t> from(total, 0xFFFFFFFFu), tile_counts(tiles, 0);
        std::vector<uint8_t> kept(total, 0), written(total, 0);
        uint64_t sum = 0;
        for (uint32_t t = 0; t < tiles; t++)
        {
            const uint32_t d0 = t * TILE, count = total - d0 < TILE ? total - d0 : TILE;
            const MergeRanges r = merge_tile_ranges(bounds[t].split, bounds[t + 1].split, d0, d0 + count);
            if (r.a0 > r.a1 || r.a1 > na || r.b0 > r.b1 || r.b1 > nb || (r.a1 - r.a0) + (r.b1 - r.b0) != count)
            {
                violations++;
                continue;
            }
            SetTile s;
            s.a0 = r.a0, s.na = r.a1 - r.a0, s.b0 = r.b0, s.nb = r.b1 - r.b0, s.nb_all = nb;
            s.start_a = bounds[t].start_a, s.start_b = bounds[t].start_b;
            std::vector<K> lds(count);
            for (uint32_t x = 0; x < count; x++) lds[x] = x < s.na ? at(a, (uint64_t) r.a0 + x) : at(b, (uint64_t) r.b0 + (x - s.na));
            const uint32_t tile_steps = merge_steps(s.na < s.nb ? s.na : s.nb);
            for (uint32_t tid = 0; tid < kMergeThreads; tid++)
            {
                const uint32_t diag = merge_thread_diag(tid, ITEMS, count);
                const uint32_t todo = count - diag < ITEMS ? count - diag : ITEMS;
                const uint32_t i0 = merge_diag_split(
                    diag, s.na, s.nb, tile_steps, [&](uint32_t i, bool any) { return any ? at(lds, i) : (K) 0; },
                    [&](uint32_t j, bool any) { return any ? at(lds, (uint64_t) s.na + j) : (K) 0; });
                if (i0 > s.na || diag - i0 > s.nb)
                {
                    violations++;
                    continue;
                }
                const uint32_t n = set_ops_thread<ITEMS, K>(
                    op, s, diag, i0, todo, merge_steps(s.na), merge_steps(s.nb), [&](uint32_t x, bool any) { return any ? at(lds, x) : (K) 0; },
                    [&](uint32_t j, bool any) {
                        if (!any) return (K) 0;
                        const uint32_t local = j - s.b0;
                        return local < s.nb ? at(lds, (uint64_t) s.na + local) : at(b, j);
                    },
                    [&](uint32_t step, uint32_t x, K, bool keep) {
                        if (step >= todo)
                        {
                            if (keep) violations++;
                            return;
                        }
                        const uint64_t o = (uint64_t) d0 + diag + step;
                        if (o >= total || x >= count)
                        {
                            violations++;
                            return;
                        }
                        from[o] = x < s.na ? r.a0 + x : na + r.b0 + (x - s.na); // as an element of A || B
                        kept[o] = keep ? 1 : 0;
                        written[o]++;
                    });
                if (n > todo) violations++;
                tile_counts[t] += n;
            }
            if (tile_counts[t] > count) violations++;
            sum += tile_counts[t];
        }
        put(from);
        put(kept);
        put(written);
        put(tile_counts);
        put(std::vector<uint32_t>{set_ops_total(sum, set_op_bound(op, na, nb))});
    }
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


def bound(op, na, nb):
    return {"union": na + nb, "symmetric_difference": na + nb, "difference": na, "intersection": min(na, nb)}[op]


def oracle(ea, eb):
    """{op: the kept elements as indices into A || B, in the output's order} by the rank rule on sorted encoded keys."""
    na, nb = ea.size, eb.size
    ra = np.arange(na) - np.searchsorted(ea, ea, "left")
    mb = np.searchsorted(eb, ea, "right") - np.searchsorted(eb, ea, "left")
    rb = np.arange(nb) - np.searchsorted(eb, eb, "left")
    ma = np.searchsorted(ea, eb, "right") - np.searchsorted(ea, eb, "left")
    match_a, match_b = ra < mb, rb < ma
    none_a, none_b = np.zeros(na, bool), np.zeros(nb, bool)
    keep = {"union": (~none_a, ~match_b), "intersection": (match_a, none_b), "difference": (~match_a, none_b),
            "symmetric_difference": (~match_a, ~match_b)}
    order = np.argsort(np.concatenate([ea, eb]), kind="stable")
    return {op: order[np.concatenate(k)[order]] for op, k in keep.items()}


def make_cases():
    """[(kind, key_bytes, A, B)]: every pair of counts; sorted with heavy ties (an alphabet of 3), sorted without ties within a side
    (about a third of the keys shared), all one value, shuffled.  The keys are the encoded ones (unsigned)."""
    rng = np.random.default_rng(20)
    cases = []
    for key_bytes in (4, 8):
        u = np.uint32 if key_bytes == 4 else np.uint64
        for na in counts(key_bytes):
            for nb in counts(key_bytes):
                ties = [np.sort(rng.integers(0, 3, n)).astype(u) * u(0x40000001) for n in (na, nb)]
                pool = max(na, nb) + (na + nb) // 4 + 1
                unique = [np.sort(rng.permutation(pool)[:n]).astype(u) * u(3 if key_bytes == 4 else 3 << 33) for n in (na, nb)]
                one = [np.full(n, 7, dtype=u) for n in (na, nb)]
                shuffled = [rng.integers(0, 1 << 10, n).astype(u) for n in (na, nb)]
                half = [np.sort(shuffled[0]), shuffled[1][::-1].copy()]  # (one side sorted, the other anything)
                rev = [np.sort(shuffled[0]), np.sort(shuffled[1])[::-1].copy()]  # (one side sorted, the other reversed)
                for kind, (a, b) in (("ties", ties), ("unique", unique), ("one", one), ("shuffled", shuffled), ("shuffled", half), ("shuffled", rev)):
                    assert a.size == na and b.size == nb
                    cases.append((kind, key_bytes, a, b))
    return cases


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The program's source, the cases and their file."""
    tmp = tmp_path_factory.mktemp("set_ops_path")
    src = tmp / "set_ops_path.cpp"
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
    """[{tiles, bounds, op: {from, kept, written, tile_counts, num_out}}] per case, and the program's count of indices that left their
    arrays."""
    tmp, src, cases, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "set_ops_path", [])
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
        r = {"tiles": tiles, "bounds": take(np.uint32, 3 * (tiles + 1)).reshape(tiles + 1, 3)}
        for op in OPS:
            r[op] = {"from": take(np.uint32, total), "kept": take(np.uint8, total), "written": take(np.uint8, total),
                     "tile_counts": take(np.uint32, tiles), "num_out": int(take(np.uint32, 1)[0])}
        out.append(r)
    violations = int(take(np.uint64, 1)[0])
    assert pos == len(raw)
    return out, violations, p.returncode


def test_no_index_leaves_its_array_sorted_or_not(results):
    _, violations, returncode = results
    assert violations == 0 and returncode == 0


def test_sorted_inputs_keep_what_the_rank_rule_keeps_in_merge_order(setup, results):
    """The bounds are merge's split and numpy's lower bounds of the first key behind every boundary; every operation keeps exactly
    the oracle's elements, in its order, and the tile counts are the kept elements of each tile."""
    _, _, cases, _ = setup
    out, _, _ = results
    seen = {"ties": 0, "unique": 0, "one": 0}
    for (kind, key_bytes, a, b), r in zip(cases, out):
        if kind == "shuffled":
            continue
        seen[kind] += 1
        T, total, na, nb = tile(key_bytes), a.size + b.size, a.size, b.size
        case = (kind, key_bytes, na, nb)
        both = np.concatenate([a, b])
        order = np.argsort(both, kind="stable")
        a_in_front = np.concatenate([[0], np.cumsum(order < na)])
        assert r["tiles"] == -(-total // T), case
        for t in range(r["tiles"] + 1):
            d = min(t * T, total)
            want = [int(a_in_front[d])] + ([int(np.searchsorted(a, both[order[d]], "left")), int(np.searchsorted(b, both[order[d]], "left"))]
                                           if d < total else [na, nb])
            assert r["bounds"][t].tolist() == want, (case, t)
        want_kept = oracle(a, b)
        for op in OPS:
            o = r[op]
            assert (o["written"] == 1).all() and (o["from"] == order).all(), (case, op)
            got = o["from"][o["kept"] == 1]
            assert got.size == want_kept[op].size and (got == want_kept[op]).all(), (case, op)
            assert o["num_out"] == got.size <= bound(op, na, nb), (case, op)
            assert o["tile_counts"].tolist() == [int(o["kept"][t * T:t * T + T].sum()) for t in range(r["tiles"])], (case, op)
    assert min(seen.values()) >= 2 * 36


def test_the_oracle_is_the_two_pointer_set_algorithm():
    """The rank rule of the oracle against the textbook two-pointer std::set_* on small multisets."""
    rng = np.random.default_rng(5)
    for _ in range(300):
        a, b = (np.sort(rng.integers(0, 6, rng.integers(0, 12))).astype(np.uint32) for _ in range(2))
        want = {op: [] for op in OPS}
        i = j = 0
        while i < a.size or j < b.size:
            if j == b.size or (i < a.size and a[i] < b[j]):
                for op in ("union", "difference", "symmetric_difference"):
                    want[op].append(i)
                i += 1
            elif i == a.size or b[j] < a[i]:
                for op in ("union", "symmetric_difference"):
                    want[op].append(a.size + j)
                j += 1
            else:
                for op in ("union", "intersection"):
                    want[op].append(i)
                i, j = i + 1, j + 1
        got = oracle(a, b)
        for op in OPS:
            # (the two-pointer walk emits a matched pair at A's place: the same elements; the order is compared by keys)
            both = np.concatenate([a, b])
            assert sorted(got[op].tolist()) == sorted(want[op]), (a, b, op)
            assert both[got[op]].tolist() == both[np.array(want[op], dtype=np.int64)].tolist(), (a, b, op)


def test_shuffled_inputs_keep_the_promise(setup, results):
    """Whatever the keys hold: every output of the merged order is visited once and comes from inside its tile's ranges, a tile keeps
    at most its outputs, and the reported length is at most the operation's bound."""
    _, _, cases, _ = setup
    out, _, _ = results
    seen = 0
    for (kind, key_bytes, a, b), r in zip(cases, out):
        T, total, na, nb = tile(key_bytes), a.size + b.size, a.size, b.size
        case = (kind, key_bytes, na, nb)
        seen += kind == "shuffled"
        for t in range(r["tiles"] + 1):
            d = min(t * T, total)
            split, start_a, start_b = (int(x) for x in r["bounds"][t])
            assert max(0, d - nb) <= split <= min(d, na) and 0 <= start_a <= na and 0 <= start_b <= nb, (case, t)
        for op in OPS:
            o = r[op]
            assert (o["written"] == 1).all() and (o["from"] < total).all(), (case, op)
            for t in range(r["tiles"]):
                assert o["tile_counts"][t] == o["kept"][t * T:t * T + T].sum() <= min(T, total - t * T), (case, op, t)
            assert o["num_out"] == min(int(o["tile_counts"].sum()), bound(op, na, nb)), (case, op)
            if op in ("intersection", "difference"):
                assert (o["from"][o["kept"] == 1] < na).all(), (case, op)  # (never an element of B)
            if op == "union":
                assert o["kept"][o["from"] < na].all(), (case, op)  # (every element of A that the walk meets)
    assert seen >= 2 * 36 * 3


def test_the_sanitized_stand_alone_program_runs_clean(setup):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly."""
    tmp, src, _, infile = setup
    p, _ = build_and_run(tmp, src, infile, "set_ops_path_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


def test_the_binding_states_merges_tile(built):
    for key_type, key_bytes in (("uint32", 4), ("float32", 4), ("uint64", 8), ("int64", 8)):
        for with_arrays in (True, False):
            assert built.plan_set_ops(1, 1, key_type, with_arrays)[0] == tile(key_bytes) == built.plan_merge(1, 1, key_type)[0]
