"""CPU test of the arithmetic of the batched merge (csrc/merge_batch_path.hpp over csrc/merge_path.hpp): the two sides of a call and
their clamps, the segment of a diagonal, the boundary of a tile, the tile's ranges and its path, the segment of a staged element and
the composite (segment, key).  The headers are plain C++: a host program walks whole calls through their functions alone, boundary by
boundary, tile by tile and thread by thread as merge_batch_kernels.hpp does (its staging buffers stand in for LDS), and reports every
boundary, range, path, output offset, merged key and source, how often each output was written and whether any index left its array
(offset words included).  Well-formed calls are held against numpy's stable lexsort on (side, enc(key), segment); malformed offsets
and shuffled keys only against the promises of the contract: no index outside an array, no output written twice, every out_offsets
entry at most a_total + b_total.  The same program, built with the address and undefined-behaviour sanitizers, runs the same cases
as a stand-alone executable.  No device needed."""
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
#include "merge_batch_path.hpp"
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

// h: key bytes, num_segments (>= 1), a_total, b_total, equal partitions?, a_len, b_len
template<typename K>
static void one_case(const std::vector<uint32_t>& h)
{
    constexpr uint32_t ITEMS = merge_items(sizeof(K), true), TILE = merge_tile(sizeof(K), true);
    typedef MergeBatchComposite<K> Composite;
    const uint32_t S = h[1], a_total = h[2], b_total = h[3], a_len = h[5], b_len = h[6];
    const bool equal = h[4] != 0;
    const std::vector<uint32_t> a_offsets = get<uint32_t>(equal ? 0 : S + 1), b_offsets = get<uint32_t>(equal ? 0 : S + 1);
    const std::vector<K> ak = get<K>(a_total), bk = get<K>(b_total);
    const auto off_a = [&](uint32_t s) {
        if (s > S) violations++;
        return equal ? s * a_len : at(a_offsets, s);
    };
    const auto off_b = [&](uint32_t s) {
        if (s > S) violations++;
        return equal ? s * b_len : at(b_offsets, s);
    };
    const uint32_t room = a_total + b_total, tiles = (room + TILE - 1) / TILE;
    const uint32_t seg_steps = merge_steps(S - 1), split_steps = merge_steps(a_total < b_total ? a_total : b_total);
    const MergeBatchSide a = merge_batch_side(off_a, S, a_total), b = merge_batch_side(off_b, S, b_total);
    const uint32_t total = a.len + b.len;
    if (a.len > a_total || b.len > b_total) violations++;

    // the partition kernel: out_offsets, then the boundaries
    std::vector<uint32_t> out_offsets(S + 1), bounds(2 * ((size_t) tiles + 1));
    for (uint32_t g = 0; g <= S; g++) out_offsets[g] = merge_batch_rel(off_a(g), a) + merge_batch_rel(off_b(g), b);
    for (uint32_t g = 0; g <= tiles; g++)
    {
        const uint64_t d64 = (uint64_t) g * TILE;
        const uint32_t d = d64 < total ? (uint32_t) d64 : total;
        const MergeBatchBoundary bd = merge_batch_boundary(
            d, S, a, b, seg_steps, split_steps, off_a, off_b, [&](uint32_t i, bool any) { return any ? at(ak, i) : (K) 0; },
            [&](uint32_t j, bool any) { return any ? at(bk, j) : (K) 0; });
        if (bd.seg >= S) violations++;
        bounds[2 * g] = bd.split, bounds[2 * g + 1] = bd.seg;
    }

    // the tile kernel
    std::vector<uint32_t> ranges(4 * (size_t) tiles), path(tiles, 0), from(room, 0), written(room, 0);
    std::vector<K> merged(room, (K) 0);
    for (uint32_t t = 0; t < tiles; t++)
    {
        const uint32_t d0 = t * TILE;
        if (d0 >= total) continue;
        const uint32_t count = total - d0 < TILE ? total - d0 : TILE;
        const MergeBatchBoundary bd0 = {bounds[2 * t], bounds[2 * t + 1]}, bd1 = {bounds[2 * t + 2], bounds[2 * t + 3]};
        const MergeBatchTile tile = merge_batch_tile(bd0, bd1, d0, d0 + count, S, [&](uint32_t s) {
            return merge_batch_rel(off_a(s + 1u), a) + merge_batch_rel(off_b(s + 1u), b);
        });
        const MergeRanges r = tile.r;
        ranges[4 * t] = r.a0, ranges[4 * t + 1] = r.a1, ranges[4 * t + 2] = r.b0, ranges[4 * t + 3] = r.b1;
        path[t] = tile.one ? 1u : 2u;
        if (r.a0 > r.a1 || r.a1 > a.len || r.b0 > r.b1 || r.b1 > b.len || (r.a1 - r.a0) + (r.b1 - r.b0) != count || tile.seg0 + tile.span >= S)
        {
            violations++;
            continue;
        }
        const uint32_t ta = r.a1 - r.a0, tb = r.b1 - r.b0, elem_steps = merge_steps(tile.span);
        std::vector<K> lk(count);
        std::vector<uint32_t> lseg(count, 0);
        for (uint32_t x = 0; x < count; x++)
        {
            const bool from_a = x < ta;
            const uint32_t rel = from_a ? r.a0 + x : r.b0 + (x - ta);
            lk[x] = from_a ? at(ak, (uint64_t) a.begin + rel) : at(bk, (uint64_t) b.begin + rel);
            if (!tile.one)
                lseg[x] = from_a ? merge_batch_element_segment(rel, tile.seg0, tile.span, elem_steps, [&](uint32_t s) { return merge_batch_rel(off_a(s), a); })
                                 : merge_batch_element_segment(rel, tile.seg0, tile.span, elem_steps, [&](uint32_t s) { return merge_batch_rel(off_b(s), b); });
            if (lseg[x] > tile.span) violations++;
        }
        const uint32_t tile_steps = merge_steps(ta < tb ? ta : tb);
        for (uint32_t tid = 0; tid < kMergeThreads; tid++)
        {
            const uint32_t diag = merge_thread_diag(tid, ITEMS, count);
            const uint32_t todo = count - diag < ITEMS ? count - diag : ITEMS;
            const auto emit = [&](uint32_t s, uint32_t x, K key, bool live) {
                if (!live) return;
                const uint64_t o = (uint64_t) d0 + diag + s;
                if (o >= room || x >= count)
                {
                    violations++;
                    return;
                }
                merged[o] = key;
                from[o] = x < ta ? a.begin + r.a0 + x : a_total + b.begin + r.b0 + (x - ta); // as an element of A || B
                written[o]++;
            };
            if (tile.one)
            {
                const uint32_t i0 = merge_diag_split(
                    diag, ta, tb, tile_steps, [&](uint32_t i, bool any) { return any ? at(lk, i) : (K) 0; },
                    [&](uint32_t j, bool any) { return any ? at(lk, (uint64_t) ta + j) : (K) 0; });
                if (i0 > ta || diag - i0 > tb)
                {
                    violations++;
                    continue;
                }
                merge_serial<ITEMS, K>(i0, diag - i0, ta, tb, todo, [&](uint32_t x, bool any) { return any ? at(lk, x) : (K) 0; }, emit);
            }
            else
            {
                typedef typename Composite::type C;
                const auto both = [&](uint64_t x) { return Composite::make(at(lseg, x), at(lk, x)); };
                const uint32_t i0 = merge_diag_split(
                    diag, ta, tb, tile_steps, [&](uint32_t i, bool any) { return any ? both(i) : (C) 0; },
                    [&](uint32_t j, bool any) { return any ? both((uint64_t) ta + j) : (C) 0; });
                if (i0 > ta || diag - i0 > tb)
                {
                    violations++;
                    continue;
                }
                merge_serial<ITEMS, C>(
                    i0, diag - i0, ta, tb, todo, [&](uint32_t x, bool any) { return any ? both(x) : (C) 0; },
                    [&](uint32_t s, uint32_t x, C key, bool live) { emit(s, x, Composite::key(key), live); });
            }
        }
    }
    put(std::vector<uint32_t>{tiles, a.begin, a.len, b.begin, b.len});
    put(bounds);
    put(ranges);
    put(path);
    put(out_offsets);
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
        const std::vector<uint32_t> h = get<uint32_t>(7);
        if (h[0] == 8)
            one_case<uint64_t>(h);
        else
            one_case<uint32_t>(h);
    }
    put(std::vector<uint64_t>{violations});
    fclose(in);
    fclose(out);
    return violations ? 1 : 0;
}
"""


def tile(key_bytes):
    return THREADS * ITEMS[key_bytes]


class Case:
    """One call.  kind: "good" (held against the model), "bad" (held to the promises alone).  offsets None: equal partitions."""

    def __init__(self, name, kind, a, b, a_off=None, b_off=None, a_len=0, b_len=0, segments=None):
        self.name, self.kind, self.a, self.b = name, kind, a, b
        self.key_bytes = a.dtype.itemsize
        self.equal = a_off is None
        self.S = segments if self.equal else len(a_off) - 1
        self.a_len, self.b_len = a_len, b_len
        if self.equal:
            assert a.size == self.S * a_len and b.size == self.S * b_len
            a_off, b_off = np.arange(self.S + 1) * a_len, np.arange(self.S + 1) * b_len
        self.a_off, self.b_off = np.asarray(a_off, dtype=np.uint32), np.asarray(b_off, dtype=np.uint32)

    def write(self, f):
        f.write(np.array([self.key_bytes, self.S, self.a.size, self.b.size, int(self.equal), self.a_len, self.b_len], dtype=np.uint32).tobytes())
        if not self.equal:
            f.write(self.a_off.tobytes())
            f.write(self.b_off.tobytes())
        f.write(self.a.tobytes())
        f.write(self.b.tobytes())

    def model(self):
        """(keys, sources as indices into A || B, out_offsets) by numpy's stable lexsort on (side, key, segment)."""
        ao, bo = self.a_off.astype(np.int64), self.b_off.astype(np.int64)
        ia, ib = np.arange(ao[0], ao[-1]), np.arange(bo[0], bo[-1])
        seg = np.concatenate([np.searchsorted(ao, ia, "right") - 1, np.searchsorted(bo, ib, "right") - 1])
        keys = np.concatenate([self.a[ao[0]:ao[-1]], self.b[bo[0]:bo[-1]]])
        side = np.concatenate([np.zeros(ia.size, dtype=np.int64), np.ones(ib.size, dtype=np.int64)])
        src = np.concatenate([ia, ib + self.a.size])
        order = np.lexsort((side, keys, seg))
        return keys[order], src[order], (ao - ao[0]) + (bo - bo[0])


def ragged(rng, u, lens_a, lens_b, descending=False, spread=1 << 20, front=(0, 0), slack=(0, 0)):
    """Sorted runs of the given lengths per segment; descending: the keys of later segments are smaller than those of earlier ones."""
    S = len(lens_a)

    def side(lens, first, extra):
        off = np.concatenate([[0], np.cumsum(lens)]) + first
        keys = rng.integers(0, spread, int(off[-1]) + extra).astype(u)
        for s in range(S):
            run = np.sort(rng.integers(0, spread, int(lens[s])).astype(u))
            if descending:
                run = run + u((S - s) * spread)
            keys[off[s]:off[s + 1]] = run
        return keys, off

    a, ao = side(lens_a, front[0], slack[0])
    b, bo = side(lens_b, front[1], slack[1])
    return a, b, ao, bo


def make_cases():
    rng = np.random.default_rng(25)
    cases = []
    for kb in (4, 8):
        u = np.uint32 if kb == 4 else np.uint64
        T = tile(kb)
        # one segment: the single merge's arrays
        for na, nb in ((0, 0), (1, 0), (5, 5), (T - 1, 1), (T, T), (3 * T + 17, T - 1)):
            a, b, ao, bo = ragged(rng, u, [na], [nb], spread=3 if na == T else 1 << 30)
            cases.append(Case("one segment", "good", a, b, ao, bo))
        # a segment boundary exactly on a tile boundary, one before, one behind
        for first in (T - 1, T, T + 1):
            la = first // 3
            a, b, ao, bo = ragged(rng, u, [la, T // 4], [first - la, T // 4], descending=True)
            cases.append(Case("boundary %d" % (first - T), "good", a, b, ao, bo))
        # hundreds of segments of 0 to 8 in one tile, later segments holding SMALLER keys; offsets not from 0, totals with slack
        S = 700
        a, b, ao, bo = ragged(rng, u, rng.integers(0, 9, S), rng.integers(0, 9, S), descending=True, front=(3, 7), slack=(5, 2))
        cases.append(Case("many a tile", "good", a, b, ao, bo))
        # 2^16 segments, five of them non-empty
        S = 1 << 16
        la, lb = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
        for s, (x, y) in zip((0, 77, 30000, 30001, S - 1), ((T + 5, 3), (0, 2 * T), (700, 900), (T, T), (17, 0))):
            la[s], lb[s] = x, y
        a, b, ao, bo = ragged(rng, u, la, lb, descending=True, spread=1 << 14)
        cases.append(Case("mostly empty", "good", a, b, ao, bo))
        # all keys equal
        lens = rng.integers(0, 2 * T // 3, 9)
        a, b, ao, bo = ragged(rng, u, lens, lens[::-1], spread=1)
        cases.append(Case("all equal", "good", a, b, ao, bo))
        # one side empty in every segment
        lens = rng.integers(0, 900, 12)
        a, b, ao, bo = ragged(rng, u, lens, np.where(np.arange(12) % 2 == 0, 0, 1) * 0, descending=True)
        cases.append(Case("b empty", "good", a, b, ao, bo))
        alt = np.arange(12) % 2
        a, b, ao, bo = ragged(rng, u, lens * alt, lens * (1 - alt), descending=True)
        cases.append(Case("one side empty per segment", "good", a, b, ao, bo))
        # both totals 0
        cases.append(Case("nothing", "good", np.zeros(0, dtype=u), np.zeros(0, dtype=u), np.zeros(6), np.zeros(6)))
        # equal partitions
        for a_len, b_len, S in ((3, 0, 50), (0, 5, 50), (7, 9, 400), (T, T - 1, 3), (0, 0, 4)):
            a, b, _, _ = ragged(rng, u, [a_len] * S, [b_len] * S, descending=True)
            cases.append(Case("equal %d %d" % (a_len, b_len), "good", a, b, a_len=a_len, b_len=b_len, segments=S))
        # malformed offsets over good keys, and shuffled keys over good offsets
        S = 40
        a, b, ao, bo = ragged(rng, u, rng.integers(0, 400, S), rng.integers(0, 400, S), descending=True)
        cases.append(Case("decreasing", "bad", a, b, ao[::-1].copy(), bo))
        cases.append(Case("decreasing both", "bad", a, b, ao[::-1].copy(), bo[::-1].copy()))
        cases.append(Case("beyond", "bad", a, b, ao * 2 + 5, bo + b.size))
        cases.append(Case("beyond from the middle", "bad", a, b, np.where(np.arange(S + 1) > 20, ao + a.size, ao), bo))
        cases.append(Case("all ones", "bad", a, b, np.full(S + 1, 0xFFFFFFFF), np.full(S + 1, 0xFFFFFFFF)))
        cases.append(Case("ones and good", "bad", a, b, np.full(S + 1, 0xFFFFFFFF), bo))
        cases.append(Case("random words", "bad", a, b, rng.integers(0, 1 << 32, S + 1), rng.integers(0, 1 << 32, S + 1)))
        cases.append(Case("random small", "bad", a, b, rng.integers(0, a.size + 9, S + 1), rng.integers(0, b.size + 9, S + 1)))
        cases.append(Case("zigzag", "bad", a, b, np.where(np.arange(S + 1) % 2, a.size, 0), np.sort(rng.integers(0, b.size, S + 1))))
        cases.append(Case("first beyond", "bad", a, b, np.concatenate([[a.size + 3], ao[1:]]), bo))
        cases.append(Case("shuffled", "bad", rng.permutation(a), rng.permutation(b), ao, bo))
        cases.append(Case("shuffled and random", "bad", rng.permutation(a), b[::-1].copy(), rng.integers(0, a.size + 9, S + 1), bo))
    return cases


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("merge_batch_path")
    src = tmp / "merge_batch_path.cpp"
    src.write_text(PROGRAM)
    cases = make_cases()
    infile = tmp / "cases.bin"
    with open(infile, "wb") as f:
        f.write(np.array([len(cases)], dtype=np.uint32).tobytes())
        for c in cases:
            c.write(f)
    return tmp, src, cases, infile


def build_and_run(tmp, src, infile, name, flags):
    exe, outfile = tmp / name, tmp / (name + ".out")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", str(exe), str(src)])
    p = subprocess.run([str(exe), str(infile), str(outfile)], capture_output=True, text=True, timeout=600)
    return p, outfile


@pytest.fixture(scope="module")
def results(setup):
    tmp, src, cases, infile = setup
    p, outfile = build_and_run(tmp, src, infile, "merge_batch_path", [])
    raw = open(outfile, "rb").read()
    pos, out = 0, []

    def take(dtype, n):
        nonlocal pos
        v = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += v.nbytes
        return v

    for c in cases:
        room = c.a.size + c.b.size
        tiles, a_begin, a_len, b_begin, b_len = (int(x) for x in take(np.uint32, 5))
        out.append({"tiles": tiles, "sides": (a_begin, a_len, b_begin, b_len), "bounds": take(np.uint32, 2 * (tiles + 1)).reshape(tiles + 1, 2),
                    "ranges": take(np.uint32, 4 * tiles).reshape(tiles, 4), "path": take(np.uint32, tiles),
                    "out_offsets": take(np.uint32, c.S + 1), "merged": take(c.a.dtype, room), "from": take(np.uint32, room),
                    "written": take(np.uint32, room)})
    violations = int(take(np.uint64, 1)[0])
    assert pos == len(raw)
    return out, violations, p.returncode


def test_no_index_leaves_its_array_whatever_offsets_and_keys_hold(results):
    _, violations, returncode = results
    assert violations == 0 and returncode == 0


def test_well_formed_calls_are_the_stable_sort_by_segment_key_and_side(setup, results):
    """Keys and sources are numpy's lexsort on (side, enc(key), segment); every output in front of the device total is written once
    and none behind it; out_offsets are oa + ob; every stored split is the number of A's elements in front of its diagonal and every
    stored segment the last one that begins at or in front of it."""
    _, _, cases, _ = setup
    out, _, _ = results
    seen = 0
    for c, r in zip(cases, out):
        if c.kind != "good":
            continue
        seen += 1
        what = (c.name, c.key_bytes)
        T, room = tile(c.key_bytes), c.a.size + c.b.size
        keys, src, offs = c.model()
        total = keys.size
        assert r["tiles"] == -(-room // T), what
        assert r["sides"] == (int(c.a_off[0]), int(c.a_off[-1] - c.a_off[0]), int(c.b_off[0]), int(c.b_off[-1] - c.b_off[0])), what
        assert (r["out_offsets"] == offs).all(), what
        assert (r["merged"][:total] == keys).all(), what
        assert (r["from"][:total] == src).all(), what
        assert (r["written"][:total] == 1).all() and (r["written"][total:] == 0).all(), what
        a_in_front = np.concatenate([[0], np.cumsum(src < c.a.size)])
        for t in range(r["tiles"] + 1):
            d = min(t * T, total)
            assert r["bounds"][t][0] == a_in_front[d], (what, t)
            assert r["bounds"][t][1] == min(np.searchsorted(offs, d, "right") - 1, c.S - 1), (what, t)
    assert seen >= 2 * 20


def test_one_segment_is_the_single_merge(setup, results):
    """One segment: every tile takes the single merge's path, and splits, keys and sources are what tests/test_merge_path.py holds the
    single merge to on the same arrays (numpy's stable argsort of the concatenation)."""
    _, _, cases, _ = setup
    out, _, _ = results
    seen = 0
    for c, r in zip(cases, out):
        if c.name != "one segment":
            continue
        seen += 1
        T, total = tile(c.key_bytes), c.a.size + c.b.size
        both = np.concatenate([c.a, c.b])
        order = np.argsort(both, kind="stable")
        a_in_front = np.concatenate([[0], np.cumsum(order < c.a.size)])
        assert r["bounds"][:, 0].tolist() == [int(a_in_front[min(t * T, total)]) for t in range(r["tiles"] + 1)]
        assert (r["merged"] == both[order]).all() and (r["from"] == order).all() and (r["written"] == 1).all()
        assert (r["path"] == 1).all()
    assert seen == 12


def test_both_tile_paths_are_walked_and_the_boundary_cases_take_the_right_one(setup, results):
    """A tile that ends exactly where its segment ends lies inside one segment (path 1); one element more and it spans two (path 2)."""
    _, _, cases, _ = setup
    out, _, _ = results
    by_name = {(c.name, c.key_bytes): r for c, r in zip(cases, out)}
    for kb in (4, 8):
        assert by_name[("boundary 0", kb)]["path"].tolist() == [1, 1]
        assert by_name[("boundary -1", kb)]["path"].tolist() == [2, 1]
        assert by_name[("boundary 1", kb)]["path"].tolist() == [1, 2]
        assert (by_name[("many a tile", kb)]["path"] == 2).all()
        paths = by_name[("mostly empty", kb)]["path"]
        assert (paths == 1).any() and (paths == 2).any()


def test_malformed_calls_keep_the_promises(setup, results):
    """Whatever the offsets and the keys hold: the splits lie in their ranges, a tile's ranges lie inside the sides and hold exactly
    its outputs, every output in front of the device total is written exactly once and none behind it, every output comes from inside
    its tile's ranges, and every out_offsets entry is at most a_total + b_total (here: at most the device total)."""
    _, _, cases, _ = setup
    out, _, _ = results
    seen = 0
    for c, r in zip(cases, out):
        seen += c.kind == "bad"
        what = (c.name, c.key_bytes)
        T, room = tile(c.key_bytes), c.a.size + c.b.size
        a_begin, na, b_begin, nb = r["sides"]
        total = na + nb
        assert na <= c.a.size and nb <= c.b.size and (na == 0 or a_begin + na <= c.a.size) and (nb == 0 or b_begin + nb <= c.b.size), what
        assert (r["out_offsets"] <= total).all() and total <= room, what
        for t in range(r["tiles"] + 1):
            d = min(t * T, total)
            assert max(0, d - nb) <= r["bounds"][t][0] <= min(d, na) and r["bounds"][t][1] < c.S, (what, t)
        for t in range(r["tiles"]):
            d0, d1 = t * T, min(t * T + T, total)
            if d0 >= total:
                continue
            a0, a1, b0, b1 = (int(x) for x in r["ranges"][t])
            assert 0 <= a0 <= a1 <= na and 0 <= b0 <= b1 <= nb and (a1 - a0) + (b1 - b0) == d1 - d0, (what, t)
            src = r["from"][d0:d1].astype(np.int64)
            inside = ((src >= a_begin + a0) & (src < a_begin + a1)) | ((src >= c.a.size + b_begin + b0) & (src < c.a.size + b_begin + b1))
            assert inside.all(), (what, t)
        assert (r["written"][:total] == 1).all() and (r["written"][total:] == 0).all(), what
        both = np.concatenate([c.a, c.b])
        assert (r["merged"][:total] == both[r["from"][:total]]).all(), what
    assert seen == 2 * 12


def test_the_sanitized_stand_alone_program_runs_clean(setup):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly."""
    tmp, src, _, infile = setup
    p, _ = build_and_run(tmp, src, infile, "merge_batch_path_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


def test_the_binding_states_the_headers_tile(built):
    for key_type, key_bytes in (("uint32", 4), ("float32", 4), ("uint64", 8), ("int64", 8)):
        for with_vals in (True, False):
            assert built.plan_merge_batch(1, 1, key_type, with_vals)[0] == tile(key_bytes)
