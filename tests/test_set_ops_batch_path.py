"""CPU test of the arithmetic of the batched set operations (csrc/set_ops_batch_path.hpp over merge_batch_path.hpp and
set_ops_path.hpp).  The headers are plain C++: a host program walks whole calls through their functions alone -- the bounds of every
tile boundary, the count of every tile thread by thread on both tile paths (its staging buffers stand in for LDS), the scan, one
out_offsets entry per segment boundary and the write of every tile from the count's words -- with every access counted against its
array (offset words included).  Well-formed calls are held against a textbook two-pointer multiset operation per segment, written
here; malformed offsets and shuffled keys only against the promises of the contract: no index outside an array, a tile's kept count at
most its outputs, num_out <= bound, every out_offsets entry <= min(bound, max_out), nothing written at or behind min(bound, max_out).
The same program, built with the address and undefined-behaviour sanitizers, runs the same cases as a stand-alone executable started
directly.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-radix-sort_amd", "csrc")
THREADS = 256
ITEMS = {4: 11, 8: 7}  # (merge_path.hpp: merge_items)
OPS = ["union", "intersection", "difference", "symmetric_difference"]
NO_SOURCE = 0xFFFFFFFF

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "set_ops_batch_path.hpp"
using namespace glu_hip;

static unsigned long long violations = 0;
static uint32_t from_memory = 0; // partners read from B's array and not from the staged part, per case
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

// h: key bytes, num_segments (>= 1), a_total, b_total, equal partitions?, a_len, b_len, op, max_out, with arrays?
template<typename K>
static void one_case(const std::vector<uint32_t>& h)
{
    constexpr uint32_t ITEMS = merge_items(sizeof(K), true), TILE = merge_tile(sizeof(K), true);
    typedef MergeBatchComposite<K> Composite;
    typedef typename Composite::type C;
    const uint32_t S = h[1], a_total = h[2], b_total = h[3], a_len = h[5], b_len = h[6], op = h[7], max_out = h[8];
    const bool equal = h[4] != 0, with_arrays = h[9] != 0;
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
    const uint32_t tiles = (a_total + b_total + TILE - 1) / TILE;
    const uint32_t seg_steps = merge_steps(S - 1), split_steps = merge_steps(a_total < b_total ? a_total : b_total);
    const uint32_t bound = set_ops_total(0xFFFFFFFFull, set_op_bound(op, a_total, b_total));
    const uint32_t room = with_arrays ? (bound < max_out ? bound : max_out) : 0u, limit = with_arrays ? room : bound;
    const MergeBatchSide a = merge_batch_side(off_a, S, a_total), b = merge_batch_side(off_b, S, b_total);
    const uint32_t total = a.len + b.len;
    if (a.len > a_total || b.len > b_total) violations++;
    const auto a_key = [&](uint32_t i, bool any) { return any ? at(ak, i) : (K) 0; };
    const auto b_key = [&](uint32_t j, bool any) { return any ? at(bk, j) : (K) 0; };

    // the bounds kernel
    std::vector<SetBatchBounds> bounds((size_t) tiles + 1);
    for (uint32_t g = 0; g <= tiles; g++)
    {
        const uint64_t d64 = (uint64_t) g * TILE;
        const uint32_t d = d64 < total ? (uint32_t) d64 : total;
        bounds[g] = set_ops_batch_boundary<K>(d, S, a, b, seg_steps, split_steps, merge_steps(a_total), merge_steps(b_total), off_a, off_b, a_key, b_key);
        if (bounds[g].seg >= S || bounds[g].start_a > a.len || bounds[g].start_b > b.len) violations++;
    }

    // a tile as both kernels stage it: its keys and (several segments) its segment words
    struct Staged
    {
        SetBatchTile tile;
        uint32_t count;
        std::vector<K> lk;
        std::vector<uint32_t> lseg;
        bool ok;
    };
    const auto stage = [&](uint32_t t) {
        Staged s;
        const uint32_t d0 = t * TILE;
        s.count = total - d0 < TILE ? total - d0 : TILE;
        s.tile = set_ops_batch_tile(
            bounds[t], bounds[t + 1], d0, d0 + s.count, S, [&](uint32_t g) { return merge_batch_rel(off_a(g + 1u), a) + merge_batch_rel(off_b(g + 1u), b); },
            [&](uint32_t g) { return merge_batch_rel(off_b(g + 1u), b); });
        const SetTile& r = s.tile.t;
        s.ok = !((uint64_t) r.a0 + r.na > a.len || (uint64_t) r.b0 + r.nb > b.len || r.na + r.nb != s.count || s.tile.seg0 + s.tile.span >= S || r.nb_all > b.len);
        if (!s.ok)
        {
            violations++;
            return s;
        }
        const uint32_t elem_steps = merge_steps(s.tile.span);
        s.lk.resize(s.count);
        s.lseg.assign(s.count, 0);
        for (uint32_t x = 0; x < s.count; x++)
        {
            const bool from_a = x < r.na;
            const uint32_t rel = from_a ? r.a0 + x : r.b0 + (x - r.na);
            s.lk[x] = from_a ? at(ak, (uint64_t) a.begin + rel) : at(bk, (uint64_t) b.begin + rel);
            if (!s.tile.one)
                s.lseg[x] = from_a ? merge_batch_element_segment(rel, s.tile.seg0, s.tile.span, elem_steps, [&](uint32_t g) { return merge_batch_rel(off_a(g), a); })
                                   : merge_batch_element_segment(rel, s.tile.seg0, s.tile.span, elem_steps, [&](uint32_t g) { return merge_batch_rel(off_b(g), b); });
            if (s.lseg[x] > s.tile.span) violations++;
        }
        return s;
    };

    // the count kernel
    std::vector<uint32_t> tile_counts(tiles, 0), words((size_t) tiles * kMergeThreads, 0), path(tiles, 0);
    for (uint32_t t = 0; t < tiles; t++)
    {
        if (t * TILE >= total) continue; // (its count is 0)
        const Staged st = stage(t);
        if (!st.ok) continue;
        const SetTile& r = st.tile.t;
        path[t] = st.tile.one ? 1u : 2u;
        const uint32_t steps = merge_steps(r.na < r.nb ? r.na : r.nb);
        const auto b_at = [&](uint32_t j, bool any) {
            if (!any) return (K) 0;
            const uint32_t local = j - r.b0;
            if (local >= r.nb) from_memory++;
            return local < r.nb ? at(st.lk, (uint64_t) r.na + local) : at(bk, (uint64_t) b.begin + j);
        };
        uint32_t rank = 0;
        for (uint32_t tid = 0; tid < kMergeThreads; tid++)
        {
            const uint32_t diag = merge_thread_diag(tid, ITEMS, st.count);
            const uint32_t todo = st.count - diag < ITEMS ? st.count - diag : ITEMS;
            uint32_t mask = 0, kept;
            if (st.tile.one)
            {
                const uint32_t i0 = merge_diag_split(
                    diag, r.na, r.nb, steps, [&](uint32_t i, bool any) { return any ? at(st.lk, i) : (K) 0; },
                    [&](uint32_t j, bool any) { return any ? at(st.lk, (uint64_t) r.na + j) : (K) 0; });
                kept = set_ops_thread<ITEMS, K>(
                    op, r, diag, i0, todo, merge_steps(r.na), merge_steps(r.nb), [&](uint32_t x, bool any) { return any ? at(st.lk, x) : (K) 0; }, b_at,
                    [&](uint32_t s, uint32_t x, K, bool keep) {
                        if (x >= st.count) violations++;
                        mask |= keep ? 1u << s : 0u;
                    });
            }
            else
            {
                const auto both = [&](uint32_t x, bool any) { return any ? Composite::make(at(st.lseg, x), at(st.lk, x)) : (C) 0; };
                const uint32_t i0 = merge_diag_split(
                    diag, r.na, r.nb, steps, [&](uint32_t i, bool any) { return both(i, any); },
                    [&](uint32_t j, bool any) { return both(any ? r.na + j : 0u, any); });
                kept = set_ops_batch_thread<ITEMS, K>(
                    op, r, diag, i0, todo, merge_steps(r.na), merge_steps(r.nb), both, b_at,
                    [&](uint32_t seg) {
                        if (seg > st.tile.span) violations++;
                        return merge_batch_rel(off_b(st.tile.seg0 + seg + 1u), b);
                    },
                    [&](uint32_t s, uint32_t x, C, bool keep) {
                        if (x >= st.count) violations++;
                        mask |= keep ? 1u << s : 0u;
                    });
            }
            if (kept > todo || kept != (uint32_t) __builtin_popcount(mask) || (mask >> todo) != 0) violations++;
            words[(size_t) t * kMergeThreads + tid] = set_batch_word(rank, mask);
            rank += kept;
        }
        if (rank > st.count) violations++; // a tile keeps at most its outputs
        tile_counts[t] = rank < st.count ? rank : st.count;
    }

    // the scan
    uint64_t sum = 0;
    std::vector<uint32_t> scanned(tiles, 0);
    for (uint32_t t = 0; t < tiles; t++)
    {
        scanned[t] = (uint32_t) sum;
        sum += tile_counts[t];
    }
    const uint32_t num_out = set_ops_total(sum, bound);

    // the offsets kernel
    std::vector<uint32_t> out_offsets(S + 1);
    for (uint32_t g = 0; g <= S; g++)
    {
        const uint32_t d = merge_batch_rel(off_a(g), a) + merge_batch_rel(off_b(g), b);
        const uint32_t kept = set_ops_batch_kept_before(
            d, total, TILE, ITEMS, num_out, [&](uint32_t t) { return at(scanned, t); }, [&](uint64_t w) { return at(words, w); });
        out_offsets[g] = set_ops_batch_entry(kept, limit);
    }

    // the write kernel: the order from the merge walk, the decisions from the words
    std::vector<K> keys(bound, (K) 0);
    std::vector<uint32_t> from(bound, 0xFFFFFFFFu), written(bound, 0);
    for (uint32_t t = 0; with_arrays && t < tiles; t++)
    {
        const uint32_t first = scanned[t];
        if (first >= room || t * TILE >= total) continue;
        const Staged st = stage(t);
        if (!st.ok) continue;
        const SetTile& r = st.tile.t;
        const uint32_t steps = merge_steps(r.na < r.nb ? r.na : r.nb);
        const uint32_t last = words[(size_t) t * kMergeThreads + kMergeThreads - 1u];
        uint32_t tile_kept = set_batch_word_rank(last) + set_batch_word_kept(last);
        tile_kept = tile_kept < st.count ? tile_kept : st.count;
        const uint32_t n = tile_kept < room - first ? tile_kept : room - first;
        for (uint32_t tid = 0; tid < kMergeThreads; tid++)
        {
            const uint32_t diag = merge_thread_diag(tid, ITEMS, st.count);
            const uint32_t todo = st.count - diag < ITEMS ? st.count - diag : ITEMS;
            const uint32_t word = words[(size_t) t * kMergeThreads + tid], mask = set_batch_word_mask(word) & ((1u << todo) - 1u);
            uint32_t rank = set_batch_word_rank(word);
            const auto emit = [&](uint32_t s, uint32_t x, K key, bool live) {
                if (!live || !(mask >> s & 1u)) return;
                if (x >= st.count)
                {
                    violations++;
                    return;
                }
                if (rank < st.count && rank < n) // (the slot in LDS, then what merge_store_tile stores)
                {
                    const uint64_t o = (uint64_t) first + rank;
                    if (o >= room)
                        violations++;
                    else
                    {
                        keys[o] = key;
                        from[o] = x < r.na ? a.begin + r.a0 + x : a_total + b.begin + r.b0 + (x - r.na); // as an element of A || B
                        written[o]++;
                    }
                }
                rank++;
            };
            if (st.tile.one)
            {
                const uint32_t i0 = merge_diag_split(
                    diag, r.na, r.nb, steps, [&](uint32_t i, bool any) { return any ? at(st.lk, i) : (K) 0; },
                    [&](uint32_t j, bool any) { return any ? at(st.lk, (uint64_t) r.na + j) : (K) 0; });
                merge_serial<ITEMS, K>(i0, diag - i0, r.na, r.nb, todo, [&](uint32_t x, bool any) { return any ? at(st.lk, x) : (K) 0; }, emit);
            }
            else
            {
                const auto both = [&](uint64_t x) { return Composite::make(at(st.lseg, x), at(st.lk, x)); };
                const uint32_t i0 = merge_diag_split(
                    diag, r.na, r.nb, steps, [&](uint32_t i, bool any) { return any ? both(i) : (C) 0; },
                    [&](uint32_t j, bool any) { return any ? both((uint64_t) r.na + j) : (C) 0; });
                merge_serial<ITEMS, C>(
                    i0, diag - i0, r.na, r.nb, todo, [&](uint32_t x, bool any) { return any ? both(x) : (C) 0; },
                    [&](uint32_t s, uint32_t x, C key, bool live) { emit(s, x, Composite::key(key), live); });
            }
        }
    }
    put(std::vector<uint32_t>{tiles, a.len + b.len, bound, room, num_out, from_memory});
    from_memory = 0;
    put(path);
    put(tile_counts);
    put(out_offsets);
    put(keys);
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
        const std::vector<uint32_t> h = get<uint32_t>(10);
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


def bound_of(op, na, nb):
    return na + nb if op in (0, 3) else (na if op == 2 else min(na, nb))


def two_pointer(a, b):
    """The textbook walk of two sorted lists: (side, index, matched) per element in merge's order (A first among equal keys).  A[i]
    and B[j] with equal keys are matched to each other and both cursors move; everything else is unmatched."""
    i = j = 0
    events = []
    na, nb = len(a), len(b)
    while i < na and j < nb:
        if a[i] < b[j]:
            events.append((0, i, False))
            i += 1
        elif b[j] < a[i]:
            events.append((1, j, False))
            j += 1
        else:
            events.append((0, i, True))
            events.append((1, j, True))
            i += 1
            j += 1
    events.extend((0, x, False) for x in range(i, na))
    events.extend((1, x, False) for x in range(j, nb))
    return events


def keeps(op, side, matched):
    if op == 0:
        return side == 0 or not matched
    if op == 1:
        return side == 0 and matched
    if op == 2:
        return side == 0 and not matched
    return not matched


class Case:
    """One call.  kind: "good" (held against the model), "bad" (held to the promises alone).  offsets None: equal partitions."""

    def __init__(self, name, kind, a, b, a_off=None, b_off=None, a_len=0, b_len=0, segments=None, op=0, max_out=None, with_arrays=True):
        self.name, self.kind, self.a, self.b = name, kind, a, b
        self.key_bytes = a.dtype.itemsize
        self.equal = a_off is None
        self.S = segments if self.equal else len(a_off) - 1
        self.a_len, self.b_len = a_len, b_len
        if self.equal:
            assert a.size == self.S * a_len and b.size == self.S * b_len
            a_off, b_off = np.arange(self.S + 1) * a_len, np.arange(self.S + 1) * b_len
        self.a_off, self.b_off = np.asarray(a_off, dtype=np.uint32), np.asarray(b_off, dtype=np.uint32)
        self.op, self.with_arrays = op, with_arrays
        self.bound = bound_of(op, a.size, b.size)
        self.max_out = self.bound + 7 if max_out is None else max_out
        self.room = min(self.bound, self.max_out) if with_arrays else 0
        self._cache = [None]

    def with_op(self, op, **kw):
        c = Case(self.name, self.kind, self.a, self.b, None if self.equal else self.a_off, None if self.equal else self.b_off, self.a_len,
                 self.b_len, self.S, op, **kw)
        c._cache = self._cache
        return c

    def write(self, f):
        f.write(np.array([self.key_bytes, self.S, self.a.size, self.b.size, int(self.equal), self.a_len, self.b_len, self.op, self.max_out,
                          int(self.with_arrays)], dtype=np.uint32).tobytes())
        if not self.equal:
            f.write(self.a_off.tobytes())
            f.write(self.b_off.tobytes())
        f.write(self.a.tobytes())
        f.write(self.b.tobytes())

    def events(self):
        """per segment, the two-pointer walk of its runs with absolute indices (shared by the four operations of one input)"""
        if self._cache[0] is None:
            ao, bo = self.a_off.astype(np.int64), self.b_off.astype(np.int64)
            al, bl = self.a.tolist(), self.b.tolist()
            events = []
            for s in range(self.S):
                ev = two_pointer(al[ao[s]:ao[s + 1]], bl[bo[s]:bo[s + 1]]) if ao[s + 1] + bo[s + 1] > ao[s] + bo[s] else []
                events.append([(side, (ao[s] if side == 0 else bo[s]) + x, m) for side, x, m in ev])
            self._cache[0] = events
        return self._cache[0]

    def model(self):
        """(keys, sources as indices into A || B, cardinalities per segment)"""
        keys, src, card = [], [], []
        for ev in self.events():
            n = 0
            for side, x, matched in ev:
                if keeps(self.op, side, matched):
                    keys.append(self.a[x] if side == 0 else self.b[x])
                    src.append(x if side == 0 else self.a.size + x)
                    n += 1
            card.append(n)
        return np.array(keys, dtype=self.a.dtype), np.array(src, dtype=np.int64), np.array(card, dtype=np.int64)


def ragged(rng, u, lens_a, lens_b, spread=1 << 20, front=(0, 0), slack=(0, 0)):
    """Sorted runs of the given lengths per segment, every segment over the SAME key range: only the offsets keep the segments apart,
    and equal keys meet across every segment boundary."""
    S = len(lens_a)

    def side(lens, first, extra):
        off = np.concatenate([[0], np.cumsum(lens)]) + first
        keys = rng.integers(0, spread, int(off[-1]) + extra).astype(u)
        for s in range(S):
            keys[off[s]:off[s + 1]] = np.sort(rng.integers(0, spread, int(lens[s])).astype(u))
        return keys, off

    a, ao = side(lens_a, front[0], slack[0])
    b, bo = side(lens_b, front[1], slack[1])
    return a, b, ao, bo


def make_cases():
    rng = np.random.default_rng(26)
    inputs = []  # (name, kind, a, b, a_off, b_off, equal)
    for kb in (4, 8):
        u = np.uint32 if kb == 4 else np.uint64
        T = tile(kb)

        def add(name, kind, a, b, ao=None, bo=None, **kw):
            inputs.append(Case(name, kind, a, b, ao, bo, **kw))

        # one segment: the single call's arrays, half of the keys shared
        for na, nb in ((0, 0), (1, 0), (0, 3), (5, 5), (T, T), (2 * T + 17, T - 1)):
            a, b, ao, bo = ragged(rng, u, [na], [nb], spread=3 if na == T else max(4, na))
            add("one segment", "good", a, b, ao, bo)
        # 1. equal keys across a segment boundary, inside a tile and exactly on a tile boundary; both directions
        for first in (T - 1, T, T + 1, T // 2):
            la, q = first // 3, T // 4
            draw = lambda n, lo, hi: np.sort(rng.integers(lo, hi, n)).astype(u)  # noqa: E731
            a = np.concatenate([draw(la - 1, 0, 49), [49], draw(q, 50, 61), [61], draw(q - 1, 62, 80)]).astype(u)  # A_0 ends with 49, A_2 begins with 61
            b = np.concatenate([draw(first - la, 0, 49), [49], draw(q - 2, 50, 61), [61], draw(q, 62, 80)]).astype(u)  # B_1 begins with 49 and ends with 61
            add("boundary %d" % (first - T), "good", a, b, [0, la, la + q, la + 2 * q], [0, first - la, first - la + q, first - la + 2 * q])
        # 2. a run of one key longer than a tile inside a segment, a segment boundary in the tile where it ends: m <, ==, > n
        for m, n in ((T + 100, T + 300), (T + 200, T + 200), (T + 300, T + 100), (2 * T + 50, 3), (3, 2 * T + 50)):
            a = np.concatenate([[1, 2], np.full(m, 7), [9], [7, 7, 8], [7]]).astype(u)
            b = np.concatenate([[2, 3], np.full(n, 7), [9, 9], [7, 8, 8], [7, 7]]).astype(u)
            add("long run", "good", a, b, [0, m + 3, m + 6, m + 7], [0, n + 4, n + 7, n + 9])
        # 3. a partner outside the staged part: B's run much longer than A's, the next segment's B begins with the same key
        for small in (3 * T - 20, 3 * T - 45, 2 * T + 1):
            a = np.concatenate([np.full(40, 5), [6], np.full(30, 5)]).astype(u)
            b = np.concatenate([np.sort(rng.integers(0, 5, small)), np.full(20, 5), np.full(25, 5), [6]]).astype(u)
            add("partner outside", "good", a, b, [0, 41, 71], [0, small + 20, small + 46])
        # 4. segments empty on one side, on both, and 2^16 empty segments at one position between two full ones
        lens = rng.integers(0, 900, 12)
        alt = np.arange(12) % 3
        a, b, ao, bo = ragged(rng, u, lens * (alt != 0), lens[::-1] * (alt != 1), spread=300)
        add("empty sides", "good", a, b, ao, bo)
        S = (1 << 16) + 2
        la, lb = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
        la[0], lb[0], la[-1], lb[-1] = T // 2, T, T + 9, T // 3
        a, b, ao, bo = ragged(rng, u, la, lb, spread=700)
        add("mostly empty", "good", a, b, ao, bo)
        # 5. many segments a tile
        S = 300
        a, b, ao, bo = ragged(rng, u, rng.integers(0, 12, S), rng.integers(0, 12, S), spread=6, front=(3, 7), slack=(5, 2))
        add("many a tile", "good", a, b, ao, bo)
        # all keys equal
        lens = rng.integers(0, 2 * T // 3, 7)
        a, b, ao, bo = ragged(rng, u, lens, lens[::-1], spread=1)
        add("all equal", "good", a, b, ao, bo)
        # both totals 0
        add("nothing", "good", np.zeros(0, dtype=u), np.zeros(0, dtype=u), np.zeros(6), np.zeros(6))
        # 9. equal partitions
        for a_len, b_len, S in ((3, 0, 50), (0, 5, 50), (7, 9, 300), (T, T - 1, 2), (0, 0, 4)):
            a, b, _, _ = ragged(rng, u, [a_len] * S, [b_len] * S, spread=8 if a_len < T else T)
            add("equal %d %d" % (a_len, b_len), "good", a, b, a_len=a_len, b_len=b_len, segments=S)
        # malformed offsets over good keys, and shuffled keys over good offsets
        S = 40
        a, b, ao, bo = ragged(rng, u, rng.integers(0, 300, S), rng.integers(0, 300, S), spread=500)
        add("decreasing", "bad", a, b, ao[::-1].copy(), bo)
        add("decreasing both", "bad", a, b, ao[::-1].copy(), bo[::-1].copy())
        add("beyond", "bad", a, b, ao * 2 + 5, bo + b.size)
        add("beyond from the middle", "bad", a, b, np.where(np.arange(S + 1) > 20, ao + a.size, ao), bo)
        add("all ones", "bad", a, b, np.full(S + 1, 0xFFFFFFFF), np.full(S + 1, 0xFFFFFFFF))
        add("ones and good", "bad", a, b, np.full(S + 1, 0xFFFFFFFF), bo)
        add("random words", "bad", a, b, rng.integers(0, 1 << 32, S + 1), rng.integers(0, 1 << 32, S + 1))
        add("random small", "bad", a, b, rng.integers(0, a.size + 9, S + 1), rng.integers(0, b.size + 9, S + 1))
        add("zigzag", "bad", a, b, np.where(np.arange(S + 1) % 2, a.size, 0), np.sort(rng.integers(0, b.size, S + 1)))
        add("shuffled", "bad", rng.permutation(a), rng.permutation(b), ao, bo)
        add("shuffled and random", "bad", rng.permutation(a), b[::-1].copy(), rng.integers(0, a.size + 9, S + 1), bo)
    cases = []
    for c in inputs:
        for op in range(4):
            cases.append(c.with_op(op))
        if c.name in ("many a tile", "boundary -1", "long run", "decreasing", "shuffled", "random small"):
            # max_out cutting inside a tile, 0 (a call that only counts), and a call that only counts by its NULL array
            cases.append(c.with_op(0, max_out=(c.a.size + c.b.size) // 3))
            cases.append(c.with_op(3, max_out=5))
            cases.append(c.with_op(2, max_out=0, with_arrays=False))
            cases.append(c.with_op(1, with_arrays=False))
    return cases


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("set_ops_batch_path")
    src = tmp / "set_ops_batch_path.cpp"
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
    p, outfile = build_and_run(tmp, src, infile, "set_ops_batch_path", [])
    raw = open(outfile, "rb").read()
    pos, out = 0, []

    def take(dtype, n):
        nonlocal pos
        v = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += v.nbytes
        return v

    for c in cases:
        tiles, total, bound, room, num_out, from_memory = (int(x) for x in take(np.uint32, 6))
        out.append({"from_memory": from_memory, "tiles": tiles, "total": total, "bound": bound, "room": room, "num_out": num_out, "path": take(np.uint32, tiles),
                    "tile_counts": take(np.uint32, tiles), "out_offsets": take(np.uint32, c.S + 1), "keys": take(c.a.dtype, bound),
                    "from": take(np.uint32, bound), "written": take(np.uint32, bound)})
    violations = int(take(np.uint64, 1)[0])
    assert pos == len(raw)
    return out, violations, p.returncode


def test_no_index_leaves_its_array_and_no_tile_keeps_more_than_its_outputs(results):
    _, violations, returncode = results
    assert violations == 0 and returncode == 0


def test_well_formed_calls_are_the_two_pointer_operation_of_every_segment(setup, results):
    """Keys and sources are the per-segment two-pointer walk's, the segments back to back; num_out is the true total also beyond
    max_out; out[0 .. min(S, max_out)) is written once and nothing behind it; out_offsets are the running cardinalities held to max_out,
    and not held to it in a call that only counts."""
    _, _, cases, _ = setup
    out, _, _ = results
    seen = cut = counted = 0
    for c, r in zip(cases, out):
        if c.kind != "good":
            continue
        seen += 1
        what = (c.name, c.key_bytes, OPS[c.op], c.max_out, c.with_arrays)
        keys, src, card = c.model()
        total = keys.size
        assert r["bound"] == c.bound and r["room"] == c.room and r["tiles"] == -(-(c.a.size + c.b.size) // tile(c.key_bytes)), what
        assert r["num_out"] == total, what
        assert int(r["tile_counts"].sum()) == total, what
        running = np.concatenate([[0], np.cumsum(card)])
        assert (r["out_offsets"] == (np.minimum(running, c.max_out) if c.with_arrays else running)).all(), what
        n = min(total, c.room)
        cut += c.with_arrays and n < total
        counted += not c.with_arrays
        assert (r["keys"][:n] == keys[:n]).all(), what
        assert (r["from"][:n] == src[:n]).all(), what
        assert (r["written"][:n] == 1).all() and (r["written"][n:] == 0).all() and (r["from"][n:] == NO_SOURCE).all(), what
    assert seen >= 2 * 4 * 28 and cut >= 6 and counted >= 6


def test_both_tile_paths_are_walked_and_the_boundary_cases_take_the_right_one(setup, results):
    _, _, cases, _ = setup
    out, _, _ = results
    by_name = {(c.name, c.key_bytes): r for c, r in zip(cases, out) if c.op == 0 and c.with_arrays and c.max_out > c.bound}
    for kb in (4, 8):
        assert by_name[("boundary 0", kb)]["path"][:2].tolist() == [1, 2]  # (the second tile holds the boundary of segments 1 and 2)
        assert by_name[("boundary -1", kb)]["path"][0] == 2 and by_name[("boundary 1", kb)]["path"][:2].tolist() == [1, 2]
        assert (by_name[("many a tile", kb)]["path"] == 2).all()
        assert (by_name[("one segment", kb)]["path"] == 1).all()
        paths = by_name[("long run", kb)]["path"]
        assert (paths == 1).any() and paths[-1] == 2
        paths = by_name[("partner outside", kb)]["path"]
        assert (paths[:-1] == 1).all() and paths[-1] == 2
        for op in (1, 2, 3):  # (the union keeps A either way and never looks into B)
            got = [r["from_memory"] for c, r in zip(cases, out) if (c.name, c.key_bytes, c.op) == ("partner outside", kb, op)]
            assert len(got) == 3 and got[0] > 0, (kb, op, got)
    assert any((r["path"] == 1).any() for r in out) and any((r["path"] == 2).any() for r in out)


def test_equal_keys_across_a_segment_boundary_never_match(setup, results):
    """A_s ends with k and B_{s + 1} begins with k (and the reverse): the intersection keeps neither, the difference keeps A's."""
    _, _, cases, _ = setup
    out, _, _ = results
    seen = 0
    for c, r in zip(cases, out):
        if not c.name.startswith("boundary") or c.max_out <= c.bound or not c.with_arrays:
            continue
        ao = c.a_off.astype(np.int64)
        last_of_a0, first_of_a2 = ao[1] - 1, ao[2]
        assert c.a[last_of_a0] == 49 and c.a[first_of_a2] == 61 and (c.b[c.b_off[0]:c.b_off[1]] != 49).all()
        kept = set(r["from"][:r["num_out"]].tolist())
        if c.op == 1:
            assert last_of_a0 not in kept, (c.name, c.key_bytes)
            seen += 1
        if c.op == 2:
            assert last_of_a0 in kept, (c.name, c.key_bytes)
            seen += 1
    assert seen == 2 * 2 * 4


def test_malformed_calls_keep_the_promises(setup, results):
    """Whatever the offsets and the keys hold: num_out <= bound, every out_offsets entry <= min(bound, max_out) (<= bound in a call
    that only counts), every tile's count at most its outputs, nothing written at or behind min(bound, max_out), nothing twice, and every
    written key is the key of the source it names."""
    _, _, cases, _ = setup
    out, _, _ = results
    seen = 0
    for c, r in zip(cases, out):
        seen += c.kind == "bad"
        what = (c.name, c.key_bytes, OPS[c.op], c.max_out, c.with_arrays)
        T = tile(c.key_bytes)
        assert r["num_out"] <= c.bound, what
        assert (r["out_offsets"] <= (c.room if c.with_arrays else c.bound)).all(), what
        for t in range(r["tiles"]):
            assert r["tile_counts"][t] <= max(0, min(T, r["total"] - t * T)), (what, t)
        assert (r["written"] <= 1).all() and (r["written"][c.room:] == 0).all(), what
        w = np.flatnonzero(r["written"])
        both = np.concatenate([c.a, c.b])
        assert (r["keys"][w] == both[r["from"][w]]).all(), what
    assert seen == 2 * 11 * 4 + 2 * 3 * 4


def test_the_sanitized_stand_alone_program_runs_clean(setup):
    """The same program and cases under -fsanitize=address,undefined: a stand-alone executable with its own main, run directly."""
    tmp, src, _, infile = setup
    p, _ = build_and_run(tmp, src, infile, "set_ops_batch_path_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
