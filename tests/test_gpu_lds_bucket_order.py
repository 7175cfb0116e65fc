"""GPU tests of step 3 of the in-LDS pass (radix_lds_bucket.hpp / bucket_order.hpp: every lane walks its buckets of two words or more
through two bit masks) and of the output loop's predicate at the ragged ends of a run.  Every case is built run by run, so that the
words of a run fall into the buckets the case is about, sorted through the C ABI on a fresh RadixSort(options=...), and compared bit
for bit with oracle.stable_sort_pairs (values = iota: stability is checked); every case asserts that the sort ended in LDS in the
tile it means to test.

How a case places words.  Behind the two top-bit passes a run holds the pairs of one value of the top 16 key bits, in input order;
the pair at place i of the run gets slot (begin & 31) + i, and its word is low << SLOT_BITS | slot (low: the 16 low key bits).  The
bucket of a word is its top DIGIT_BITS bits: for both tiles of 4-byte keys used here, bits [SLOT_BITS + 16 - DIGIT_BITS, ...) lie
above the slot, so the bucket is low >> (16 - DIGIT_BITS) -- 16 low values per bucket in the 256 x 18 tile (4096 buckets), 64 in the
256 x 6 tile (1024 buckets) --, and thread t owns the buckets j * THREADS + t, j < BPT.  The constants below restate BucketSmem.

A tile holds 4608 (1536) words and has 4096 (1024) buckets, so not every bucket of a run can hold two words: 'every bucket' below
means every bucket that holds a word -- the rows j < 9 of every thread, or all BPT buckets of as many threads as the tile fills."""
import functools

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

SMALL = dict(GLU_HIP_SORT_PAIR_MIN=1, GLU_HIP_SORT_FINISH_MIN=1)
BUCKET_MAX_LEN = 24  # kBucketMaxLen: a bucket of more words makes its run a crowded one


class Tile:
    """BucketSmem<KeyT, THREADS, KPT> (radix_lds_bucket.hpp), restated."""

    def __init__(self, threads, kpt, low_bits=16):
        self.threads, self.tile = threads, threads * kpt
        self.cap = self.tile + 32
        self.slot_bits = (self.cap - 1).bit_length()
        self.nb = 1 << (self.tile.bit_length() - 1)
        self.digit_bits = (self.nb - 1).bit_length()
        self.bpt = self.nb // threads
        self.low_bits = low_bits
        self.dsh = max(low_bits + self.slot_bits - self.digit_bits, 0)
        assert self.dsh >= self.slot_bits  # (the slot does not reach into the bucket: a bucket is a range of low key bits)
        self.per_bucket = 1 << (self.dsh - self.slot_bits)  # low values per bucket

    def bucket(self, low, slot=0):
        return ((int(low) << self.slot_bits) | slot) >> self.dsh

    def low_of(self, bucket, k=0):
        """the k-th low value that falls into `bucket`"""
        return bucket * self.per_bucket + k


BIG, LITTLE = Tile(256, 18), Tile(256, 6)
assert (BIG.cap, BIG.slot_bits, BIG.nb, BIG.bpt, BIG.per_bucket) == (4640, 13, 4096, 16, 16)
assert (LITTLE.cap, LITTLE.slot_bits, LITTLE.nb, LITTLE.bpt, LITTLE.per_bucket) == (1568, 11, 1024, 4, 64)
assert BIG.bucket(BIG.low_of(4095, 15), 4639) == 4095 and LITTLE.bucket(LITTLE.low_of(17, 63), 1567) == 17


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def _deal(seqs, rng):
    """One sequence of all the elements of `seqs`, dealt at random, every sequence's elements in their order."""
    owner = np.repeat(np.arange(len(seqs)), [len(q) for q in seqs])
    rng.shuffle(owner)
    out = np.empty(owner.size, dtype=seqs[0].dtype)
    out[np.argsort(owner, kind="stable")] = np.concatenate(seqs)
    return out


def _assemble(runs, seed, top_shift=16, dtype=np.uint32):
    """runs: [(top value, low key bits in the order the run's pairs shall have in the input)], tops distinct.  The pairs of all runs are
    dealt over the array at random, every run's in its order."""
    runs = sorted(runs, key=lambda r: r[0])
    assert len({t for t, _ in runs}) == len(runs)
    return _deal([(dtype(t) << dtype(top_shift)) | low.astype(dtype) for t, low in runs], np.random.default_rng(seed))


def _buckets_of(tile, buckets, words, rng):
    """`words` words in each of `buckets`, the buckets dealt into one another (bucket mates are no neighbours in the run).  The low
    values of a bucket are distinct as far as it has room for them, and come with descending values at ascending slots: input order
    is the reverse of sorted order, whatever places the atomics hand out.  (Beyond the room: equal keys, whose values keep input order.)"""
    out = []
    for b in buckets:
        k = np.sort(rng.choice(tile.per_bucket, min(words, tile.per_bucket), replace=False))[::-1]
        k = np.concatenate([k, rng.integers(0, tile.per_bucket, words - k.size)])
        out.append((tile.low_of(int(b)) + k).astype(np.uint32))
    return _deal(out, rng)


N_MIN = (1 << 22) + 1000  # (sorts are planned, and the narrow hand-off taken, from 2^22 pairs)


def _with_fillers(runs, rng, n_min=N_MIN):
    """More runs of 2600 .. 4608 uniformly drawn pairs, at tops not taken (lengths that walk `begin` through every alignment), until the
    input has n_min pairs: more than an eighth of the pairs then lie in runs longer than the 256 x 10 tile holds, and the device
    chooses the 256 x 18 tile.  Tops 0 and 65535 are taken: the runs are the top 16 bits of the whole key."""
    taken = {t for t, _ in runs}
    free = [int(t) for t in rng.permutation(np.arange(1, 65535)) if int(t) not in taken]
    for t in (0, 65535):
        if t not in taken:
            free.insert(0, t)
    total = sum(low.size for _, low in runs)
    runs = list(runs)
    while total < n_min or free[0] in (0, 65535):
        low = rng.integers(0, 65536, int(rng.integers(2600, 4609)), dtype=np.uint32)
        runs.append((free.pop(0), low))
        total += low.size
    return runs


def _big_tile_input(special, seed):
    """`special`: the low-bit arrays of the runs a case is about, at tops drawn over the key range, among filler runs."""
    rng = np.random.default_rng(seed)
    tops = rng.choice(np.arange(1, 65535), len(special), replace=False)
    return _assemble(_with_fillers([(int(t), low) for t, low in zip(tops, special)], rng), seed + 1)


def _little_tile_input(special, seed):
    """Full-range keys in the 256 x 6 tile: `special` at tops 300, 301, ..., every other top a run of about 64 uniformly drawn pairs."""
    rng = np.random.default_rng(seed)
    runs = [(300 + i, low) for i, low in enumerate(special)]
    others = np.setdiff1d(np.arange(65536), np.arange(300, 300 + len(special)))
    lens = rng.poisson((N_MIN - sum(low.size for low in special)) / others.size + 1, others.size)
    lens[[0, -1]] = np.maximum(lens[[0, -1]], 1)  # (tops 0 and 65535 are there)
    runs += [(int(t), rng.integers(0, 65536, int(l), dtype=np.uint32)) for t, l in zip(others, lens) if l]
    return _assemble(runs, seed + 1)


def _rows(tile, rows, threads=None):
    """the buckets j * THREADS + t for j in rows, t in threads (all of them by default)"""
    return [j * tile.threads + t for j in rows for t in (range(tile.threads) if threads is None else threads)]


def _case_every_bucket():
    rng = np.random.default_rng(100)
    T = BIG
    return [
        _buckets_of(T, _rows(T, range(9)), 2, rng),               # two words in 9 buckets of every thread: the whole tile, 4608 words
        _buckets_of(T, _rows(T, range(16), range(144)), 2, rng),  # two words in ALL 16 buckets of 144 threads: the longest worklist
        _buckets_of(T, _rows(T, range(16), range(100, 172)), 4, rng),  # four words in all 16 buckets of 72 threads
        _buckets_of(T, _rows(T, range(16), range(199, 256)), 5, rng),  # five words in all 16 buckets of 57 threads: the second mask full
        _buckets_of(T, _rows(T, range(16), range(30, 66)), 8, rng),
        _buckets_of(T, _rows(T, range(16), range(3, 35)), 9, rng),     # the insertion, 16 times per thread
        _buckets_of(T, _rows(T, range(12), range(60, 76)), BUCKET_MAX_LEN, rng),
    ]


def _case_one_lane():
    rng = np.random.default_rng(101)
    T = BIG
    out = []
    for words in (2, 3, 5):
        for t in (0, 63, 64, 255):
            own = _rows(T, range(16), [t])
            single = rng.choice(np.setdiff1d(np.arange(T.nb), own), 1000, replace=False)  # (one word each: nothing to order there)
            for pick in (own, own[-1:], own[:1]):  # a full worklist beside empty ones; only the thread's last bucket; only its first
                out.append(_deal([_buckets_of(T, pick, words, rng), _buckets_of(T, single, 1, rng)], rng))
    out.append(_buckets_of(T, [T.nb - 1], 2, rng))  # (a run of ONE bucket: the last of the table, its two words the stage's last)
    out.append(_buckets_of(T, rng.choice(T.nb, 3000, replace=False), 1, rng))  # (no bucket of two at all)
    return out


EDGE_LENGTHS = (2, 3, 4, 5, 8, 9, BUCKET_MAX_LEN, BUCKET_MAX_LEN + 1)


def _case_branch_edges():
    """A run per bucket length at every branch edge of the walk, the bucket at a thread's first, a middle and its last place, with
    single words around (dealt among them: a wave whose first words crowd into one bucket would bail out before it counts); and a
    run that holds all of the lengths the walk orders.  25 words in a bucket make the run a crowded one."""
    rng = np.random.default_rng(102)
    T = BIG
    out = []
    for words in EDGE_LENGTHS:
        for b in (0, 5 * T.threads + 77, T.nb - 1):
            single = rng.choice(np.setdiff1d(np.arange(T.nb), [b]), 2000, replace=False)
            out.append(_deal([_buckets_of(T, [b], words, rng), _buckets_of(T, single, 1, rng)], rng))
    picks = rng.choice(T.nb, 7 * 40, replace=False).reshape(7, 40)
    out.append(_deal([_buckets_of(T, picks[i], w, rng) for i, w in enumerate(EDGE_LENGTHS[:7])], rng))
    return out


def _mixed_runs(rng, lengths):
    out = []
    for length in lengths:
        out.append(rng.integers(0, 65536, length, dtype=np.uint32))                                     # uniform low bits
        for bits in (9, 10, 11):                                                                        # two to four words per bucket everywhere
            spread = np.sort(rng.choice(16, bits, replace=False))
            draw = rng.integers(0, 1 << bits, length, dtype=np.uint32)
            out.append(sum(((draw >> np.uint32(i)) & np.uint32(1)) << np.uint32(s) for i, s in enumerate(spread)).astype(np.uint32))
        out.append(rng.integers(0, 4096, length, dtype=np.uint32) * np.uint32(16))                      # multiples of 16
    return out


def _run_end_lengths(tile):
    return (1, 2, 3, 31, 32, 33, tile.tile - 1, tile.tile)


def _check_alignments(runs, lengths):
    """(the input does what it says: runs of every length in `lengths` begin at many alignments of the line and at all of the piece)"""
    runs = sorted(runs, key=lambda r: r[0])
    begins = np.cumsum([0] + [low.size for _, low in runs])[:-1]
    seen = {}
    for (_, low), b in zip(runs, begins):
        seen.setdefault(low.size, set()).add(int(b) & 31)
    for length in lengths:
        assert len(seen[length]) >= 16 and len({b & 3 for b in seen[length]}) == 4, (length, seen[length])


@functools.lru_cache(maxsize=None)
def _input(name):
    """(keys, values, expected keys, expected values, capacity): built and sorted by the oracle once, read-only."""
    if name == "run_ends_big":
        # 40 runs of every length, at neighbouring tops so that short runs follow one another: `begin` walks through the alignments
        rng = np.random.default_rng(104)
        runs = [(1000 + i, rng.integers(0, 65536, length, dtype=np.uint32)) for i, length in enumerate(_run_end_lengths(BIG) * 40)]
        runs = _with_fillers(runs, rng)
        _check_alignments(runs, _run_end_lengths(BIG))
        keys, cap = _assemble(runs, 1041), BIG.tile
    elif name == "run_ends_little":
        rng = np.random.default_rng(105)
        special = [rng.integers(0, 65536, length, dtype=np.uint32) for length in _run_end_lengths(LITTLE) * 40]
        _check_alignments([(300 + i, low) for i, low in enumerate(special)], _run_end_lengths(LITTLE))
        keys, cap = _little_tile_input(special, 1051), LITTLE.tile
    elif name == "little_tile_buckets":
        # the 256 x 6 tile (BPT = 4): runs with two, four, five, nine, 24 and 25 words in every bucket they fill, and mixed ones
        rng = np.random.default_rng(106)
        T = LITTLE
        special = [_buckets_of(T, _rows(T, range(3)), 2, rng), _buckets_of(T, _rows(T, range(4), range(192)), 2, rng),
                   _buckets_of(T, _rows(T, range(4), range(96)), 4, rng), _buckets_of(T, _rows(T, range(4), range(180, 256)), 5, rng),
                   _buckets_of(T, _rows(T, range(4), range(42)), 9, rng), _buckets_of(T, _rows(T, range(4), range(16)), BUCKET_MAX_LEN, rng),
                   _deal([_buckets_of(T, [T.nb - 1], BUCKET_MAX_LEN + 1, rng), _buckets_of(T, range(0, 900), 1, rng)], rng)]
        special += _mixed_runs(rng, (1536, 1535, 700))
        keys, cap = _little_tile_input(special, 1061), LITTLE.tile
    else:
        special = {"every_bucket": _case_every_bucket, "one_lane": _case_one_lane, "branch_edges": _case_branch_edges,
                   "mixed": lambda: _mixed_runs(np.random.default_rng(103), (4608, 4607, 4000, 2561))}[name]()
        assert all(low.size <= BIG.tile for low in special), [low.size for low in special]
        keys, cap = _big_tile_input(special, 200 + len(name)), BIG.tile
    vals = np.arange(keys.size, dtype=np.uint32)
    ek, ev = O.stable_sort_pairs(keys, vals)
    for a in (keys, vals, ek, ev):
        a.setflags(write=False)
    return keys, vals, ek, ev, cap


def _sort_and_check(G, keys, vals, ek, ev, cap, narrow):
    s = G.RadixSort(options=dict(SMALL, GLU_HIP_SORT_NARROW_HANDOFF=narrow))
    kb, vb = G.ShaderStorageBuffer(keys), G.ShaderStorageBuffer(vals)
    s(kb, vb, keys.size)
    G.synchronize()
    gk, gv, fin = kb.get_data(np.uint32), vb.get_data(np.uint32), s.read_finish()
    assert fin["attempted"] == 1 and fin["accepted"] == 1 and fin["capacity"] == cap and fin["top_bit"] == 32, fin
    assert fin["longest_run"] <= cap, fin  # (no run for the segmented passes: the bucket kernel orders every run, or lists it as crowded)
    assert s.read_handoff()["narrow"] == narrow
    assert (gk == ek).all(), "keys differ from the oracle at %s" % np.flatnonzero(gk != ek)[:5]
    assert (gv == ev).all(), "values differ from the oracle at %s" % np.flatnonzero(gv != ev)[:5]


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("name", ["every_bucket", "one_lane", "branch_edges", "mixed", "run_ends_big", "run_ends_little",
                                  "little_tile_buckets"])
def test_buckets_and_run_ends(G, name, narrow):
    """every_bucket: two, four, five, eight, nine and 24 words in every bucket a run fills (full worklists in the first mask, in the
    second, and for the insertion).  one_lane: only the buckets of one thread hold two words or more -- all 16, only its last, only its
    first.  branch_edges: bucket lengths 2, 3, 4, 5, 8, 9, 24 and 25 -- the last one bails out as crowded and is ordered by the ballot
    kernel; the library reports no count of crowded runs, so what shows it is the result (a listed run that no kernel took would come
    out unsorted) -- with descending keys at ascending slots.  mixed: uniform low bits, low bits with 9 .. 11 varying bits, multiples of
    16.  run_ends_*: runs of 1, 2, 3, 31, 32, 33, tile - 1 and tile pairs at every alignment of their first pair.  little_tile_buckets:
    the 256 x 6 tile's four buckets per thread."""
    _sort_and_check(G, *_input(name), narrow)


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("tail", [1, 2, 3])
def test_last_piece_of_the_array(G, narrow, tail):
    """n = 4 k + tail: the array's last run ends in a piece that is loaded and stored element by element; it holds buckets of two to five
    words up to its last word."""
    keys, vals, _, _, cap = _input("mixed")
    n = keys.size - ((keys.size - tail) % 4)
    assert n % 4 == tail
    keys = keys[:n].copy()
    last = keys >= np.uint32(0xFFFF0000)
    rng = np.random.default_rng(tail)
    keys[last] = np.uint32(0xFFFF0000) | (rng.integers(0, 1500, int(last.sum()), dtype=np.uint32) * np.uint32(16) + rng.integers(0, 16, int(last.sum()), dtype=np.uint32))
    vals = vals[:n]
    ek, ev = O.stable_sort_pairs(keys, vals)
    assert int(last.sum()) > 2560
    _sort_and_check(G, keys, vals, ek, ev, cap, narrow)


def test_keys_only(G):
    """Keys only, 256 x 18 tile: no values to gather, no hand-off."""
    keys = _input("mixed")[0]
    s = G.RadixSort(options=dict(SMALL, GLU_HIP_SORT_LARGE_MIN=1, GLU_HIP_SORT_NARROW_HANDOFF=0))
    kb = G.ShaderStorageBuffer(keys)
    s.sort_keys_ptr(kb.device_ptr(), keys.size)
    G.synchronize()
    fin = s.read_finish()
    assert fin["attempted"] == 1 and fin["accepted"] == 1 and fin["capacity"] == BIG.tile and fin["top_bit"] == 32, fin
    assert (kb.get_data(np.uint32) == _input("mixed")[2]).all()


def test_float32_keys_with_values(G):
    """float32 keys: encoded by the first top-bit pass, decoded by the in-LDS pass's output loop (the ragged pieces too)."""
    code = _input("branch_edges")[0]  # the order-preserving code of the floats: what the kernel sees
    top = np.uint32(0x80000000)
    stored = np.where(code & top, code ^ top, ~code)
    # (some patterns are NaNs: the sort orders the code, whatever the pattern means, and so does the comparison below)
    vals = np.arange(code.size, dtype=np.uint32)
    s = G.RadixSort(options=dict(SMALL, GLU_HIP_SORT_NARROW_HANDOFF=0))
    kb, vb = G.ShaderStorageBuffer(stored), G.ShaderStorageBuffer(vals)
    s.sort_typed_ptr(kb.device_ptr(), vb.device_ptr(), code.size, "float32")
    G.synchronize()
    fin = s.read_finish()
    assert fin["attempted"] == 1 and fin["accepted"] == 1 and fin["capacity"] == BIG.tile, fin
    out = kb.get_data(np.uint32)
    out = np.where(out & top, ~out, out ^ top)
    assert (out == _input("branch_edges")[2]).all() and (vb.get_data(np.uint32) == _input("branch_edges")[3]).all()


def test_u64_keys_in_the_512_x_9_tile(G):
    """64-bit keys with values: 48 bits are left to order, a bucket is the top 12 of them (BPT = 8).  Runs with two to 24 words per
    bucket, and uniformly drawn ones."""
    T = Tile(512, 9, low_bits=48)
    assert (T.cap, T.slot_bits, T.nb, T.bpt, T.dsh) == (4640, 13, 4096, 8, 49)
    rng = np.random.default_rng(107)

    def low48(buckets, words):
        # (words of one bucket: the same top 12 of the 48 bits, descending below)
        per = [np.sort(rng.integers(0, 1 << 36, words, dtype=np.uint64))[::-1] + (np.uint64(b) << np.uint64(36)) for b in buckets]
        return _deal(per, rng)

    special = [low48(_rows(T, range(4)), 2), low48(_rows(T, range(8), range(288)), 2), low48(_rows(T, range(8), range(100, 215)), 5),
               low48(_rows(T, range(8), range(500, 512)), 9), low48(_rows(T, range(8), range(24)), BUCKET_MAX_LEN),
               low48([T.nb - 1, 0, 513], BUCKET_MAX_LEN + 1)]
    tops = rng.choice(np.arange(1, 65535), len(special) + 1200, replace=False)
    runs = [(int(t), low) for t, low in zip(tops, special)]
    runs += [(int(t), rng.integers(0, 2**48, int(rng.integers(2600, 4609)), dtype=np.uint64)) for t in tops[len(special):]]
    runs += [(t, rng.integers(0, 2**48, 3000, dtype=np.uint64)) for t in (0, 65535)]
    keys = _assemble(runs, 108, top_shift=48, dtype=np.uint64)
    vals = np.arange(keys.size, dtype=np.uint32)
    s = G.RadixSort(options=dict(SMALL, GLU_HIP_SORT_NARROW_HANDOFF=0))
    kb, vb = G.ShaderStorageBuffer(keys), G.ShaderStorageBuffer(vals)
    s(kb, vb, keys.size, 0, key_bytes=8)
    G.synchronize()
    fin = s.read_finish()
    assert fin["attempted"] == 1 and fin["accepted"] == 1 and fin["capacity"] == T.tile and fin["top_bit"] == 64, fin
    ek, ev = O.stable_sort_pairs(keys, vals)
    assert (kb.get_data(np.uint64) == ek).all() and (vb.get_data(np.uint32) == ev).all()
