"""GPU tests of the batched set operations (glu_set_ops_run_batch_offsets_ptr, glu_set_ops_run_batch_ptr): union, intersection,
difference and symmetric difference of the two sorted runs of every segment, all segments in one call.  The oracle is the textbook
two-pointer walk of every segment's two runs (test_set_ops_batch_path.two_pointer, on encoded keys), the kept elements back to back;
the expected keys are compared as bit patterns, the expected values are A's iota and B's iota + 2^31, so the side and the place every
output came from are visible.  Every comparison is `==`.  Every array the call writes sits inside an allocation with poison in front
of it and behind it and is itself filled with poison first: what lies behind out[min(S, max_out)) must come back intact.  The inputs
and the offsets are checked unchanged; last() is checked against plan_set_ops_batch.  Sizes are a handful of tiles.  The helpers are
test_gpu_merge.py's and test_gpu_merge_batch.py's."""
import ctypes
import gc
import os
import subprocess

import numpy as np
import pytest

import test_gpu_merge as mg
from test_gpu_merge import Array, B_VALS, KEYS, POISON, enc, stream
from test_gpu_merge_batch import offsets_of
from test_set_ops_batch_path import keeps, two_pointer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["union", "intersection", "difference", "symmetric_difference"]
POISON_WORD = 0xA5A5A5A5


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def tile_of(G, key_type):
    return G.plan_set_ops_batch(1, 1, 1, key_type)[0]


def bound_of(op, na, nb):
    return na + nb if op in ("union", "symmetric_difference") else (na if op == "difference" else min(na, nb))


class Oracle:
    """The two-pointer walk of every segment, once per input; per operation the kept sources (indices into A || B, in output order) and
    the cardinality of every segment."""

    def __init__(self, a, b, a_off, b_off):
        self.a, self.b = a, b
        u = KEYS[str(a.dtype)]
        ea, eb = enc(a).tolist(), enc(b).tolist()
        ao, bo = np.asarray(a_off, dtype=np.int64), np.asarray(b_off, dtype=np.int64)
        self.S = len(ao) - 1
        self.events = {}
        for s in np.flatnonzero(np.diff(ao) + np.diff(bo)):
            ra, rb = ea[ao[s]:ao[s + 1]], eb[bo[s]:bo[s + 1]]
            assert ra == sorted(ra) and rb == sorted(rb), "the test's inputs are not sorted inside a segment"
            self.events[int(s)] = [(side, int(ao[s] if side == 0 else bo[s]) + x, m) for side, x, m in two_pointer(ra, rb)]
        self.bits = np.concatenate([a.view(u), b.view(u)])
        self.vals = np.concatenate([np.arange(a.size, dtype=np.uint32), np.arange(b.size, dtype=np.uint32) + np.uint32(B_VALS)])
        self.by_op = {}

    def of(self, op):
        """(keys as bit patterns, values, cardinalities per segment)"""
        if op not in self.by_op:
            code = OPS.index(op)
            src, card = [], np.zeros(self.S, dtype=np.int64)
            for s, ev in self.events.items():
                kept = [x if side == 0 else self.a.size + x for side, x, m in ev if keeps(code, side, m)]
                card[s] = len(kept)
                src.append((s, kept))
            src = np.array([x for _, kept in sorted(src) for x in kept], dtype=np.int64)
            self.by_op[op] = (self.bits[src], self.vals[src], card)
        return self.by_op[op]


def check_batch(G, so, op, a, b, a_off=None, b_off=None, equal=None, with_vals=True, with_offsets=True, max_out=None, count_only=False,
                shifts=(0, 0, 0, 0, 0, 0), oracle=None, malformed=False, b_vals_anyway=False):
    """One call.  `a` and `b`: whole arrays of one of the six key types.  a_off / b_off: the offset words (any integers, they go to the
    device as uint32), or equal = (a_len, b_len, segments).  max_out None: room to spare.  count_only: out_keys is NULL.  shifts: bytes
    behind a 16-byte boundary of a_keys, a_vals, b_keys, b_vals, out_keys, out_vals.  b_vals is passed only where the operation can
    write elements of B (else NULL: it must not be read), unless b_vals_anyway.  malformed: only the poison, the inputs, last() and the
    bounds on num_out and out_offsets are checked.  Returns (the oracle, what the call wrote as bytes)."""
    import torch

    key_type = str(a.dtype)
    u, kb = KEYS[key_type], a.dtype.itemsize
    if equal:
        a_len, b_len, S = equal
        assert a.size == a_len * S and b.size == b_len * S
        a_off, b_off = np.arange(S + 1, dtype=np.int64) * a_len, np.arange(S + 1, dtype=np.int64) * b_len
    S = len(a_off) - 1
    bound = bound_of(op, a.size, b.size)
    max_out = bound + 9 if max_out is None else max_out
    with_arrays = not count_only and max_out > 0
    with_vals = with_vals and with_arrays
    room = min(bound, max_out) if with_arrays else 0
    av, bv = np.arange(a.size, dtype=np.uint32), np.arange(b.size, dtype=np.uint32) + np.uint32(B_VALS)
    ak, bk = Array(a.view(u), shifts[0]), Array(b.view(u), shifts[2])
    ava, bva = Array(av, shifts[1]), Array(bv, shifts[3])
    ok, ov = Array.poisoned(kb * (bound + 3), shifts[4]), Array.poisoned(4 * (bound + 3), shifts[5])
    oo, no = Array.poisoned(4 * (S + 1)), Array.poisoned(4)
    ao32, bo32 = np.asarray(a_off).astype(np.uint32), np.asarray(b_off).astype(np.uint32)
    aoa, boa = Array(ao32), Array(bo32)
    p = lambda arr, n, on=True: arr.ptr if n and on else None  # noqa: E731  (an array of no elements passes NULL)
    b_vals_on = with_vals and (b_vals_anyway or op in ("union", "symmetric_difference"))
    tail = dict(out_offsets_ptr=oo.ptr if with_offsets else None, key_type=key_type, stream=stream())
    out_k = None if count_only else ok.ptr
    if equal:
        so.run_batch_ptr(op, p(ak, a.size), p(ava, a.size, with_vals), equal[0], p(bk, b.size), p(bva, b.size, b_vals_on), equal[1], S, out_k,
                         ov.ptr if with_vals else None, max_out, no.ptr, **tail)
    else:
        so.run_batch_offsets_ptr(op, p(ak, a.size), p(ava, a.size, with_vals), aoa.ptr, a.size, p(bk, b.size), p(bva, b.size, b_vals_on), boa.ptr,
                                 b.size, S, out_k, ov.ptr if with_vals else None, max_out, no.ptr, **tail)
    torch.cuda.synchronize()
    what = (op, key_type, a.size, b.size, S, with_vals, with_offsets, max_out, count_only, shifts)
    assert so.last() == G.plan_set_ops_batch(a.size, b.size, S, key_type, with_arrays, with_offsets)[1:3], (what, so.last())
    got_keys, got_vals, got_offsets, got_n = ok.result(u), ov.result(np.uint32), oo.result(np.uint32), int(no.result(np.uint32)[0])
    assert (ak.result(u) == a.view(u)).all() and (bk.result(u) == b.view(u)).all(), "the call wrote to its keys"
    assert (ava.result(np.uint32) == av).all() and (bva.result(np.uint32) == bv).all(), "the call wrote to its values"
    assert (aoa.result(np.uint32) == ao32).all() and (boa.result(np.uint32) == bo32).all(), "the call wrote to its offsets"
    if not with_vals:
        assert (got_vals.view(np.uint8) == POISON).all(), (what, "no values, and out_vals was written")
    if not with_offsets:
        assert (got_offsets.view(np.uint8) == POISON).all(), (what, "no out_offsets, and it was written")
    wrote = (got_keys.tobytes(), got_vals.tobytes(), got_offsets.tobytes(), got_n)
    if malformed:
        assert got_n <= bound, (what, got_n)
        assert not with_offsets or (got_offsets <= (room if with_arrays else bound)).all(), (what, got_offsets.max())
        assert (got_keys[room:].view(np.uint8) == POISON).all() and (got_vals[room:].view(np.uint8) == POISON).all(), what
        return None, wrote
    oracle = oracle or Oracle(a, b, a_off, b_off)
    keys, vals, card = oracle.of(op)
    total, running = keys.size, np.concatenate([[0], np.cumsum(card)])
    assert got_n == total, (what, "num_out", got_n, total)
    if with_offsets:
        want = np.minimum(running, max_out) if with_arrays else running
        bad = np.flatnonzero(got_offsets != want)
        assert bad.size == 0, (what, "out_offsets", int(bad[0]), int(got_offsets[bad[0]]), int(want[bad[0]]))
    n = min(total, room)
    bad = np.flatnonzero(got_keys[:n] != keys[:n])
    assert bad.size == 0, (what, "keys", int(bad[0]), int(got_keys[bad[0]]), int(keys[bad[0]]))
    assert (got_keys[n:].view(np.uint8) == POISON).all(), (what, "out_keys was written behind the last output")
    if with_vals:
        bad = np.flatnonzero(got_vals[:n] != vals[:n])
        assert bad.size == 0, (what, "values", int(bad[0]), int(got_vals[bad[0]]), int(vals[bad[0]]))
        assert (got_vals[n:].view(np.uint8) == POISON).all(), (what, "out_vals was written behind the last output")
    return oracle, wrote


def ragged(rng, dtype, lens_a, lens_b, spread=1 << 12, front=(0, 0), slack=(0, 0)):
    """Sorted runs per segment of an unsigned type, every segment over the SAME key range: only the offsets keep the segments apart."""
    dtype = np.dtype(dtype)

    def side(lens, first, extra):
        off = offsets_of(lens, first)
        keys = rng.integers(0, spread, int(off[-1]) + extra).astype(dtype)
        for s in range(len(lens)):
            keys[off[s]:off[s + 1]] = np.sort(rng.integers(0, spread, int(lens[s]))).astype(dtype)
        return keys, off

    a, ao = side(lens_a, front[0], slack[0])
    b, bo = side(lens_b, front[1], slack[1])
    return a, b, ao, bo


def every_op(G, so, a, b, a_off=None, b_off=None, **kw):
    oracle = kw.pop("oracle", None)
    for op in OPS:
        oracle, _ = check_batch(G, so, op, a, b, a_off, b_off, oracle=oracle, **kw)
    return oracle


def test_tiny(G):
    """1 and 2 segments of 0 to 5 elements, every combination of empty sides, keys from {0 .. 3}; no segments at all."""
    so = G.SetOps()
    rng = np.random.default_rng(1)
    for S in (1, 2):
        for pattern in range(4 ** S):
            kinds = [(pattern >> (2 * s)) & 3 for s in range(S)]  # bit 0: A has elements, bit 1: B has
            la = [int(rng.integers(1, 6)) if k & 1 else 0 for k in kinds]
            lb = [int(rng.integers(1, 6)) if k & 2 else 0 for k in kinds]
            a, b, ao, bo = ragged(rng, np.uint32, la, lb, spread=4)
            every_op(G, so, a, b, ao, bo, with_vals=pattern % 3 != 0)
    # num_segments == 0: *num_out = 0, out_offsets[0] = 0 and nothing else
    a = np.arange(5, dtype=np.uint32)
    for op in OPS:
        check_batch(G, so, op, a, a.copy(), np.zeros(1), np.zeros(1))
        assert so.last() == (1, 1)
    assert G.plan_set_ops_batch(0, 0, 3)[1:3] == (0, 2) and G.plan_set_ops_batch(1, 0, 3)[1:3] == (1, 5)


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_equal_keys_across_a_segment_boundary(G, key_type):
    """A_0 ends with k and B_1 begins with k; B_1 ends with k' and A_2 begins with k'; the boundary of segments 0 and 1 one in front of
    a tile boundary, on it, one behind it and in the middle of a tile.  An intersection must not keep them, a difference must."""
    T = tile_of(G, key_type)
    rng = np.random.default_rng(2)
    so = G.SetOps()
    u = np.dtype(key_type)
    draw = lambda n, lo, hi: np.sort(rng.integers(lo, hi, n)).astype(u)  # noqa: E731
    for first in (T - 1, T, T + 1, T // 2):
        la, q = first // 3, T // 4
        a = np.concatenate([draw(la - 1, 0, 49), [49], draw(q, 50, 61), [61], draw(q - 1, 62, 80)]).astype(u)
        b = np.concatenate([draw(first - la, 0, 49), [49], draw(q - 2, 50, 61), [61], draw(q, 62, 80)]).astype(u)
        ao, bo = [0, la, la + q, la + 2 * q], [0, first - la, first - la + q, first - la + 2 * q]
        oracle = every_op(G, so, a, b, ao, bo)
        assert so.last()[0] in (2, 3)
        _, inter_vals, _ = oracle.of("intersection")
        _, diff_vals, _ = oracle.of("difference")
        assert la - 1 not in inter_vals and la - 1 in diff_vals and la + q not in inter_vals and la + q in diff_vals


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_a_run_longer_than_a_tile_that_ends_beside_a_segment_boundary(G, key_type):
    """m copies of one key in A and n in B inside segment 0, both longer than a tile, m <, == and > n; the tile where the run ends holds
    two more segments with the same key: the starts of the run are searched in the right segment."""
    T = tile_of(G, key_type)
    so = G.SetOps()
    u = np.dtype(key_type)
    for m, n in ((T + 100, T + 300), (T + 200, T + 200), (T + 300, T + 100), (2 * T + 50, 3), (3, 2 * T + 50)):
        a = np.concatenate([[1, 2], np.full(m, 7), [9], [7, 7, 8], [7]]).astype(u)
        b = np.concatenate([[2, 3], np.full(n, 7), [9, 9], [7, 8, 8], [7, 7]]).astype(u)
        every_op(G, so, a, b, [0, m + 3, m + 6, m + 7], [0, n + 4, n + 7, n + 9])


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_a_partner_outside_the_staged_part(G, key_type):
    """40 copies of k in A_0 against 20 in B_0 behind three tiles of smaller keys, B_1 beginning with 25 more copies of k: the partners
    of A's copies lie in the next tile (read from memory), and those of ranks 20 .. 39 lie in B_1: the end of B_0 decides."""
    T = tile_of(G, key_type)
    rng = np.random.default_rng(3)
    so = G.SetOps()
    u = np.dtype(key_type)
    for small in (3 * T - 20, 3 * T - 45, 2 * T + 1):
        a = np.concatenate([np.full(40, 5), [6], np.full(30, 5)]).astype(u)
        b = np.concatenate([np.sort(rng.integers(0, 5, small)), np.full(20, 5), np.full(25, 5), [6]]).astype(u)
        oracle = every_op(G, so, a, b, [0, 41, 71], [0, small + 20, small + 46])
        assert oracle.of("intersection")[2].tolist() == [20, 25] and oracle.of("difference")[2].tolist() == [21, 5]


def test_empty_segments(G):
    """Segments empty on one side and on both; 2^16 empty segments at one position between two full ones: every out_offsets entry is
    written (check_batch compares all of them)."""
    T = tile_of(G, "uint32")
    rng = np.random.default_rng(4)
    so = G.SetOps()
    lens = rng.integers(0, 900, 12)
    alt = np.arange(12) % 3
    a, b, ao, bo = ragged(rng, np.uint32, lens * (alt != 0), lens[::-1] * (alt != 1), spread=300)
    every_op(G, so, a, b, ao, bo)
    S = (1 << 16) + 2
    la, lb = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    la[0], lb[0], la[-1], lb[-1] = T // 2, T, T + 9, T // 3
    a, b, ao, bo = ragged(rng, np.uint32, la, lb, spread=700)
    oracle = every_op(G, so, a, b, ao, bo)
    check_batch(G, so, "intersection", a, b, ao, bo, count_only=True, oracle=oracle)
    a, b, ao, bo = ragged(rng, np.uint64, la, lb, spread=700)
    check_batch(G, so, "symmetric_difference", a, b, ao, bo, with_vals=False)


def test_many_segments_a_tile(G):
    """A thousand rows of 3 to 40 keys a side from a small range: every tile holds dozens of segments."""
    rng = np.random.default_rng(5)
    so = G.SetOps()
    a, b, ao, bo = ragged(rng, np.uint32, rng.integers(3, 41, 1000), rng.integers(3, 41, 1000), spread=30)
    oracle = every_op(G, so, a, b, ao, bo)
    assert so.last()[0] >= 6
    assert (oracle.of("intersection")[2] > 0).sum() > 900 and (oracle.of("difference")[2] > 0).sum() > 900
    a, b, ao, bo = ragged(rng, np.uint64, rng.integers(3, 41, 300), rng.integers(3, 41, 300), spread=30)
    every_op(G, so, a, b, ao, bo)


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_one_segment_is_the_single_call_byte_for_byte(G, key_type):
    """One segment over all tiles: what glu_set_ops_run_ptr writes for the same arrays, num_out included."""
    import torch

    T = tile_of(G, key_type)
    rng = np.random.default_rng(6)
    na, nb = 2 * T + 100, T + T // 2
    a, b, ao, bo = ragged(rng, key_type, [na], [nb], spread=2 * T)
    u, kb = KEYS[key_type], a.dtype.itemsize
    so = G.SetOps()
    oracle = None
    for op in OPS:
        oracle, wrote = check_batch(G, so, op, a, b, ao, bo, oracle=oracle)
        assert so.last()[0] >= 3
        bound = bound_of(op, na, nb)
        ak, bk, ava = Array(a.view(u)), Array(b.view(u)), Array(np.arange(na, dtype=np.uint32))
        bva = Array(np.arange(nb, dtype=np.uint32) + np.uint32(B_VALS))
        ok, ov, no = Array.poisoned(kb * (bound + 3)), Array.poisoned(4 * (bound + 3)), Array.poisoned(4)
        so.run_ptr(op, ak.ptr, ava.ptr, na, bk.ptr, bva.ptr, nb, ok.ptr, ov.ptr, bound + 9, no.ptr, key_type, stream())
        torch.cuda.synchronize()
        assert (ok.result(u).tobytes(), ov.result(np.uint32).tobytes(), int(no.result(np.uint32)[0])) == (wrote[0], wrote[1], wrote[3]), op


def test_max_out(G):
    """max_out cutting inside a segment inside a tile, at 0 and beyond S: num_out is still the true S, out_offsets are held to max_out,
    nothing at or behind out[max_out] is touched (check_batch)."""
    T = tile_of(G, "uint32")
    rng = np.random.default_rng(7)
    so = G.SetOps()
    a, b, ao, bo = ragged(rng, np.uint32, rng.integers(0, 700, 15), rng.integers(0, 700, 15), spread=2000)
    oracle = None
    for op in OPS:
        total = (oracle or Oracle(a, b, ao, bo)).of(op)[0].size
        assert total > (T + 50 if op in ("union", "symmetric_difference") else 500)  # (the cut lies in the second tile, or in the first)
        for max_out in (T + 37 if total > T + 50 else total // 2 + 37, 1, total - 1, total, total + 1, 0):
            oracle, _ = check_batch(G, so, op, a, b, ao, bo, max_out=max_out, oracle=oracle)
    check_batch(G, so, "union", a, b, ao, bo, max_out=T // 2, with_vals=False, with_offsets=False, oracle=oracle)


def test_count_only_with_out_offsets_gives_every_segments_cardinality(G):
    """A call that only counts (out_keys NULL, or max_out 0) writes no array; its out_offsets are the running cardinalities, not held to
    max_out; without out_offsets it still writes num_out."""
    rng = np.random.default_rng(8)
    so = G.SetOps()
    a, b, ao, bo = ragged(rng, np.uint32, rng.integers(0, 60, 300), rng.integers(0, 60, 300), spread=64)
    oracle = None
    for op in OPS:
        oracle, wrote = check_batch(G, so, op, a, b, ao, bo, count_only=True, oracle=oracle)
        cards = np.diff(np.frombuffer(wrote[2], dtype=np.uint32).astype(np.int64))
        assert (cards == oracle.of(op)[2]).all() and cards.sum() == wrote[3] > 1000
        check_batch(G, so, op, a, b, ao, bo, max_out=0, oracle=oracle)
        check_batch(G, so, op, a, b, ao, bo, count_only=True, max_out=5, oracle=oracle)
        check_batch(G, so, op, a, b, ao, bo, count_only=True, with_offsets=False, oracle=oracle)


@pytest.mark.parametrize("key_type", sorted(KEYS))
def test_every_key_type(G, key_type):
    """Five ragged segments with the type's specials on both sides of every segment (+-0.0, NaNs of different bits; INT_MIN / INT_MAX;
    0 / UINT_MAX), with and without values; b_vals NULL where the operation cannot write B, and given all the same."""
    T = tile_of(G, key_type)
    rng = np.random.default_rng(len(key_type) + T)
    lens_a, lens_b = [T + T // 2, 40, 0, T // 3, 900], [100, T, 50, 0, 1000]
    a = np.concatenate([mg.typed_keys(rng, n, key_type) if n else np.zeros(0, dtype=key_type) for n in lens_a])
    b = np.concatenate([mg.typed_keys(rng, n, key_type) if n else np.zeros(0, dtype=key_type) for n in lens_b])
    so = G.SetOps()
    ao, bo = offsets_of(lens_a), offsets_of(lens_b)
    oracle = every_op(G, so, a, b, ao, bo)
    every_op(G, so, a, b, ao, bo, with_vals=False, oracle=oracle)
    every_op(G, so, a, b, ao, bo, b_vals_anyway=True, oracle=oracle)
    if a.dtype.kind == "f":  # (-0.0 and +0.0 are different keys: both sides hold both, and both are matched)
        bits = oracle.of("intersection")[0]
        assert (bits == 0).any() and (bits == KEYS[key_type](1) << KEYS[key_type](8 * a.dtype.itemsize - 1)).any()


def test_offsets_not_from_zero_totals_beyond_the_last_offset_and_equal_partitions(G):
    rng = np.random.default_rng(9)
    T = tile_of(G, "uint32")
    so = G.SetOps()
    lens_a, lens_b = [5, 0, T, 3, 0, T + 1], [0, 0, 17, T + 9, 1, 700]
    a, b, ao, bo = ragged(rng, np.uint32, lens_a, lens_b, spread=900, front=(13, 6), slack=(100, 57))
    every_op(G, so, a, b, ao, bo)
    for a_len, b_len, S in ((3, 0, 500), (0, 5, 500), (7, 9, 700), (T, T - 1, 2), (0, 0, 4)):
        a, b, _, _ = ragged(rng, np.uint32, [a_len] * S, [b_len] * S, spread=8 if a_len < T else T)
        oracle = every_op(G, so, a, b, equal=(a_len, b_len, S))
        check_batch(G, so, "difference", a, b, equal=(a_len, b_len, S), with_vals=False, with_offsets=False, oracle=oracle)


def test_alignment(G):
    """Each of the six data arrays at element shifts off a 16-byte boundary, in turn and together, between poison bands; tiles inside
    a segment and tiles over several."""
    rng = np.random.default_rng(10)
    so = G.SetOps()
    T = tile_of(G, "uint32")
    a, b, ao, bo = ragged(rng, np.uint32, [T + 5, 3, 0, 40, T // 2], [11, T, 9, 0, T // 2], spread=3000)
    oracle = None
    single = [tuple(s if i == j else 0 for j in range(6)) for i in range(6) for s in (4, 12)]
    for i, shifts in enumerate(single + [(4, 8, 12, 4, 8, 12), (12, 12, 12, 12, 12, 12)]):
        oracle, _ = check_batch(G, so, OPS[i % 4], a, b, ao, bo, shifts=shifts, oracle=oracle, max_out=None if i % 3 else T + 3)
    T = tile_of(G, "uint64")
    a, b, ao, bo = ragged(rng, np.uint64, [T + 3, 2, 0, T // 2], [7, T, 5, T // 2], spread=3000)
    oracle = None
    for i, shifts in enumerate(((8, 0, 0, 0, 0, 0), (0, 0, 8, 0, 0, 0), (0, 0, 0, 0, 8, 0), (0, 4, 0, 8, 0, 12), (8, 4, 8, 12, 8, 4))):
        oracle, _ = check_batch(G, so, OPS[i % 4], a, b, ao, bo, shifts=shifts, oracle=oracle)


def test_counts_that_live_on_the_device(G):
    """A chain of two intersections with no host read between them: (A1 & A2) & A3.  The first is glu_set_ops_run_ptr, whose num_out
    lands in the second offset word of the batched call's one segment on the same stream."""
    import torch

    rng = np.random.default_rng(11)
    n = 5000
    a1, a2, a3 = (np.unique(rng.integers(0, 9000, n).astype(np.uint32)) for _ in range(3))
    first = np.intersect1d(a1, a2)
    want = np.intersect1d(first, a3)
    cap = min(a1.size, a2.size)
    dev = lambda x: torch.from_numpy(x.view(np.int32).copy()).cuda()  # noqa: E731
    t1, t2, t3 = dev(a1), dev(a2), dev(a3)
    mid = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    aot = torch.zeros(2, dtype=torch.int32, device="cuda")
    bot = dev(np.array([0, a3.size], dtype=np.uint32))
    ok = torch.full((cap,), -1515870811, dtype=torch.int32, device="cuda")
    oo, no = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    so, s = G.SetOps(), stream()
    so.run_ptr("intersection", t1.data_ptr(), None, a1.size, t2.data_ptr(), None, a2.size, mid.data_ptr(), None, cap, aot.data_ptr() + 4, "uint32", s)
    so.run_batch_offsets_ptr("intersection", mid.data_ptr(), None, aot.data_ptr(), cap, t3.data_ptr(), None, bot.data_ptr(), a3.size, 1,
                             ok.data_ptr(), None, cap, no.data_ptr(), oo.data_ptr(), "uint32", s)
    torch.cuda.synchronize()
    assert aot.cpu().numpy().tolist() == [0, first.size] and 0 < want.size < first.size < cap
    got = ok.cpu().numpy().view(np.uint32)
    assert (got[:want.size] == want).all() and (got[want.size:] == POISON_WORD).all()
    assert oo.cpu().numpy().tolist() == [0, want.size] and int(no.cpu().numpy()[0]) == want.size


def test_with_the_family(G):
    """A per-group anti-join, all on one stream with no host read in between: both sides are (group, item) composites in 64-bit keys,
    sorted by the family's sort (A beside a column of weights); key runs over the group bits of both sides give the two offsets arrays;
    the batched difference keeps, per group, A's items beyond B's copies; a batched reduce sums the kept weights over out_offsets."""
    import torch

    rng = np.random.default_rng(12)
    groups, na, nb = 200, 9000, 7000
    ga, gb = rng.integers(0, groups, na).astype(np.uint64), rng.integers(0, groups, nb).astype(np.uint64)
    ga[:groups], gb[:groups] = np.arange(groups), np.arange(groups)  # (every group on both sides: the runs of both sides line up)
    ca, cb = (ga << np.uint64(32)) | rng.integers(0, 400, na).astype(np.uint64), (gb << np.uint64(32)) | rng.integers(0, 400, nb).astype(np.uint64)
    wa = rng.integers(0, 1000, na).astype(np.uint32)
    sort, runs, so, red = G.RadixSort(), G.KeyRuns(), G.SetOps(), G.Reduce(G.DataType_Uint, G.ReduceOperator_Sum)
    s = stream()
    cak, wak, cbk = Array(ca), Array(wa), Array(cb)
    aoa, boa = Array.poisoned(4 * (groups + 1)), Array.poisoned(4 * (groups + 1))
    nra, nrb = Array.poisoned(4), Array.poisoned(4)
    ok, ov, oo, no, sums = Array.poisoned(8 * na), Array.poisoned(4 * na), Array.poisoned(4 * (groups + 1)), Array.poisoned(4), Array.poisoned(4 * groups)
    sort.sort_typed_ptr(cak.ptr, wak.ptr, na, "uint64", s)
    sort.sort_typed_ptr(cbk.ptr, None, nb, "uint64", s)
    runs.run_ptr(cak.ptr, na, aoa.ptr, groups, nra.ptr, key_bits=64, begin_bit=32, end_bit=64, stream=s)
    runs.run_ptr(cbk.ptr, nb, boa.ptr, groups, nrb.ptr, key_bits=64, begin_bit=32, end_bit=64, stream=s)
    so.run_batch_offsets_ptr("difference", cak.ptr, wak.ptr, aoa.ptr, na, cbk.ptr, None, boa.ptr, nb, groups, ok.ptr, ov.ptr, na, no.ptr, oo.ptr,
                             "uint64", s)
    red.run_batch_offsets_ptr(ov.ptr, sums.ptr, na, oo.ptr, groups, s)
    torch.cuda.synchronize()
    order = np.argsort(ca, kind="stable")
    sa, swa, sb = ca[order], wa[order], np.sort(cb)
    ao, bo = np.searchsorted(sa >> np.uint64(32), np.arange(groups + 1)), np.searchsorted(sb >> np.uint64(32), np.arange(groups + 1))
    assert int(nra.result(np.uint32)[0]) == groups == int(nrb.result(np.uint32)[0])
    assert (aoa.result(np.uint32) == ao).all() and (boa.result(np.uint32) == bo).all()
    keys, from_a, card = Oracle(sa, sb, ao, bo).of("difference")
    running = np.concatenate([[0], np.cumsum(card)])
    assert int(no.result(np.uint32)[0]) == keys.size and 0 < keys.size < na and (oo.result(np.uint32) == running).all()
    assert (ok.result(np.uint64)[:keys.size] == keys).all() and (ov.result(np.uint32)[:keys.size] == swa[from_a]).all()
    want = [int(swa[from_a[running[g]:running[g + 1]]].sum(dtype=np.uint64)) & 0xFFFFFFFF for g in range(groups)]
    assert sums.result(np.uint32).tolist() == want


def test_prepared_captured_replayed(G, monkeypatch):
    """After prepare_batch a call leaves the device's free memory as it found it, and one call captured on one stream (no parallel
    branches) is replayed on other keys AND other offsets of the same capacity.  The scratch does not grow behind prepare_batch."""
    import torch

    monkeypatch.setenv("GLU_HIP_SCRATCH_FILL", "0x5A")
    T = tile_of(G, "uint32")
    S, cap_a, cap_b = 50, 3 * T + 3, 2 * T + 1
    rng = np.random.default_rng(90)
    so = G.SetOps()
    at, bt = torch.empty(cap_a, dtype=torch.int32, device="cuda"), torch.empty(cap_b, dtype=torch.int32, device="cuda")
    avt = torch.arange(cap_a, dtype=torch.int32, device="cuda")
    bvt = torch.from_numpy((np.arange(cap_b, dtype=np.uint32) + np.uint32(B_VALS)).view(np.int32)).cuda()
    aot, bot = torch.empty(S + 1, dtype=torch.int32, device="cuda"), torch.empty(S + 1, dtype=torch.int32, device="cuda")
    ok, ov = torch.empty(cap_a + cap_b, dtype=torch.int32, device="cuda"), torch.empty(cap_a + cap_b, dtype=torch.int32, device="cuda")
    oo, no = torch.empty(S + 1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def contents(used_a, used_b, empty_every):
        def lens(used):
            return np.diff(np.concatenate([[0], np.sort(rng.integers(0, used, S - 1)), [used]]))
        la, lb = lens(used_a), lens(used_b)
        if empty_every:
            keep = np.arange(S) % empty_every == 0
            la, lb = la * keep, lb * keep
        return ragged(rng, np.uint32, la, lb, spread=500, slack=(cap_a - int(la.sum()), cap_b - int(lb.sum())))

    def fill(a, b, ao, bo):
        at.copy_(torch.from_numpy(a.view(np.int32)))
        bt.copy_(torch.from_numpy(b.view(np.int32)))
        aot.copy_(torch.from_numpy(ao.astype(np.uint32).view(np.int32)))
        bot.copy_(torch.from_numpy(bo.astype(np.uint32).view(np.int32)))
        for t in (ok, ov, oo, no):
            t.fill_(-1515870811)

    def verify(a, b, ao, bo):
        keys, vals, card = Oracle(a, b, ao, bo).of("symmetric_difference")
        got_k, got_v = ok.cpu().numpy().view(np.uint32), ov.cpu().numpy().view(np.uint32)
        assert (got_k[:keys.size] == keys).all() and (got_v[:keys.size] == vals).all()
        assert (got_k[keys.size:] == POISON_WORD).all() and (got_v[keys.size:] == POISON_WORD).all()
        assert (oo.cpu().numpy().view(np.uint32) == np.concatenate([[0], np.cumsum(card)])).all()
        assert int(no.cpu().numpy().view(np.uint32)[0]) == keys.size

    def call(s):
        so.run_batch_offsets_ptr("symmetric_difference", at.data_ptr(), avt.data_ptr(), aot.data_ptr(), cap_a, bt.data_ptr(), bvt.data_ptr(),
                                 bot.data_ptr(), cap_b, S, ok.data_ptr(), ov.data_ptr(), cap_a + cap_b, no.data_ptr(), oo.data_ptr(), "uint32", s)

    with torch.cuda.stream(side):
        data = contents(cap_a, cap_b, 0)
        fill(*data)
        side.synchronize()
        before = G.scratch_filled_bytes()
        so.prepare_batch(cap_a + cap_b, S, "uint32")
        filled = G.scratch_filled_bytes()
        assert filled - before >= G.plan_set_ops_batch(cap_a, cap_b, S)[3] > 0
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(*data)
        fill(*data)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        assert so.last() == (6, 5) == G.plan_set_ops_batch(cap_a, cap_b, S)[1:3]
        verify(*data)
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        for used_a, used_b, empty_every in ((cap_a, cap_b, 0), (2 * T, T + 7, 3), (T // 2, 1, 7), (cap_a - 1, T, 2)):
            data = contents(used_a, used_b, empty_every)
            fill(*data)
            graph.replay()
            side.synchronize()
            verify(*data)
        fill(*data)
        call(side.cuda_stream)  # (and an ordinary call on the last contents)
        side.synchronize()
        verify(*data)
        assert G.scratch_filled_bytes() == filled, "a call behind prepare_batch grew the scratch"


@pytest.mark.parametrize("prepared", [False, True], ids=["grows_in_the_call", "prepared"])
@pytest.mark.parametrize("kind", ["u32pairs", "u64keys"])
def test_scratch_fill(G, monkeypatch, kind, prepared):
    """Fresh objects under GLU_HIP_SCRATCH_FILL = 0x00, 0xFF and 0x5A (the method of test_gpu_scratch_fill.py): the bounds, the tile
    counts and the threads' words are all written by the bounds and the count kernel before the scan, the offsets and the write kernel
    read them, so every fill gives the oracle's bytes -- also in a call whose device total is tiles short of the host's."""
    import test_gpu_scratch_fill as sf

    key_type, with_vals = ("uint32", True) if kind == "u32pairs" else ("uint64", False)
    T = tile_of(G, key_type)
    rng = np.random.default_rng(13)
    lens_a, lens_b = [T, 0, 5, T + 5, 40], [3, 0, T, T // 2, 0]
    a, b, ao, bo = ragged(rng, key_type, lens_a, lens_b, spread=2000, slack=(T + 9, T))
    oracle = Oracle(a, b, ao, bo)
    held = G.plan_set_ops_batch(a.size, b.size, 5, key_type)[3]

    def case():
        so = G.SetOps()
        if prepared:
            so.prepare_batch(a.size + b.size, 5, key_type)
        told = {}
        for op in OPS:
            told[op] = check_batch(G, so, op, a, b, ao, bo, with_vals=with_vals, oracle=oracle)[1]
        told["count"] = check_batch(G, so, "intersection", a, b, ao, bo, count_only=True, oracle=oracle)[1]
        return held, dict(told, last=so.last())

    sf.under_every_fill(G, monkeypatch, case)


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_malformed_offsets_and_shuffled_keys_stay_inside_their_arrays(G, key_type):
    """The malformed cases of tests/test_set_ops_batch_path.py (which walks them on the host, under the sanitizers too), at most 10 000
    elements: ordinary calls that the contract defines.  The poison around every output and behind min(bound, max_out) is intact, the
    inputs and the offsets are unchanged, num_out <= bound and every out_offsets entry <= min(bound, max_out); the contents are
    unspecified and not looked at."""
    rng = np.random.default_rng(14)
    S = 40
    a, b, ao, bo = ragged(rng, key_type, rng.integers(0, 200, S), rng.integers(0, 200, S), spread=500)
    assert tile_of(G, key_type) < a.size + b.size <= 10000
    so = G.SetOps()
    ones = np.full(S + 1, 0xFFFFFFFF, dtype=np.int64)
    cases = [(ao[::-1].copy(), bo), (ao[::-1].copy(), bo[::-1].copy()), (ao * 2 + 5, bo + b.size),
             (np.where(np.arange(S + 1) > 20, ao + a.size, ao), bo), (ones, ones), (ones, bo),
             (rng.integers(0, 1 << 32, S + 1), rng.integers(0, 1 << 32, S + 1)),
             (rng.integers(0, a.size + 9, S + 1), rng.integers(0, b.size + 9, S + 1)),
             (np.where(np.arange(S + 1) % 2, a.size, 0), np.sort(rng.integers(0, b.size, S + 1)))]
    for i, (a_off, b_off) in enumerate(cases):
        check_batch(G, so, OPS[i % 4], a, b, a_off, b_off, malformed=True)
        check_batch(G, so, OPS[(i + 1) % 4], a, b, a_off, b_off, malformed=True, max_out=700 + i, with_vals=i % 2 == 0)
    for i, op in enumerate(OPS):
        check_batch(G, so, op, rng.permutation(a), rng.permutation(b), ao, bo, malformed=True, max_out=None if i % 2 else 1000,
                    shifts=(0, 4, 8, 12, 8, 4) if key_type == "uint32" else (8, 4, 0, 12, 8, 4))
        check_batch(G, so, op, rng.permutation(a), b[::-1].copy(), rng.integers(0, a.size + 9, S + 1), bo, malformed=True, count_only=i == 2)


def test_argument_errors(G):
    """What the host can check: each INVALID_ARGUMENT with its own message, and a witness buffer shows that nothing was written."""
    import torch

    so = G.SetOps()
    n, S = 4096, 8
    keys = np.arange(n, dtype=np.uint32)
    at, bt = torch.from_numpy(keys.view(np.int32).copy()).cuda(), torch.from_numpy(keys.view(np.int32).copy()).cuda()
    avt, bvt = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    offs = torch.from_numpy((np.arange(S + 1, dtype=np.uint32) * 8).view(np.int32).copy()).cuda()
    aot, bot = offs.clone(), offs.clone()
    wt = torch.zeros(8 * n, dtype=torch.int32, device="cuda")  # the witness: out_keys, out_vals, out_offsets, num_out
    ap, bp, avp, bvp, aop, bop, wp = (t.data_ptr() for t in (at, bt, avt, bvt, aot, bot, wt))
    okp, ovp, oop, nop = wp, wp + 8 * n, wp + 16 * n, wp + 24 * n
    L, vp = G.lib(), ctypes.c_void_p

    def run(op="union", a=ap, av=avp, ao=aop, na=64, b=bp, bv=bvp, bo=bop, nb=64, S=S, ok=okp, ov=ovp, max_out=128, no=nop, oo=oop, key_type="uint32"):
        so.run_batch_offsets_ptr(op, a, av, ao, na, b, bv, bo, nb, S, ok, ov, max_out, no, oo, key_type)

    def equal(op="union", a=ap, av=avp, a_len=8, b=bp, bv=bvp, b_len=8, S=S, ok=okp, ov=ovp, max_out=128, no=nop, oo=oop, key_type="uint32"):
        so.run_batch_ptr(op, a, av, a_len, b, bv, b_len, S, ok, ov, max_out, no, oo, key_type)

    def raw(set_ops=None, op=0, key_type=0):
        return G.check(L.glu_set_ops_run_batch_offsets_ptr(set_ops, op, vp(ap), vp(avp), vp(aop), 64, vp(bp), vp(bvp), vp(bop), 64, S, vp(okp),
                                                           vp(ovp), 128, vp(oop), vp(nop), key_type, None))

    bad = [
        (lambda: raw(), "set_ops is NULL"),
        (lambda: G.check(L.glu_set_ops_run_batch_ptr(None, 0, vp(ap), vp(avp), 8, vp(bp), vp(bvp), 8, S, vp(okp), vp(ovp), 128, vp(oop), vp(nop), 0,
                                                     None)), "set_ops is NULL"),
        (lambda: G.check(L.glu_set_ops_prepare_batch(None, 64, 1, 0)), "set_ops is NULL"),
        (lambda: raw(so._h, op=4), "op must be one of"),
        (lambda: raw(so._h, op=-1), "op must be one of"),
        (lambda: raw(so._h, key_type=6), "Invalid key type"),
        (lambda: G.check(L.glu_set_ops_prepare_batch(so._h, 64, 1, 9)), "Invalid key type"),
        (lambda: run(a=None), "Invalid a_keys buffer"),
        (lambda: run(b=None), "Invalid b_keys buffer"),
        (lambda: equal(no=None), "Invalid num_out pointer"),
        (lambda: run(av=None), "a_vals and out_vals must both be given or both be NULL"),
        (lambda: run(ov=None), "a_vals and out_vals must both be given or both be NULL"),
        (lambda: run(bv=None), "b_vals is required"),
        (lambda: equal(op="symmetric_difference", bv=None), "b_vals is required"),
        (lambda: run(ok=None), "out_vals needs out_keys"),
        (lambda: equal(max_out=0), "out_vals needs out_keys"),
        (lambda: run(ao=None), "Invalid a_offsets array"),
        (lambda: run(bo=None), "Invalid b_offsets array"),
        (lambda: run(ao=aop + 2), "a_offsets is not aligned"),
        (lambda: run(bo=bop + 1), "b_offsets is not aligned"),
        (lambda: run(oo=oop + 2), "out_offsets is not aligned"),
        (lambda: run(no=nop + 2), "num_out is not aligned"),
        (lambda: run(a=ap + 2), "a_keys is not aligned"),
        (lambda: run(b=bp + 4, key_type="int64"), "b_keys is not aligned"),
        (lambda: equal(ok=okp + 4, key_type="float64"), "out_keys is not aligned"),
        (lambda: run(av=avp + 1), "a_vals is not aligned"),
        (lambda: run(bv=bvp + 2), "b_vals is not aligned"),
        (lambda: equal(ov=ovp + 3), "out_vals is not aligned"),
        (lambda: run(ok=ap), "out_keys overlaps a_keys"),
        (lambda: run(ok=bp - 4 * 127), "out_keys overlaps b_keys"),
        (lambda: run(ok=aop + 4 * S), "out_keys overlaps a_offsets"),
        (lambda: run(ov=bvp + 128), "out_vals overlaps b_vals"),
        (lambda: run(ov=bop), "out_vals overlaps b_offsets"),
        (lambda: run(ov=okp + 4 * 127), "out_vals overlaps out_keys"),
        (lambda: run(oo=aop), "out_offsets overlaps a_offsets"),
        (lambda: run(oo=ap + 4 * 63), "out_offsets overlaps a_keys"),
        (lambda: run(oo=okp + 4 * 127), "out_offsets overlaps out_keys"),
        (lambda: equal(oo=ovp), "out_offsets overlaps out_vals"),
        (lambda: run(no=bp), "num_out overlaps b_keys"),
        (lambda: run(no=bop + 4), "num_out overlaps b_offsets"),
        (lambda: run(no=okp + 4), "num_out overlaps out_keys"),
        (lambda: equal(no=oop + 4 * S), "num_out overlaps out_offsets"),
        (lambda: run(S=(1 << 24) + 1), "exceeds 2^24"),
        (lambda: equal(S=(1 << 24) + 1, a_len=1, b_len=1), "exceeds 2^24"),
        (lambda: so.prepare_batch(64, (1 << 24) + 1), "exceeds 2^24"),
        (lambda: run(na=1 << 31, nb=1 << 31), "a_count + b_count below 2^32"),
        (lambda: equal(a_len=1 << 20, b_len=1 << 20, S=1 << 11), "a_count + b_count below 2^32"),
        (lambda: equal(a_len=1 << 32, b_len=0, S=1), "a_count + b_count below 2^32"),
        (lambda: so.prepare_batch(1 << 32), "a_count + b_count below 2^32"),
        (lambda: run(max_out=1 << 32), "max_out"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, (i, e.value.message)
        assert message in e.value.message, (i, e.value.message)
    torch.cuda.synchronize()
    assert (wt.cpu().numpy() == 0).all(), "a refused call wrote something"
    assert (at.cpu().numpy().view(np.uint32) == keys).all() and (aot.cpu().numpy() == offs.cpu().numpy()).all()
    # the intersection may overlap what only the union's bound covers: out_keys behind min(a_total, b_total) entries is not the call's
    run(op="intersection", ov=okp + 4 * 64)
    for good in (run, equal):  # (the same arguments, none changed, are a good call: A's keys, every one matched)
        wt.zero_()
        good()
        torch.cuda.synchronize()
        got = wt.cpu().numpy().view(np.uint32)
        assert (got[:64] == np.arange(64)).all() and (got[64:128] == 0).all()
        assert (got[4 * n:4 * n + S + 1] == np.arange(S + 1) * 8).all() and got[6 * n] == 64


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_set_ops_batch_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
