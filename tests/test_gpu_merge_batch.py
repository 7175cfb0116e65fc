"""GPU tests of the batched merge (glu_merge_run_batch_offsets_ptr, glu_merge_run_batch_ptr): the two sorted runs of every segment
into one, all segments in one call.  The oracle is always numpy: order = lexsort((side, enc(key), segment)) over the elements the
offsets cover; the expected keys are compared as bit patterns, the expected values are A's iota and B's iota + 2^31, so the side and
the place every output came from are visible.  Every comparison is `==`.  Every array the call writes sits inside an allocation with
poison in front of it and behind it and is itself filled with poison first: what lies behind the last output must come back intact.
The inputs and the offsets are checked unchanged; last() is checked against plan_merge_batch.  The helpers are test_gpu_merge.py's."""
import ctypes
import gc
import os
import subprocess

import numpy as np
import pytest

import test_gpu_merge as mg
from test_gpu_merge import Array, B_VALS, KEYS, POISON, enc, stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def tile_of(G, key_type):
    return G.plan_merge_batch(1, 1, key_type)[0]


def offsets_of(lens, first=0):
    return (np.concatenate([[0], np.cumsum(lens)]) + first).astype(np.int64)


def oracle(a, b, a_off, b_off):
    """(keys as bit patterns, values, out_offsets) of the stable sort by (segment, enc(key), side) of what the offsets cover."""
    u = KEYS[str(a.dtype)]
    ia, ib = np.arange(a_off[0], a_off[-1]), np.arange(b_off[0], b_off[-1])
    seg = np.concatenate([np.searchsorted(a_off, ia, "right") - 1, np.searchsorted(b_off, ib, "right") - 1])
    keys = np.concatenate([enc(a)[ia], enc(b)[ib]])
    for e, off in ((enc(a), a_off), (enc(b), b_off)):
        for s in range(len(off) - 1) if len(off) <= 64 else ():
            run = e[off[s]:off[s + 1]]
            assert (run[1:] >= run[:-1]).all(), "the test's inputs are not sorted inside a segment"
    side = np.concatenate([np.zeros(ia.size, dtype=np.int8), np.ones(ib.size, dtype=np.int8)])
    order = np.lexsort((side, keys, seg))
    bits = np.concatenate([a.view(u)[ia], b.view(u)[ib]])
    vals = np.concatenate([ia.astype(np.uint32), ib.astype(np.uint32) + np.uint32(B_VALS)])
    return bits[order], vals[order], ((a_off - a_off[0]) + (b_off - b_off[0])).astype(np.uint32)


def check_batch(G, mg_, a, b, a_off=None, b_off=None, equal=None, with_vals=True, with_offsets=True, shifts=(0, 0, 0, 0, 0, 0), want=None,
                malformed=False):
    """One call.  `a` and `b`: whole arrays of one of the six key types.  a_off / b_off: the offset words (any integers, they go to the
    device as uint32), or equal = (a_len, b_len, segments).  shifts: bytes behind a 16-byte boundary of a_keys, a_vals, b_keys, b_vals,
    out_keys, out_vals.  malformed: only the poison, the inputs, last() and the bound on out_offsets are checked.  Returns the oracle's
    (keys, values, out_offsets)."""
    import torch

    key_type = str(a.dtype)
    u, kb, room = KEYS[key_type], a.dtype.itemsize, a.size + b.size
    if equal:
        a_len, b_len, S = equal
        assert a.size == a_len * S and b.size == b_len * S
        a_off, b_off = np.arange(S + 1, dtype=np.int64) * a_len, np.arange(S + 1, dtype=np.int64) * b_len
    S = len(a_off) - 1
    av, bv = np.arange(a.size, dtype=np.uint32), np.arange(b.size, dtype=np.uint32) + np.uint32(B_VALS)
    ak, bk = Array(a.view(u), shifts[0]), Array(b.view(u), shifts[2])
    ava, bva = Array(av, shifts[1]), Array(bv, shifts[3])
    ok, ov = Array.poisoned(kb * room, shifts[4]), Array.poisoned(4 * room, shifts[5])
    oo = Array.poisoned(4 * (S + 1))
    ao32, bo32 = np.asarray(a_off).astype(np.uint32), np.asarray(b_off).astype(np.uint32)
    aoa, boa = Array(ao32), Array(bo32)
    args = dict(out_offsets_ptr=oo.ptr if with_offsets else None, key_type=key_type, stream=stream())
    p = lambda arr, n, on=True: arr.ptr if n and on else None  # noqa: E731  (an array of no elements passes NULL)
    if equal:
        mg_.run_batch_ptr(p(ak, a.size), p(ava, a.size, with_vals), equal[0], p(bk, b.size), p(bva, b.size, with_vals), equal[1], S,
                          p(ok, room), p(ov, room, with_vals), **args)
    else:
        mg_.run_batch_offsets_ptr(p(ak, a.size), p(ava, a.size, with_vals), aoa.ptr, a.size, p(bk, b.size), p(bva, b.size, with_vals), boa.ptr,
                                  b.size, S, p(ok, room), p(ov, room, with_vals), **args)
    torch.cuda.synchronize()
    what = (key_type, a.size, b.size, S, with_vals, shifts)
    assert mg_.last() == G.plan_merge_batch(room, S, key_type, with_vals)[1:3], (what, mg_.last())
    got_keys, got_vals, got_offsets = ok.result(u), ov.result(np.uint32), oo.result(np.uint32)
    assert (ak.result(u) == a.view(u)).all() and (bk.result(u) == b.view(u)).all(), "the call wrote to its keys"
    assert (ava.result(np.uint32) == av).all() and (bva.result(np.uint32) == bv).all(), "the call wrote to its values"
    assert (aoa.result(np.uint32) == ao32).all() and (boa.result(np.uint32) == bo32).all(), "the call wrote to its offsets"
    if not with_vals:
        assert (got_vals.view(np.uint8) == POISON).all(), (what, "keys only, and out_vals was written")
    if not with_offsets:
        assert (got_offsets.view(np.uint8) == POISON).all(), (what, "no out_offsets, and it was written")
    if malformed:
        assert not with_offsets or (got_offsets <= room).all(), (what, got_offsets.max())
        return None
    want = want or oracle(a, b, np.asarray(a_off, dtype=np.int64), np.asarray(b_off, dtype=np.int64))
    total = want[0].size
    if with_offsets:
        assert (got_offsets == want[2]).all(), (what, "out_offsets")
    bad = np.flatnonzero(got_keys[:total] != want[0])
    assert bad.size == 0, (what, "keys", int(bad[0]), int(got_keys[bad[0]]), int(want[0][bad[0]]))
    assert (got_keys[total:].view(np.uint8) == POISON).all(), (what, "out_keys was written behind the last output")
    if with_vals:
        bad = np.flatnonzero(got_vals[:total] != want[1])
        assert bad.size == 0, (what, "values", int(bad[0]), int(got_vals[bad[0]]), int(want[1][bad[0]]))
        assert (got_vals[total:].view(np.uint8) == POISON).all(), (what, "out_vals was written behind the last output")
    return want


def ragged(rng, dtype, lens_a, lens_b, descending=True, spread=1 << 16, front=(0, 0), slack=(0, 0)):
    """Sorted runs per segment of an unsigned type; descending: later segments hold smaller keys than earlier ones."""
    dtype = np.dtype(dtype)
    S = len(lens_a)

    def side(lens, first, extra):
        off = offsets_of(lens, first)
        keys = rng.integers(0, spread, int(off[-1]) + extra).astype(dtype)
        for s in range(S):
            if lens[s]:
                keys[off[s]:off[s + 1]] = np.sort(rng.integers(0, spread, int(lens[s]))).astype(dtype) + dtype.type((S - s) * spread if descending else 0)
        return keys, off

    a, ao = side(lens_a, front[0], slack[0])
    b, bo = side(lens_b, front[1], slack[1])
    return a, b, ao, bo


def test_tiny(G):
    """1 to 3 segments of 0 to 5 elements, every combination of empty sides; no segments at all."""
    m = G.Merge()
    rng = np.random.default_rng(1)
    for S in (1, 2, 3):
        for pattern in range(4 ** S):
            kinds = [(pattern >> (2 * s)) & 3 for s in range(S)]  # bit 0: A has elements, bit 1: B has
            la = [int(rng.integers(1, 6)) if k & 1 else 0 for k in kinds]
            lb = [int(rng.integers(1, 6)) if k & 2 else 0 for k in kinds]
            a, b, ao, bo = ragged(rng, np.uint32, la, lb, spread=4)
            check_batch(G, m, a, b, ao, bo, with_vals=pattern % 3 != 0)
    assert G.plan_merge_batch(0, 3)[1:3] == (0, 1) and G.plan_merge_batch(1, 3)[1:3] == (1, 2)
    # num_segments == 0: out_offsets[0] = 0 and nothing else
    a = np.arange(5, dtype=np.uint32)
    want = (np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint32))
    check_batch(G, m, a, a.copy(), np.zeros(1), np.zeros(1), want=want)
    assert m.last() == (1, 0)


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_one_segment_is_the_single_merge_byte_for_byte(G, key_type):
    """4000 + 4500 keys (three tiles of 4-byte keys): what glu_merge_run_ptr writes for the same arrays."""
    rng = np.random.default_rng(2)
    a, b = mg.uniform(rng, 4000, key_type), mg.uniform(rng, 4500, key_type)
    m = G.Merge()
    single = mg.check_case(G, m, a, b)
    keys, vals, offs = check_batch(G, m, a, b, [0, 4000], [0, 4500])
    assert (keys == single[0]).all() and (vals == single[1]).all() and offs.tolist() == [0, 8500]
    assert m.last()[0] >= 3
    check_batch(G, m, a, b, [0, 4000], [0, 4500], with_vals=False, with_offsets=False)


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_segment_boundaries_on_and_beside_a_tile_boundary(G, key_type):
    T = tile_of(G, key_type)
    rng = np.random.default_rng(3)
    m = G.Merge()
    for first in (T - 1, T, T + 1):
        la = first // 3
        a, b, ao, bo = ragged(rng, key_type, [la, T // 4], [first - la, T // 4])
        check_batch(G, m, a, b, ao, bo)
        assert m.last() == (2, 2)


def test_many_segments_a_tile(G):
    """1000 ragged segments of 0 to 8 elements a side, later segments holding smaller keys, values an iota: segment order and
    stability (few distinct keys a segment) are both visible."""
    rng = np.random.default_rng(4)
    m = G.Merge()
    a, b, ao, bo = ragged(rng, np.uint32, rng.integers(0, 9, 1000), rng.integers(0, 9, 1000), spread=3)
    keys, vals, _ = check_batch(G, m, a, b, ao, bo)
    assert m.last()[0] >= 2 and (np.diff(keys.astype(np.int64)) < 0).sum() > 500  # (a merge that ignored the segments would sort them away)
    a, b, ao, bo = ragged(rng, np.uint64, rng.integers(0, 9, 1000), rng.integers(0, 9, 1000), spread=3)
    check_batch(G, m, a, b, ao, bo)


def test_many_empty_segments(G):
    """2^20 segments, five of them non-empty with a few thousand keys."""
    S = 1 << 20
    rng = np.random.default_rng(5)
    la, lb = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    where = (0, 1000, 500000, 500001, S - 1)
    for s, (x, y) in zip(where, ((3000, 2000), (0, 4000), (2500, 2500), (4000, 0), (1234, 4321))):
        la[s], lb[s] = x, y
    ao, bo = offsets_of(la), offsets_of(lb)
    a, b = np.zeros(int(ao[-1]), dtype=np.uint32), np.zeros(int(bo[-1]), dtype=np.uint32)
    for i, s in enumerate(where):
        a[ao[s]:ao[s + 1]] = np.sort(rng.integers(0, 1000, la[s])) + (10 - i) * 1000
        b[bo[s]:bo[s + 1]] = np.sort(rng.integers(0, 1000, lb[s])) + (10 - i) * 1000
    m = G.Merge()
    check_batch(G, m, a, b, ao, bo)
    assert m.last() == (-(-(a.size + b.size) // tile_of(G, "uint32")), 2)


def test_ties(G):
    """Every key equal in A and in B, values iota: A first and each side in its order, segment by segment."""
    T = tile_of(G, "uint32")
    rng = np.random.default_rng(6)
    lens = rng.integers(0, T, 7)
    ao, bo = offsets_of(lens), offsets_of(lens[::-1])
    a, b = np.full(int(ao[-1]), 77, dtype=np.uint32), np.full(int(bo[-1]), 77, dtype=np.uint32)
    keys, vals, offs = check_batch(G, G.Merge(), a, b, ao, bo)
    for s in range(7):
        v = vals[offs[s]:offs[s + 1]]
        assert (v == np.concatenate([np.arange(ao[s], ao[s + 1]), np.arange(bo[s], bo[s + 1]) + B_VALS])).all()


@pytest.mark.parametrize("key_type", sorted(KEYS))
def test_every_key_type(G, key_type):
    """Five segments of up to a tile and a half a side with the type's specials on both sides of every segment: +-0.0, +-inf, NaNs of
    both signs; INT_MIN / INT_MAX; 0 / UINT_MAX.  The segments' key ranges are the same, so only the offsets keep them apart."""
    T = tile_of(G, key_type)
    rng = np.random.default_rng(len(key_type) + T)
    lens_a, lens_b = [T + T // 2, 40, 0, T // 3, 900], [100, T, 50, 0, 1000]
    a = np.concatenate([mg.typed_keys(rng, n, key_type) if n else np.zeros(0, dtype=key_type) for n in lens_a])
    b = np.concatenate([mg.typed_keys(rng, n, key_type) if n else np.zeros(0, dtype=key_type) for n in lens_b])
    m = G.Merge()
    check_batch(G, m, a, b, offsets_of(lens_a), offsets_of(lens_b))
    check_batch(G, m, a, b, offsets_of(lens_a), offsets_of(lens_b), with_vals=False)


def test_offsets_that_do_not_start_at_zero_and_totals_beyond_the_last_offset(G):
    """a_offsets[0] = 13 and b_offsets[0] = 6, 100 and 57 elements behind the last offsets: the outputs start at out[0], out_offsets are
    relative to the first offsets, and the poison behind oa[S] + ob[S] comes back intact (check_batch)."""
    rng = np.random.default_rng(8)
    T = tile_of(G, "uint32")
    lens_a, lens_b = [5, 0, T, 3, 0, 2 * T + 1], [0, 0, 17, T + 9, 1, 700]
    a, b, ao, bo = ragged(rng, np.uint32, lens_a, lens_b, front=(13, 6), slack=(100, 57))
    keys, _, offs = check_batch(G, G.Merge(), a, b, ao, bo)
    assert offs[0] == 0 and offs[-1] == keys.size == sum(lens_a) + sum(lens_b) < a.size + b.size - 150


@pytest.mark.parametrize("a_len,b_len,segments", [(3, 0, 500), (0, 5, 500), (7, 9, 1000), (4096, 4096, 3)])
def test_equal_partitions(G, a_len, b_len, segments):
    rng = np.random.default_rng(a_len + b_len)
    a, b, _, _ = ragged(rng, np.uint32, [a_len] * segments, [b_len] * segments, spread=1 << 12)
    m = G.Merge()
    check_batch(G, m, a, b, equal=(a_len, b_len, segments))
    check_batch(G, m, a, b, equal=(a_len, b_len, segments), with_vals=False, with_offsets=False)


def test_alignment(G):
    """Each of the six data arrays at every element shift off a 16-byte boundary, in turn and together, between poison bands; one
    tile inside a segment and tiles over several."""
    rng = np.random.default_rng(9)
    m = G.Merge()
    T = tile_of(G, "uint32")
    lens_a, lens_b = [T + 5, 3, 0, 40, T // 2], [11, T, 9, 0, T // 2]
    a, b, ao, bo = ragged(rng, np.uint32, lens_a, lens_b)
    want = check_batch(G, m, a, b, ao, bo)
    single = [tuple(s if i == j else 0 for j in range(6)) for i in range(6) for s in (4, 8, 12)]
    for shifts in single + [(4, 8, 12, 4, 8, 12), (12, 12, 12, 12, 12, 12), (4, 4, 8, 8, 12, 4)]:
        check_batch(G, m, a, b, ao, bo, shifts=shifts, want=want)
    check_batch(G, m, a, b, ao, bo, with_vals=False, shifts=(8, 0, 4, 0, 12, 0), want=want)
    T = tile_of(G, "uint64")
    lens_a, lens_b = [T + 3, 2, 0, T // 2], [7, T, 5, T // 2]
    a, b, ao, bo = ragged(rng, np.uint64, lens_a, lens_b)
    want = check_batch(G, m, a, b, ao, bo)
    for shifts in ((8, 0, 0, 0, 0, 0), (0, 0, 8, 0, 0, 0), (0, 0, 0, 0, 8, 0), (0, 4, 0, 8, 0, 12), (8, 4, 8, 12, 8, 4), (8, 8, 8, 8, 8, 8)):
        check_batch(G, m, a, b, ao, bo, shifts=shifts, want=want)


@pytest.mark.parametrize("key_type", ["uint32", "float64"])
def test_many_tiles_on_both_paths(G, key_type):
    """2^20 + 2^20 pairs in 37 ragged segments: several hundred tiles (last() against the plan), of which those that hold a segment
    boundary merge by (segment, key) and the others as the single merge does; the count of each is worked out from the offsets."""
    T = tile_of(G, key_type)
    rng = np.random.default_rng(10)
    n = 1 << 20

    def lens():
        cut = np.sort(rng.integers(0, n, 36))
        cut[10] = cut[9]  # (an empty segment)
        return np.diff(np.concatenate([[0], cut, [n]]))

    la, lb = lens(), lens()
    if key_type == "uint32":
        a, b, ao, bo = ragged(rng, np.uint32, la, lb, spread=1 << 24)
    else:
        ao, bo = offsets_of(la), offsets_of(lb)
        a = np.concatenate([np.sort(rng.standard_normal(k)) for k in la])
        b = np.concatenate([np.sort(rng.standard_normal(k)) for k in lb])
    m = G.Merge()
    _, _, offs = check_batch(G, m, a, b, ao, bo)
    tiles = -(-2 * n // T)
    assert m.last() == (tiles, 2) and tiles > 500
    inner = offs[1:-1].astype(np.int64)
    straddled = np.unique(inner[inner % T != 0] // T).size
    assert 20 <= straddled <= 36 and tiles - straddled > 400


def test_prepared_captured_replayed(G, monkeypatch):
    """After prepare_batch a call leaves the device's free memory as it found it, and one call captured on a side stream is replayed on
    other keys AND other offsets of the same capacity: another number of non-empty segments, another device total.  The object's
    scratch does not grow behind prepare_batch: under GLU_HIP_SCRATCH_FILL every growth moves glu_scratch_filled_bytes, and it stays."""
    import torch

    monkeypatch.setenv("GLU_HIP_SCRATCH_FILL", "0x5A")

    T = tile_of(G, "uint32")
    S, cap_a, cap_b = 50, 12 * T + 3, 9 * T + 1
    rng = np.random.default_rng(90)
    m = G.Merge()
    at, bt = torch.empty(cap_a, dtype=torch.int32, device="cuda"), torch.empty(cap_b, dtype=torch.int32, device="cuda")
    avt = torch.arange(cap_a, dtype=torch.int32, device="cuda")
    bvt = torch.from_numpy((np.arange(cap_b, dtype=np.uint32) + np.uint32(B_VALS)).view(np.int32)).cuda()
    aot, bot = torch.empty(S + 1, dtype=torch.int32, device="cuda"), torch.empty(S + 1, dtype=torch.int32, device="cuda")
    ok, ov = torch.empty(cap_a + cap_b, dtype=torch.int32, device="cuda"), torch.empty(cap_a + cap_b, dtype=torch.int32, device="cuda")
    oo = torch.empty(S + 1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def contents(used_a, used_b, empty_every):
        def lens(used):
            cut = np.sort(rng.integers(0, used, S - 1))
            l = np.diff(np.concatenate([[0], cut, [used]]))
            return l
        la, lb = lens(used_a), lens(used_b)
        if empty_every:
            keep = np.arange(S) % empty_every == 0
            la, lb = la * keep, lb * keep
        a, b, ao, bo = ragged(rng, np.uint32, la, lb, slack=(cap_a - int(la.sum()), cap_b - int(lb.sum())))
        return a, b, ao, bo

    def fill(a, b, ao, bo):
        at.copy_(torch.from_numpy(a.view(np.int32)))
        bt.copy_(torch.from_numpy(b.view(np.int32)))
        aot.copy_(torch.from_numpy(ao.astype(np.uint32).view(np.int32)))
        bot.copy_(torch.from_numpy(bo.astype(np.uint32).view(np.int32)))
        for t in (ok, ov, oo):
            t.fill_(-1515870811)

    def verify(a, b, ao, bo):
        keys, vals, offs = oracle(a, b, ao, bo)
        got_k, got_v = ok.cpu().numpy().view(np.uint32), ov.cpu().numpy().view(np.uint32)
        assert (got_k[:keys.size] == keys).all() and (got_v[:keys.size] == vals).all()
        assert (got_k[keys.size:] == 0xA5A5A5A5).all() and (got_v[keys.size:] == 0xA5A5A5A5).all()
        assert (oo.cpu().numpy().view(np.uint32) == offs).all()

    def call(s):
        m.run_batch_offsets_ptr(at.data_ptr(), avt.data_ptr(), aot.data_ptr(), cap_a, bt.data_ptr(), bvt.data_ptr(), bot.data_ptr(), cap_b, S,
                                ok.data_ptr(), ov.data_ptr(), oo.data_ptr(), "uint32", s)

    with torch.cuda.stream(side):
        data = contents(cap_a, cap_b, 0)
        fill(*data)
        side.synchronize()
        before = G.scratch_filled_bytes()
        m.prepare_batch(cap_a + cap_b, "uint32")
        filled = G.scratch_filled_bytes()
        assert filled - before >= G.plan_merge_batch(cap_a + cap_b, S)[3] > 0
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(*data)
        fill(*data)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        assert m.last() == (21 + 1, 2) == G.plan_merge_batch(cap_a + cap_b, S)[1:3]
        assert G.plan_merge_batch(cap_a + cap_b, S)[3] == (22 + 1) * 8
        verify(*data)
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        for used_a, used_b, empty_every in ((cap_a, cap_b, 0), (5 * T, 2 * T + 7, 3), (T // 2, 1, 7), (cap_a - 1, 3 * T, 2)):
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


def test_counts_that_live_on_the_device(G):
    """One segment whose two lengths are the num_out words of two set operations, copied into the offset words on the device: no host
    read between the three calls.  The merge of (A1 union A2) and (B1 intersection B2) against numpy."""
    import torch

    rng = np.random.default_rng(11)
    n = 5000
    a1, a2 = np.unique(rng.integers(0, 20000, n).astype(np.uint32)), np.unique(rng.integers(0, 20000, n).astype(np.uint32))
    b1, b2 = np.unique(rng.integers(0, 9000, n).astype(np.uint32)), np.unique(rng.integers(0, 9000, n).astype(np.uint32))
    want_a, want_b = np.union1d(a1, a2), np.intersect1d(b1, b2)
    cap_a, cap_b = a1.size + a2.size, min(b1.size, b2.size)
    dev = lambda x: torch.from_numpy(x.view(np.int32).copy()).cuda()  # noqa: E731
    ta1, ta2, tb1, tb2 = dev(a1), dev(a2), dev(b1), dev(b2)
    ua, ub = torch.full((cap_a,), -1, dtype=torch.int32, device="cuda"), torch.full((cap_b,), -1, dtype=torch.int32, device="cuda")
    aot, bot = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    ok = torch.full((cap_a + cap_b,), -1515870811, dtype=torch.int32, device="cuda")
    oo = torch.zeros(2, dtype=torch.int32, device="cuda")
    sets, m = G.SetOps(), G.Merge()
    s = stream()
    sets.run_ptr("union", ta1.data_ptr(), None, a1.size, ta2.data_ptr(), None, a2.size, ua.data_ptr(), None, cap_a, aot.data_ptr() + 4, "uint32", s)
    sets.run_ptr("intersection", tb1.data_ptr(), None, b1.size, tb2.data_ptr(), None, b2.size, ub.data_ptr(), None, cap_b, bot.data_ptr() + 4, "uint32", s)
    m.run_batch_offsets_ptr(ua.data_ptr(), None, aot.data_ptr(), cap_a, ub.data_ptr(), None, bot.data_ptr(), cap_b, 1, ok.data_ptr(), None,
                            oo.data_ptr(), "uint32", s)
    torch.cuda.synchronize()
    assert aot.cpu().numpy().tolist() == [0, want_a.size] and bot.cpu().numpy().tolist() == [0, want_b.size]
    total = want_a.size + want_b.size
    got = ok.cpu().numpy().view(np.uint32)
    assert (got[:total] == np.sort(np.concatenate([want_a, want_b]), kind="stable")).all() and (got[total:] == 0xA5A5A5A5).all()
    assert oo.cpu().numpy().tolist() == [0, total] and 0 < want_b.size and total < cap_a + cap_b


def test_with_the_family(G):
    """Batched sort of A's and of B's segments, batched merge, batched reduce (max) over out_offsets, all on one stream with no host
    read in between: the merged rows and every row's maximum against numpy."""
    import torch

    rng = np.random.default_rng(12)
    S = 200
    la, lb = rng.integers(0, 300, S), rng.integers(0, 300, S)
    la[5], lb[5], la[9], lb[9] = 0, 0, 7000, 9000
    ao, bo = offsets_of(la), offsets_of(lb)
    a, b = rng.integers(0, 1 << 20, int(ao[-1])).astype(np.uint32), rng.integers(0, 1 << 20, int(bo[-1])).astype(np.uint32)
    av, bv = np.arange(a.size, dtype=np.uint32), np.arange(b.size, dtype=np.uint32) + np.uint32(B_VALS)
    ak, ava, bk, bva = Array(a), Array(av), Array(b), Array(bv)
    aoa, boa = Array(ao.astype(np.uint32)), Array(bo.astype(np.uint32))
    ok, ov, oo = Array.poisoned(4 * (a.size + b.size)), Array.poisoned(4 * (a.size + b.size)), Array.poisoned(4 * (S + 1))
    top = Array.poisoned(4 * S)
    s = stream()
    sort, m, red = G.RadixSort(), G.Merge(), G.Reduce(G.DataType_Uint, G.ReduceOperator_Max)
    sort.sort_batch_offsets_ptr(ak.ptr, ava.ptr, a.size, aoa.ptr, S, "uint32", s)
    sort.sort_batch_offsets_ptr(bk.ptr, bva.ptr, b.size, boa.ptr, S, "uint32", s)
    m.run_batch_offsets_ptr(ak.ptr, ava.ptr, aoa.ptr, a.size, bk.ptr, bva.ptr, boa.ptr, b.size, S, ok.ptr, ov.ptr, oo.ptr, "uint32", s)
    red.run_batch_offsets_ptr(ok.ptr, top.ptr, a.size + b.size, oo.ptr, S, s)
    torch.cuda.synchronize()
    seg = np.concatenate([np.repeat(np.arange(S), la), np.repeat(np.arange(S), lb)])
    keys, vals = np.concatenate([a, b]), np.concatenate([av, bv])
    order = np.lexsort((vals, keys, seg))  # (the sorts are stable and A's values lie below B's)
    offs = (ao + bo).astype(np.uint32)
    assert (oo.result(np.uint32) == offs).all()
    assert (ok.result(np.uint32) == keys[order]).all() and (ov.result(np.uint32) == vals[order]).all()
    want_max = np.array([keys[order][offs[i]:offs[i + 1]].max() if offs[i + 1] > offs[i] else 0 for i in range(S)], dtype=np.uint32)
    assert (top.result(np.uint32) == want_max).all()


@pytest.mark.parametrize("prepared", [False, True], ids=["grows_in_the_call", "prepared"])
@pytest.mark.parametrize("kind", ["u32pairs", "u64keys"])
def test_scratch_fill(G, monkeypatch, kind, prepared):
    """Fresh objects under GLU_HIP_SCRATCH_FILL = 0x00, 0xFF and 0x5A (the method of test_gpu_scratch_fill.py): the boundaries are all
    written by the partition kernel before the tile kernel reads them, so every fill gives the oracle's bytes."""
    import test_gpu_scratch_fill as sf

    key_type, with_vals = ("uint32", True) if kind == "u32pairs" else ("uint64", False)
    T = tile_of(G, key_type)
    rng = np.random.default_rng(13)
    lens_a, lens_b = [T, 0, 5, 2 * T + 5, 40], [3, 0, T, T // 2, 0]
    a, b, ao, bo = ragged(rng, key_type, lens_a, lens_b)
    want = oracle(a, b, ao, bo)
    held = G.plan_merge_batch(a.size + b.size, 5, key_type, with_vals)[3]

    def case():
        m = G.Merge()
        if prepared:
            m.prepare_batch(a.size + b.size, key_type)
        check_batch(G, m, a, b, ao, bo, with_vals=with_vals, want=want)
        return held, {"last": m.last()}

    sf.under_every_fill(G, monkeypatch, case)


def test_argument_errors(G):
    """What the host can check: each INVALID_ARGUMENT with its own message, and a witness buffer shows that nothing was written."""
    import torch

    m = G.Merge()
    n, S = 4096, 8
    keys = np.arange(n, dtype=np.uint32)
    at, bt = torch.from_numpy(keys.view(np.int32).copy()).cuda(), torch.from_numpy(keys.view(np.int32).copy()).cuda()
    avt, bvt = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    offs = torch.from_numpy((np.arange(S + 1, dtype=np.uint32) * 8).view(np.int32).copy()).cuda()
    aot, bot = offs.clone(), offs.clone()
    wt = torch.zeros(8 * n, dtype=torch.int32, device="cuda")  # the witness: out_keys, out_vals, out_offsets
    ap, bp, avp, bvp, aop, bop, wp = (t.data_ptr() for t in (at, bt, avt, bvt, aot, bot, wt))
    okp, ovp, oop = wp, wp + 8 * n, wp + 16 * n
    L, vp = G.lib(), ctypes.c_void_p

    def run(a=ap, av=avp, ao=aop, na=64, b=bp, bv=bvp, bo=bop, nb=64, S=S, ok=okp, ov=ovp, oo=oop, key_type="uint32"):
        m.run_batch_offsets_ptr(a, av, ao, na, b, bv, bo, nb, S, ok, ov, oo, key_type)

    def equal(a=ap, av=avp, a_len=8, b=bp, bv=bvp, b_len=8, S=S, ok=okp, ov=ovp, oo=oop, key_type="uint32"):
        m.run_batch_ptr(a, av, a_len, b, bv, b_len, S, ok, ov, oo, key_type)

    bad = [
        (lambda: G.check(L.glu_merge_run_batch_offsets_ptr(None, vp(ap), vp(avp), vp(aop), 64, vp(bp), vp(bvp), vp(bop), 64, S, vp(okp), vp(ovp),
                                                           vp(oop), 0, None)), "merge is NULL"),
        (lambda: G.check(L.glu_merge_run_batch_ptr(None, vp(ap), vp(avp), 8, vp(bp), vp(bvp), 8, S, vp(okp), vp(ovp), vp(oop), 0, None)), "merge is NULL"),
        (lambda: G.check(L.glu_merge_prepare_batch(None, 64, 0)), "merge is NULL"),
        (lambda: run(av=None), "all NULL (keys only) or all non-NULL"),
        (lambda: run(bv=None), "all NULL (keys only) or all non-NULL"),
        (lambda: run(ov=None), "all NULL (keys only) or all non-NULL"),
        (lambda: equal(av=None, bv=None), "all NULL (keys only) or all non-NULL"),
        (lambda: run(a=None), "Invalid a_keys buffer"),
        (lambda: run(b=None), "Invalid b_keys buffer"),
        (lambda: equal(ok=None), "Invalid out_keys buffer"),
        (lambda: run(ao=None), "Invalid a_offsets array"),
        (lambda: run(bo=None), "Invalid b_offsets array"),
        (lambda: run(ao=aop + 2), "a_offsets is not aligned"),
        (lambda: run(bo=bop + 1), "b_offsets is not aligned"),
        (lambda: run(oo=oop + 2), "out_offsets is not aligned"),
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
        (lambda: G.check(L.glu_merge_run_batch_offsets_ptr(m._h, vp(ap), vp(avp), vp(aop), 64, vp(bp), vp(bvp), vp(bop), 64, S, vp(okp), vp(ovp),
                                                           vp(oop), 6, None)), "Invalid key type"),
        (lambda: G.check(L.glu_merge_prepare_batch(m._h, 64, 9)), "Invalid key type"),
        (lambda: run(S=(1 << 24) + 1), "exceeds 2^24"),
        (lambda: equal(S=(1 << 24) + 1, a_len=1, b_len=1), "exceeds 2^24"),
        (lambda: run(na=1 << 31, nb=1 << 31), "a_count + b_count below 2^32"),
        (lambda: equal(a_len=1 << 20, b_len=1 << 20, S=1 << 11), "a_count + b_count below 2^32"),
        (lambda: equal(a_len=1 << 32, b_len=0, S=1), "a_count + b_count below 2^32"),
        (lambda: m.prepare_batch(1 << 32), "a_count + b_count below 2^32"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, (i, e.value.message)
        assert message in e.value.message, (i, e.value.message)
    torch.cuda.synchronize()
    assert (wt.cpu().numpy() == 0).all(), "a refused call wrote something"
    assert (at.cpu().numpy().view(np.uint32) == keys).all() and (aot.cpu().numpy() == offs.cpu().numpy()).all()
    for good in (run, equal):  # (the same arguments, none changed, are a good call: every key of a segment twice)
        wt.zero_()
        good()
        torch.cuda.synchronize()
        got = wt.cpu().numpy().view(np.uint32)
        assert (got[:128] == np.repeat(np.arange(64), 2)).all()
        assert (got[4 * n:4 * n + S + 1] == np.arange(S + 1) * 16).all()


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_merge_batch_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout


@pytest.mark.parametrize("key_type", ["uint32", "uint64"])
def test_malformed_offsets_and_shuffled_keys_stay_inside_their_arrays(G, key_type):
    """The malformed cases of tests/test_merge_batch_path.py (which walks them on the host, under the sanitizers too), at most 10 000
    elements: the poison around every output is intact, the inputs and the offsets are unchanged, every out_offsets entry is at most
    a_total + b_total; the outputs' contents are unspecified and not looked at."""
    rng = np.random.default_rng(14)
    S = 40
    a, b, ao, bo = ragged(rng, key_type, rng.integers(0, 200, S), rng.integers(0, 200, S))
    assert a.size + b.size <= 10000 and a.size + b.size > tile_of(G, key_type)
    m = G.Merge()
    ones = np.full(S + 1, 0xFFFFFFFF, dtype=np.int64)
    for a_off, b_off in ((ao[::-1].copy(), bo), (ao[::-1].copy(), bo[::-1].copy()), (ao * 2 + 5, bo + b.size),
                         (np.where(np.arange(S + 1) > 20, ao + a.size, ao), bo), (ones, ones), (ones, bo),
                         (rng.integers(0, 1 << 32, S + 1), rng.integers(0, 1 << 32, S + 1)),
                         (rng.integers(0, a.size + 9, S + 1), rng.integers(0, b.size + 9, S + 1)),
                         (np.where(np.arange(S + 1) % 2, a.size, 0), np.sort(rng.integers(0, b.size, S + 1))),
                         (np.concatenate([[a.size + 3], ao[1:]]), bo)):
        check_batch(G, m, a, b, a_off, b_off, malformed=True)
    check_batch(G, m, rng.permutation(a), rng.permutation(b), ao, bo, malformed=True, shifts=(0, 4, 8, 12, 8, 4) if key_type == "uint32" else (8, 4, 0, 12, 8, 4))
    check_batch(G, m, rng.permutation(a), b[::-1].copy(), rng.integers(0, a.size + 9, S + 1), bo, malformed=True)
