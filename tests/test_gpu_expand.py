"""GPU tests of expand (glu_expand_run_ptr): from the offsets of segments to the segment, the rank and the segment's item of every
element.  The oracle is always numpy: s = searchsorted(offsets, arange(total), side="right") - 1, covered = (s >= 0) & (s < n).
Every comparison is `==`.  Every array the call writes sits inside an allocation with 64 bytes of poison in front of it and behind
it, and is itself filled with poison first, so positions that are not covered are seen to stay untouched; the inputs are checked
unchanged; last() is checked against plan_expand.  The scheme is that of test_gpu_merge.py."""
import ctypes
import gc
import itertools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # bytes of poison in front of and behind an array, inside its allocation
POISON = 0xA5


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


class Array:
    """The bytes of `d` on the device, `shift` bytes behind a 16-byte boundary, inside an allocation that holds poison in front of
    and behind them."""

    def __init__(self, d, shift=0):
        import torch

        d = np.ascontiguousarray(d)
        self.dtype, self.n, self.nbytes, self.front = d.dtype, d.size, d.nbytes, GUARD + shift
        self.host = np.concatenate([np.full(self.front, POISON, dtype=np.uint8), d.view(np.uint8).ravel(), np.full(GUARD, POISON, dtype=np.uint8)])
        self.t = torch.from_numpy(self.host.copy()).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.front

    @classmethod
    def poisoned(cls, nbytes, shift=0):
        return cls(np.full(nbytes, POISON, dtype=np.uint8), shift)

    def result(self, dtype=None):
        """The array after the call; asserts that the poison around it is intact."""
        raw = self.t.cpu().numpy()
        assert (raw[:self.front] == POISON).all() and (raw[self.front + self.nbytes:] == POISON).all(), "the call wrote outside the array"
        return raw[self.front:self.front + self.nbytes].copy().view(dtype or self.dtype)


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def tile_of(G):
    return G.plan_expand(1, 1)[0]


def offsets_of(lens, first=0):
    return (np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]) + first).astype(np.uint32)


def split_total(rng, total, n):
    """n segment lengths that sum to total"""
    return rng.multinomial(total, np.ones(n) / n)


def oracle(offsets, total):
    n = offsets.size - 1
    s = np.searchsorted(offsets, np.arange(total), side="right") - 1
    return s, (s >= 0) & (s < n)


def check_case(G, ex, offsets, total, item_bytes=4, outputs=("seg", "rank", "item"), shifts=(0, 0, 0, 0), malformed=False, seed=0):
    """One call.  offsets: n + 1 uint32.  outputs: which of the three are requested.  shifts: bytes behind a 16-byte boundary of
    out_segments, out_ranks, out_items, items.  Items are random bytes.  `malformed`: only the poison, the inputs, last() and
    out_segments < n where written are checked."""
    import torch

    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    n = offsets.size - 1
    items = np.random.default_rng(1000 + seed + n).integers(0, 256, (n, item_bytes), dtype=np.uint8)
    ob, ib = Array(offsets), Array(items, shifts[3])
    seg, rank, out = Array.poisoned(4 * total, shifts[0]), Array.poisoned(4 * total, shifts[1]), Array.poisoned(item_bytes * total, shifts[2])
    for arr, s in zip((seg, rank, out, ib), shifts):
        assert arr.ptr % 16 == s
    want_items = "item" in outputs
    ex.run_ptr(ob.ptr, n, total, seg.ptr if "seg" in outputs else None, rank.ptr if "rank" in outputs else None,
               ib.ptr if want_items else None, out.ptr if want_items else None, item_bytes, stream())
    torch.cuda.synchronize()
    what = (n, total, item_bytes, outputs, shifts, offsets[:3].tolist())
    assert ex.last() == (G.plan_expand(total, n)[1:3] if outputs and total and n else (0, 0)), (what, ex.last())
    got_seg, got_rank, got_items = seg.result(np.uint32), rank.result(np.uint32), out.result(np.uint8).reshape(total, item_bytes)
    assert (ob.result(np.uint32) == offsets).all(), "the call wrote to its offsets"
    assert (ib.result(np.uint8).reshape(n, item_bytes) == items).all(), "the call wrote to its items"
    for name, got in (("seg", got_seg), ("rank", got_rank), ("item", got_items)):
        if name not in outputs:
            assert (got.view(np.uint8) == POISON).all(), (what, name, "was not requested and was written")
    if malformed:
        if "seg" in outputs:
            written = got_seg != np.uint32(0xA5A5A5A5)
            assert (got_seg[written] < n).all(), (what, "a segment at or beyond n was written")
        return None
    s, covered = oracle(offsets, total)
    sc = s[covered]
    if "seg" in outputs:
        want = np.where(covered, s, 0xA5A5A5A5).astype(np.uint32)
        bad = np.flatnonzero(got_seg != want)
        assert bad.size == 0, (what, "segments", int(bad[0]), int(got_seg[bad[0]]), int(want[bad[0]]))
    if "rank" in outputs:
        want = np.full(total, 0xA5A5A5A5, dtype=np.uint32)
        want[covered] = (np.arange(total)[covered] - offsets[sc]).astype(np.uint32)
        bad = np.flatnonzero(got_rank != want)
        assert bad.size == 0, (what, "ranks", int(bad[0]), int(got_rank[bad[0]]), int(want[bad[0]]))
    if want_items:
        want = np.full((total, item_bytes), POISON, dtype=np.uint8)
        want[covered] = items[sc]
        bad = np.flatnonzero((got_items != want).any(axis=1))
        assert bad.size == 0, (what, "items", int(bad[0]))
    return s, covered


def test_tiny(G):
    rng = np.random.default_rng(1)
    ex = G.Expand()
    for total in (1, 2, 63, 64, 65):
        for n in sorted({1, 2, total}):
            check_case(G, ex, offsets_of(split_total(rng, total, n)), total)
    assert G.plan_expand(1, 1)[1:3] == (1, 2)


@pytest.mark.parametrize("mean", [1, 3, 1000])
def test_tile_boundaries(G, mean):
    T = tile_of(G)
    rng = np.random.default_rng(mean)
    ex = G.Expand()
    for M in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 1):
        n = max(1, (M - 1) // (mean + 1))
        total = M - n - 1
        assert G.plan_expand(total, n)[1] == -(-M // T)
        check_case(G, ex, offsets_of(split_total(rng, total, n)), total)
    assert ex.last() == (4, 2)


def test_one_segment_and_every_segment_of_length_one(G):
    T = tile_of(G)
    ex = G.Expand()
    total = 3 * T + 7
    s, covered = check_case(G, ex, np.array([0, total]), total)
    assert covered.all() and (s == 0).all()
    s, covered = check_case(G, ex, np.arange(total + 1), total)
    assert covered.all() and (s == np.arange(total)).all()


@pytest.mark.parametrize("run", ["1", "T-1", "T", "T+1", "3T+5"])
def test_empty_segments(G, run):
    """Runs of equal offsets in front, behind and in the middle; the interior run starts exactly on a tile boundary of the merged
    sequence (T - 2 positions and the two offsets around them fill the first tile), so with the longer runs whole tiles write
    nothing."""
    T = tile_of(G)
    run = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[run]
    ex = G.Expand()
    check_case(G, ex, offsets_of([0] * run + [5, 9]), 14)
    check_case(G, ex, offsets_of([5, 9] + [0] * run), 14)
    s, covered = check_case(G, ex, offsets_of([T - 2] + [0] * run + [T + 3]), 2 * T + 1)
    assert covered.all() and set(np.unique(s)) == {0, run + 1}
    check_case(G, ex, offsets_of([0] * run + [T + 1] + [0] * run + [40] + [0] * run), T + 41, item_bytes=8)


def test_key_runs_form(G):
    """Offsets written by key runs with max_runs far above the number of runs: the tail holds `count`, many trailing empty segments
    at total.  Decoding the unique keys gives the keys back."""
    import torch

    T = tile_of(G)
    rng = np.random.default_rng(5)
    count, max_runs = 3 * T + 11, 5 * T
    keys = np.sort(rng.integers(0, 200, count).astype(np.uint32) * np.uint32(7919))
    kb = Array(keys)
    fb, ub, nb = Array.poisoned(4 * (max_runs + 1)), Array.poisoned(4 * max_runs), Array.poisoned(4)
    G.KeyRuns().run_ptr(kb.ptr, count, fb.ptr, max_runs, nb.ptr, unique_keys_ptr=ub.ptr, stream=stream())
    torch.cuda.synchronize()
    offsets = fb.result(np.uint32)
    R = int(nb.result(np.uint32)[0])
    assert R == np.unique(keys).size and (offsets[R:] == count).all()
    ex = G.Expand()
    s, covered = check_case(G, ex, offsets, count)
    assert covered.all() and s.max() == R - 1
    out = Array.poisoned(4 * count)
    ex.run_ptr(fb.ptr, max_runs, count, items_ptr=ub.ptr, out_items_ptr=out.ptr, item_bytes=4, stream=stream())
    torch.cuda.synchronize()
    assert (out.result(np.uint32) == keys).all()


def test_partial_cover(G):
    T = tile_of(G)
    ex = G.Expand()
    # offsets[0] > 0 and offsets[n] < total: head and tail keep their poison
    s, covered = check_case(G, ex, offsets_of([4, 0, T, 7], first=5), T + 40)
    assert not covered[:5].any() and not covered[T + 16:].any() and covered[5:T + 16].all()
    # offsets[n] > total: nothing at or behind total (the poison behind the arrays), the positions below it as the oracle
    s, covered = check_case(G, ex, offsets_of([4, 0, T, 700], first=5), T + 40)
    assert covered[5:].all()
    check_case(G, ex, offsets_of([T, 2 * T, 3 * T]), 2 * T + 3, item_bytes=32)
    s, covered = check_case(G, ex, offsets_of([1, 2, 3], first=2 * T), T)  # nothing covered
    assert not covered.any()


def test_alignment(G):
    """Output arrays 4, 8 and 12 bytes behind a 16-byte boundary, independently per output; items shifted by their alignment."""
    T = tile_of(G)
    rng = np.random.default_rng(8)
    ex = G.Expand()
    total, n = 2 * T + 5, 300
    offsets = offsets_of(split_total(rng, total - 9, n), first=3)
    for shifts in ((4, 0, 0, 0), (0, 8, 0, 0), (0, 0, 12, 0), (0, 0, 0, 4), (4, 8, 12, 8), (12, 4, 8, 12), (8, 12, 4, 4), (12, 12, 12, 12)):
        check_case(G, ex, offsets, total, 4, shifts=shifts)
    for shifts in ((4, 12, 8, 0), (0, 0, 8, 8), (8, 4, 0, 8)):
        check_case(G, ex, offsets, total, 8, shifts=shifts)
    for item_bytes in (16, 32):
        check_case(G, ex, offsets, total, item_bytes, shifts=(4, 12, 0, 0))


@pytest.mark.parametrize("item_bytes", [4, 8, 16, 32])
def test_item_sizes_and_every_subset_of_outputs(G, item_bytes):
    T = tile_of(G)
    rng = np.random.default_rng(item_bytes)
    ex = G.Expand()
    n = 97
    total = 2 * T - n - 1 - 13  # two tiles of the merged sequence, the second not full
    offsets = offsets_of(split_total(rng, total - 6, n), first=2)
    assert G.plan_expand(total, n)[1] == 2
    for k in (1, 2, 3):
        for outputs in itertools.combinations(("seg", "rank", "item"), k):
            check_case(G, ex, offsets, total, item_bytes, outputs=outputs)
    check_case(G, ex, offsets, total, item_bytes, outputs=())  # nothing asked for: nothing enqueued
    assert ex.last() == (0, 0)


def test_many_tiles(G):
    rng = np.random.default_rng(9)
    ex = G.Expand()
    total = 2 ** 22 + 321
    lens = rng.geometric(1 / 38.0, total // 30) - 1  # geometric lengths from 0 on, mean 37
    lens = lens[np.cumsum(lens) <= total]
    check_case(G, ex, offsets_of(lens), total)
    assert ex.last()[0] > 256  # the partition kernel's second workgroup
    total = 2 ** 22
    check_case(G, ex, np.array([0, 5, 2 ** 20, 2 ** 20, 2 ** 22 - 3, 2 ** 22]), total, item_bytes=16)


def test_prepared_captured_replayed(G):
    """After prepare a call leaves the device's free memory as it found it, and one call captured on a side stream is replayed on
    three offset contents of the same n and total: the launch sequence does not depend on the data."""
    import torch

    T = tile_of(G)
    total, n = 20 * T + 3, 7 * T + 1
    rng = np.random.default_rng(90)
    ex = G.Expand()
    ot = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    items = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    it = torch.from_numpy(items.view(np.int32)).cuda()
    seg, rank, out = (torch.empty(total, dtype=torch.int32, device="cuda") for _ in range(3))
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def fill(offsets):
        ot.copy_(torch.from_numpy(offsets.view(np.int32)))
        for t in (seg, rank, out):
            t.fill_(-1515870811)

    def verify(offsets):
        s, covered = oracle(offsets, total)
        sc = s[covered]
        poison = np.full(total, 0xA5A5A5A5, dtype=np.uint32)
        want_seg, want_rank, want_out = poison.copy(), poison.copy(), poison.copy()
        want_seg[covered], want_rank[covered], want_out[covered] = sc, np.arange(total)[covered] - offsets[sc], items[sc]
        assert (seg.cpu().numpy().view(np.uint32) == want_seg).all()
        assert (rank.cpu().numpy().view(np.uint32) == want_rank).all()
        assert (out.cpu().numpy().view(np.uint32) == want_out).all()

    def call(s):
        ex.run_ptr(ot.data_ptr(), n, total, seg.data_ptr(), rank.data_ptr(), it.data_ptr(), out.data_ptr(), 4, s)

    one_long = np.zeros(n, dtype=np.int64)
    one_long[n // 2] = total - 1000
    contents = [offsets_of(split_total(rng, total, n)),  # everything covered, short segments
                offsets_of(one_long, first=7),  # one segment among empty ones
                offsets_of(rng.geometric(0.5, n) - 1, first=T)]  # a partial cover, half the segments empty
    with torch.cuda.stream(side):
        fill(contents[0])
        side.synchronize()
        ex.prepare(total, n)
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(contents[0])
        fill(contents[0])
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        assert ex.last() == G.plan_expand(total, n)[1:3] == (28, 2)
        verify(contents[0])
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        for offsets in contents[::-1]:
            fill(offsets)
            graph.replay()
            side.synchronize()
            verify(offsets)


def test_malformed_offsets_stay_inside_the_arrays(G):
    """Shuffled offsets, offsets beyond total and a decreasing pair (tests/test_expand_path.py runs the same kinds through the
    header's arithmetic on the host and finds every index inside its bound): the poison around the outputs is intact, the inputs
    are unchanged, every segment written is below n.  The contents are otherwise unspecified and not looked at."""
    T = tile_of(G)
    rng = np.random.default_rng(13)
    ex = G.Expand()
    base = offsets_of(split_total(rng, 3 * T, 500))
    total = int(base[-1])
    beyond = base.copy()
    beyond[base.size // 2:] += np.uint32(2 * T)
    far = base.copy()
    far[3], far[-1] = 0xFFFFFFFF, 0xFFFFFFF0
    pair = base.copy()
    pair[[10, 11]] = pair[[11, 10]] + np.uint32([7, 0])
    for offsets in (rng.permutation(base), beyond, far, pair, base[::-1].copy()):
        check_case(G, ex, offsets, total, item_bytes=8, shifts=(4, 8, 8, 8), malformed=True)


def test_argument_errors(G):
    """Every refusal of the contract: INVALID_ARGUMENT with a message that names the argument, and a witness buffer (every output
    lies in it) shows that nothing was written."""
    import torch

    ex = G.Expand()
    n, total = 64, 1024
    offsets = offsets_of(np.full(n, total // n))
    far = 4 * total  # words between the offsets and the items: an output laid over one of them does not reach the other
    inputs = np.zeros(4 * far, dtype=np.uint32)  # (room behind the items too: the refused outputs stay inside this allocation)
    inputs[far:far + n + 1] = offsets
    ot = torch.from_numpy(inputs.view(np.int32).copy()).cuda()
    wt = torch.zeros(16 * total, dtype=torch.int32, device="cuda")  # the witness: out_segments, out_ranks, out_items
    op, ip, wp = ot.data_ptr() + 4 * far, ot.data_ptr() + 8 * far, wt.data_ptr()
    sp, rp, xp = wp, wp + 4 * total, wp + 8 * total
    L, vp = G.lib(), ctypes.c_void_p

    def run(o=op, n_=n, total_=total, seg=sp, rank=rp, items=ip, out=xp, item_bytes=4):
        ex.run_ptr(o, n_, total_, seg, rank, items, out, item_bytes)

    bad = [
        (lambda: G.check(L.glu_expand_run_ptr(None, vp(op), n, total, vp(ip), 4, vp(xp), vp(sp), vp(rp), None)), "expand is NULL"),
        (lambda: G.check(L.glu_expand_prepare(None, 64, 64)), "expand is NULL"),
        (lambda: G.check(L.glu_expand_last(None, None, None)), "expand is NULL"),
        (lambda: G.check(L.glu_expand_create(None)), "out is NULL"),
        (lambda: run(o=None), "offsets"),
        (lambda: run(items=None), "items and out_items"),
        (lambda: run(out=None), "items and out_items"),
        (lambda: run(item_bytes=0), "item_bytes"),
        (lambda: run(item_bytes=12), "item_bytes"),
        (lambda: run(item_bytes=64), "item_bytes"),
        (lambda: run(o=op + 2), "offsets is not aligned"),
        (lambda: run(seg=sp + 1), "out_segments is not aligned"),
        (lambda: run(rank=rp + 2), "out_ranks is not aligned"),
        (lambda: run(items=ip + 2), "items is not aligned"),
        (lambda: run(out=xp + 4, item_bytes=8), "out_items is not aligned"),
        (lambda: run(items=ip + 8, item_bytes=32), "items is not aligned"),
        (lambda: run(out=xp + 8, item_bytes=16), "out_items is not aligned"),
        (lambda: run(n_=2 ** 24 + 1), "num_segments"),
        (lambda: run(total_=2 ** 32), "total"),
        (lambda: run(total_=2 ** 32 - 1 - n), "total + num_segments + 1"),
        (lambda: ex.prepare(2 ** 32, 1), "total"),
        (lambda: ex.prepare(10, 2 ** 24 + 1), "num_segments"),
        (lambda: run(seg=op), "out_segments overlaps offsets"),
        (lambda: run(seg=op + 4 * n), "out_segments overlaps offsets"),
        (lambda: run(seg=ip), "out_segments overlaps items"),
        (lambda: run(rank=op - 4 * (total - 1)), "out_ranks overlaps offsets"),
        (lambda: run(rank=ip + 4 * (n - 1)), "out_ranks overlaps items"),
        (lambda: run(out=op), "out_items overlaps offsets"),
        (lambda: run(out=ip), "out_items overlaps items"),
        (lambda: run(rank=sp + 4 * (total - 1)), "out_segments overlaps out_ranks"),
        (lambda: run(out=sp + 4 * (total - 1)), "out_segments overlaps out_items"),
        (lambda: run(out=rp, rank=rp), "out_ranks overlaps out_items"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, (i, e.value.message)
        assert message in e.value.message, (i, e.value.message)
    torch.cuda.synchronize()
    assert (wt.cpu().numpy() == 0).all(), "a refused call wrote something"
    assert (ot.cpu().numpy().view(np.uint32) == inputs).all()
    # nothing to do: GLU_OK whatever the arrays are
    ex.run_ptr(None, 0, total, None, None, None, None, 4)
    ex.run_ptr(None, n, 0, None, None, None, None, 4)
    assert ex.last() == (0, 0)
    # arrays that only touch are fine: the offsets, then out_segments right behind them, then out_ranks
    big = torch.from_numpy(np.concatenate([offsets, np.zeros(2 * total, dtype=np.uint32)]).view(np.int32).copy()).cuda()
    bp = big.data_ptr()
    ex.run_ptr(bp, n, total, bp + 4 * (n + 1), bp + 4 * (n + 1 + total), stream=stream())
    torch.cuda.synchronize()
    got = big.cpu().numpy().view(np.uint32)
    assert (got[:n + 1] == offsets).all()
    assert (got[n + 1:n + 1 + total] == np.arange(total) // (total // n)).all()
    assert (got[n + 1 + total:] == np.arange(total) % (total // n)).all()


def test_with_the_family(G):
    """Sort pairs, key runs, a batched sum per group, then expand: every element gets its group's sum and its index inside the
    group.  And a join: sorted search's ranges become counts, a batched scan of one segment turns them into offsets, and expand's
    (segment, lower[segment] + rank) pairs are numpy's join."""
    import torch

    rng = np.random.default_rng(70)
    count, max_runs = 70001, 4096
    keys = rng.integers(0, 900, count).astype(np.uint32) * np.uint32(7919)
    vals = rng.integers(0, 1000, count, dtype=np.uint32)
    kb, vb = Array(keys), Array(vals)
    fb, nb, sums = Array.poisoned(4 * (max_runs + 1)), Array.poisoned(4), Array.poisoned(4 * max_runs)
    out, rank = Array.poisoned(4 * count), Array.poisoned(4 * count)
    s = stream()
    ex = G.Expand()
    G.RadixSort().sort_typed_ptr(kb.ptr, vb.ptr, count, "uint32", s)
    G.KeyRuns().run_ptr(kb.ptr, count, fb.ptr, max_runs, nb.ptr, stream=s)
    G.Reduce(G.DataType_Uint, G.ReduceOperator_Sum).run_batch_offsets_ptr(vb.ptr, sums.ptr, count, fb.ptr, max_runs, s)
    ex.run_ptr(fb.ptr, max_runs, count, None, rank.ptr, sums.ptr, out.ptr, 4, s)
    torch.cuda.synchronize()
    order = np.argsort(keys, kind="stable")
    sk, sv = keys[order], vals[order]
    assert (kb.result(np.uint32) == sk).all() and (vb.result(np.uint32) == sv).all()
    group = np.cumsum(np.concatenate([[0], sk[1:] != sk[:-1]]))
    group_sum = np.bincount(group, weights=sv).astype(np.uint64).astype(np.uint32)
    heads = np.flatnonzero(np.concatenate([[1], sk[1:] != sk[:-1]]))
    assert (out.result(np.uint32) == group_sum[group]).all(), "the broadcast of the group sums differs from numpy"
    assert (rank.result(np.uint32) == np.arange(count) - heads[group]).all(), "the index inside the group differs from numpy"

    # the join of `needles` with the sorted keys
    m = 3001
    needles = rng.integers(0, 1000, m).astype(np.uint32) * np.uint32(7919)
    lo, hi = np.searchsorted(sk, needles, "left"), np.searchsorted(sk, needles, "right")
    pairs = int((hi - lo).sum())
    eb, lb, ub = Array(needles), Array.poisoned(4 * m), Array.poisoned(4 * m)
    G.SortedSearch().run_ptr(kb.ptr, count, eb.ptr, m, lb.ptr, ub.ptr, "uint32", stream=s)
    torch.cuda.synchronize()
    lower = torch.from_numpy(lb.result(np.uint32).view(np.int32)).cuda()
    upper = torch.from_numpy(ub.result(np.uint32).view(np.int32)).cuda()
    counts = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    counts[:m] = upper - lower
    one = torch.tensor([0, m + 1], dtype=torch.int32, device="cuda")
    G.BlellochScan(G.DataType_Uint).run_batch_offsets_ptr(counts.data_ptr(), m + 1, one.data_ptr(), 1, s)  # counts -> offsets, in place
    seg, rk = Array.poisoned(4 * pairs), Array.poisoned(4 * pairs)
    ex.run_ptr(counts.data_ptr(), m, pairs, seg.ptr, rk.ptr, stream=s)
    torch.cuda.synchronize()
    assert int(counts[m].item()) == pairs and 0 < pairs
    want_needle = np.repeat(np.arange(m), hi - lo)
    want_match = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)])
    got_needle = seg.result(np.uint32)
    assert (got_needle == want_needle).all()
    assert (lb.result(np.uint32)[got_needle] + rk.result(np.uint32) == want_match).all()
    assert (sk[want_match] == needles[want_needle]).all()


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_expand_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
