"""GPU tests of the batched reduce (glu_reduce_run_batch_ptr / glu_reduce_run_batch_offsets_ptr): out[s] = the reduction of
segment s, every segment on its own, the input only read.  Expected results come from numpy: oracle.reduce_expected /
oracle.dtype_info applied to every segment's slice, the operator's identity for an empty one.  Inputs are built the way
test_reduce_every_type_and_operator builds them (float sums that are exact in any order, products of mostly ones), so `==` is the
check for every type; the floats that do round have a test of their own against math.fsum."""
import math
import os
import subprocess

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4  # elements in front of and behind `out` that must keep their pattern
GUARD_BYTE = 0xA5


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def identity(npdt, op):
    if op == 0:
        return npdt(0)
    if op == 1:
        return npdt(1)
    if np.issubdtype(npdt, np.floating):
        return npdt(np.inf) if op == 2 else npdt(-np.inf)
    return npdt(np.iinfo(npdt).max) if op == 2 else npdt(np.iinfo(npdt).min)


def make_data(rng, n, dt, op):
    """n elements (n * components scalars), as in test_reduce_every_type_and_operator."""
    npdt, comps = O.dtype_info(dt)
    if op == 1:  # products: mostly ones so nothing overflows / underflows
        d = np.ones(n * comps, dtype=npdt)
        if n:
            d[rng.integers(0, n * comps, 4)] = 2
            if np.issubdtype(npdt, np.signedinteger) or np.issubdtype(npdt, np.floating):
                d[rng.integers(0, n * comps, 3)] = -1
        return d
    if np.issubdtype(npdt, np.floating):
        return (rng.integers(-4000, 4000, n * comps) * 0.125).astype(npdt)  # exact sums
    if npdt == np.int32:
        return rng.integers(-2**31, 2**31, n * comps).astype(npdt)
    return rng.integers(0, 2**32, n * comps, dtype=np.uint32)


def expected_segments(d, dt, op, offsets, total=None):
    """[num_segments, components]: oracle.reduce_expected of every well-formed, non-empty segment's slice, the identity for the
    others (empty ones, and with `total` given those whose end lies below their begin or beyond total)."""
    npdt, comps = O.dtype_info(dt)
    rows = d.reshape(-1, comps)
    offsets = np.asarray(offsets, dtype=np.int64)
    out = np.empty((offsets.size - 1, comps), dtype=npdt)
    for s, (b, e) in enumerate(zip(offsets[:-1], offsets[1:])):
        if e <= b or (total is not None and e > total):
            out[s] = identity(npdt, op)
            continue
        seg = rows[b:e]
        if op == 1 and np.issubdtype(npdt, np.integer):
            seg = seg[(seg != 1).any(axis=1)]  # rows of ones are the identity of a product: the oracle multiplies row by row
            if seg.shape[0] == 0:
                out[s] = 1
                continue
        out[s] = np.asarray(O.reduce_expected(seg.reshape(-1), dt, op)).astype(npdt)
    return out


class Arrays:
    """`data` (optionally shifted by `shift` elements from the allocation's start, with poison in front and behind) and a guarded
    `out` on the device."""

    def __init__(self, d, dt, num_segments, shift=0, poison=None):
        import torch

        npdt, comps = O.dtype_info(dt)
        self.npdt, self.comps, self.es = npdt, comps, npdt().itemsize * comps
        self.nseg = num_segments
        pad = np.full(shift * comps, 0 if poison is None else poison, dtype=npdt)
        tail = np.full(8 * comps, 0 if poison is None else poison, dtype=npdt)
        self.host = np.concatenate([pad, d, tail])
        self.shift = shift
        self.n = d.size // comps
        self.data_t = torch.from_numpy(self.host.view(np.uint8).copy()).cuda()
        self.out_t = torch.full(((num_segments + 2 * GUARD) * self.es,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.data_ptr = self.data_t.data_ptr() + shift * self.es
        self.out_ptr = self.out_t.data_ptr() + GUARD * self.es

    def reset_out(self):
        self.out_t.fill_(GUARD_BYTE)

    def result(self):
        """out as [num_segments, components]; asserts that the guards around it and the whole data allocation are unchanged."""
        raw = self.out_t.cpu().numpy()
        g = GUARD * self.es
        assert (raw[:g] == GUARD_BYTE).all() and (raw[raw.size - g:] == GUARD_BYTE).all(), "out was written outside its segments"
        assert (self.data_t.cpu().numpy() == self.host.view(np.uint8)).all(), "data was written"
        return raw[g:raw.size - g].copy().view(self.npdt).reshape(self.nseg, self.comps)


def device_offsets(offsets):
    import torch

    return torch.from_numpy(np.asarray(offsets, dtype=np.uint32).view(np.int32).copy()).cuda()


def sync_stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def run_offsets(G, red, d, dt, offsets, shift=0, total=None, poison=None):
    import torch

    arr = Arrays(d, dt, len(offsets) - 1, shift, poison)
    ot = device_offsets(offsets)
    red.run_batch_offsets_ptr(arr.data_ptr, arr.out_ptr, arr.n if total is None else total, ot.data_ptr(), len(offsets) - 1, sync_stream())
    torch.cuda.synchronize()
    return arr.result()


def run_equal(G, red, d, dt, count, parts, shift=0):
    import torch

    arr = Arrays(d, dt, parts, shift)
    red.run_batch_ptr(arr.data_ptr, arr.out_ptr, count, parts, sync_stream())
    torch.cuda.synchronize()
    return arr.result()


def class_limits(G, es):
    """Last length of the wave class and last length of the workgroup class, found from plan_reduce_batch alone."""
    def last_of(path):
        lo, hi = 0, 1 << 40  # plan(lo).path <= path < plan(hi).path
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if G.plan_reduce_batch(mid, es)[0] <= path:
                lo = mid
            else:
                hi = mid
        return lo
    return last_of(1), last_of(2)


def boundary_lengths(G, es):
    wave, block = class_limits(G, es)
    assert G.plan_reduce_batch(wave, es)[0] == 1 and G.plan_reduce_batch(wave + 1, es)[0] == 2
    assert G.plan_reduce_batch(block, es)[0] == 2 and G.plan_reduce_batch(block + 1, es)[0] == 3
    lens = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65]
    for b in (wave, block):  # (the last length of a class and the first of the next: both readings of "boundary", each +- 1)
        lens += [b - 1, b, b + 1, b + 2]
    two = next(c for c in range(block + 1, 4 * block + 4) if G.plan_reduce_batch(c, es)[1] == 3) - 1  # last length on two workgroups
    lens += [two - 1, two, two + 1]
    return lens


@pytest.mark.parametrize("dt", range(12))
@pytest.mark.parametrize("op", range(4))
def test_every_type_and_operator_across_the_class_boundaries(G, dt, op):
    npdt, comps = O.dtype_info(dt)
    es = npdt().itemsize * comps
    rng = np.random.default_rng(100 + dt * 4 + op)
    lens = boundary_lengths(G, es)
    order = rng.permutation(len(lens))
    lens = [lens[i] for i in order]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = make_data(rng, int(offsets[-1]), dt, op)
    red = G.Reduce(dt, op)
    got = run_offsets(G, red, d, dt, offsets)
    want = expected_segments(d, dt, op, offsets)
    assert (got == want).all(), (dt, op, [lens[s] for s in np.nonzero((got != want).any(axis=1))[0]])
    rb = red.read_batch()
    paths = [G.plan_reduce_batch(n, es)[0] for n in lens]
    assert [rb["wave"], rb["block"], rb["long"]] == [paths.count(p) for p in (1, 2, 3)]
    # the same lengths as equal partitions, three of each
    for n in sorted(set(lens)):
        parts = 3
        dd = d[:n * parts * comps]
        got = run_equal(G, red, dd, dt, n, parts)
        want = expected_segments(dd, dt, op, np.arange(parts + 1) * n)
        assert (got == want).all(), (dt, op, n, got, want)
        path = G.plan_reduce_batch(n, es)[0]
        rb = red.read_batch()
        assert [rb["wave"], rb["block"], rb["long"]] == [parts if path == p else 0 for p in (1, 2, 3)]


def mixed_lengths(rng, es, extra=()):
    """Zeros, ones, geometric around 40, uniform up to 3000, a few workgroup-sized and long ones, shuffled."""
    lens = np.concatenate([np.zeros(20, np.int64), np.ones(20, np.int64), rng.geometric(1 / 40.0, 600), rng.integers(0, 3001, 120),
                           np.asarray([20000 // es * 4, 262144 // es, 262144 // es + 1, 1000000 // es * 4, 3 * 262144 // es + 7], dtype=np.int64),
                           np.asarray(extra, dtype=np.int64)])
    rng.shuffle(lens)
    return lens


@pytest.mark.parametrize("dt,op", [(3, 0), (0, 2), (7, 0), (10, 3), (1, 1)])
def test_offsets_with_empty_and_single_segments_anywhere(G, dt, op):
    """Empty segments at the start, in the middle and at the end, one-element segments, offsets that neither start at 0 nor end at
    `total`, on an array whose base is one element off its allocation: identities, results, read_batch."""
    npdt, comps = O.dtype_info(dt)
    es = npdt().itemsize * comps
    rng = np.random.default_rng(200 + dt * 4 + op)
    lens = np.concatenate([[0, 0, 1], mixed_lengths(rng, es), [1, 0, 0]])
    mid = lens.size // 2
    lens[mid:mid + 3] = [0, 1, 0]
    head, tail = 777, 1234
    offsets = np.concatenate([[0], np.cumsum(lens)]) + head
    total = int(offsets[-1]) + tail
    d = make_data(rng, total, dt, op)
    red = G.Reduce(dt, op)
    got = run_offsets(G, red, d, dt, offsets, shift=1)
    want = expected_segments(d, dt, op, offsets)
    assert (got == want).all()
    for s in (0, 1, mid, mid + 2, lens.size - 2, lens.size - 1):
        assert (got[s] == identity(npdt, op)).all()
    rb = red.read_batch()
    assert rb["wave"] > 0 and rb["block"] > 0 and rb["long"] > 0
    paths = [G.plan_reduce_batch(int(n), es)[0] for n in lens]
    assert [rb["wave"], rb["block"], rb["long"]] == [paths.count(p) for p in (1, 2, 3)]


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_bases(G, shift):
    """uint32 arrays that start 4, 8 and 12 bytes behind a 16-byte boundary, through both entry points."""
    dt, op = 3, 0
    rng = np.random.default_rng(300 + shift)
    lens = mixed_lengths(rng, 4)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = make_data(rng, int(offsets[-1]), dt, op)
    red = G.Reduce(dt, op)
    assert (run_offsets(G, red, d, dt, offsets, shift=shift) == expected_segments(d, dt, op, offsets)).all()
    for count in (5, 33, 1025, 70001):
        parts = 7
        dd = d[:count * parts]
        assert (run_equal(G, red, dd, dt, count, parts, shift=shift) == expected_segments(dd, dt, op, np.arange(parts + 1) * count)).all()


def test_a_million_tiny_segments(G):
    """2^20 segments of 0 .. 8 elements: binning and list walking at scale."""
    dt, op = 3, 0
    rng = np.random.default_rng(13)
    lens = rng.integers(0, 9, 1 << 20)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = make_data(rng, int(offsets[-1]), dt, op)
    red = G.Reduce(dt, op)
    got = run_offsets(G, red, d, dt, offsets)
    want = np.add.reduceat(np.concatenate([d, [0]]).astype(np.uint64), offsets[:-1]) & 0xFFFFFFFF  # (numpy: sums of the slices)
    want[lens == 0] = 0
    assert (got[:, 0] == want.astype(np.uint32)).all()
    assert red.read_batch() == {"wave": int((lens > 0).sum()), "block": 0, "long": 0}


@pytest.mark.parametrize("dt", [0, 1])
def test_float_sums_that_round(G, dt):
    """float32 / float64 Sum over random normal data, one segment per class, both entry points: within n * eps * sum|x| of the
    exact sum (math.fsum) -- twice the standard worst-case bound (n - 1) * eps / 2 * sum|x| * (1 + O(n eps)) of summation in any
    order -- and bit for bit the same when the same call runs again."""
    import torch

    npdt, _ = O.dtype_info(dt)
    es = npdt().itemsize
    wave, block = class_limits(G, es)
    lens = [wave - 3, block - 5, 3 * block + 11]
    assert [G.plan_reduce_batch(n, es)[0] for n in lens] == [1, 2, 3]
    rng = np.random.default_rng(400 + dt)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = rng.standard_normal(int(offsets[-1])).astype(npdt)
    eps = float(np.finfo(npdt).eps)
    red = G.Reduce(dt, 0)

    def check(got, slices):
        for value, x in zip(got, slices):
            exact = math.fsum(x.astype(np.float64).tolist())
            bound = x.size * eps * math.fsum(np.abs(x).astype(np.float64).tolist())
            print("n = %d: |got - exact| = %.3e, bound %.3e" % (x.size, abs(float(value) - exact), bound))
            assert abs(float(value) - exact) <= bound, (x.size, float(value), exact, bound)

    arr = Arrays(d, dt, len(lens))
    ot = device_offsets(offsets)
    runs = []
    for _ in range(2):
        arr.reset_out()
        red.run_batch_offsets_ptr(arr.data_ptr, arr.out_ptr, arr.n, ot.data_ptr(), len(lens), sync_stream())
        torch.cuda.synchronize()
        runs.append(arr.result())
    assert (runs[0].view(np.uint8) == runs[1].view(np.uint8)).all(), "the same call gave different bits"
    check(runs[0][:, 0], [d[b:e] for b, e in zip(offsets[:-1], offsets[1:])])
    for n in lens:
        parts = 2
        arr = Arrays(d[:n * parts], dt, parts)
        runs = []
        for _ in range(2):
            arr.reset_out()
            red.run_batch_ptr(arr.data_ptr, arr.out_ptr, n, parts, sync_stream())
            torch.cuda.synchronize()
            runs.append(arr.result())
        assert (runs[0].view(np.uint8) == runs[1].view(np.uint8)).all(), "the same call gave different bits"
        check(runs[0][:, 0], [d[p * n:(p + 1) * n] for p in range(parts)])


@pytest.mark.parametrize("dt,op", [(3, 0), (0, 2)])
def test_malformed_offsets_read_nothing_outside_the_array(G, dt, op):
    """Offsets that decrease or point beyond `total`: such segments are empty (identity), the well-formed ones are right, and no
    element outside [0, total) matters -- the allocation holds poison (uint32: all ones; float Min: -inf) in front of and behind
    the array -- while the guards around `out` stay intact.  (The well-formed segments overlap each other here; together they hold
    fewer than `total` elements, which is what the segment lists are sized for.)"""
    npdt, comps = O.dtype_info(dt)
    rng = np.random.default_rng(500 + dt)
    total = 400000
    o = [0, 100, 60, 200, total + 50, 300, 300, 5000, 5000 + 70000, total, total + 1, 2**32 - 1, 7, 40]
    d = make_data(rng, total, dt, op)
    poison = npdt(-np.inf) if np.issubdtype(npdt, np.floating) else npdt(0xFFFFFFFF)
    red = G.Reduce(dt, op)
    got = run_offsets(G, red, d, dt, o, shift=4, poison=poison)
    want = expected_segments(d, dt, op, o, total=total)
    well_formed = [s for s in range(len(o) - 1) if o[s] <= o[s + 1] <= total]
    assert well_formed == [0, 2, 5, 6, 7, 8, 12]
    for s in well_formed:
        assert (got[s] == want[s]).all(), (s, got[s], want[s])
    assert (got == want).all()  # (the malformed ones: the identity, as for any empty segment)


@pytest.mark.parametrize("length", [16, 64, 1024, 65536, 65537, 1 << 20])
def test_overlapping_segments_beyond_the_lists_capacity(G, length):
    """Offsets 0, L, 0, L, ...: every even segment is the whole array [0, L) again, every odd one runs backwards (empty).  The
    segments together hold 64 times `total`, far more than the list of their class (and, for the long ones, the chunk list) is
    sized for, so the clamped list lengths and the chunk list's end are what the kernels run into.  Memory safety is the contract
    then: every out element of a non-empty segment is either the right sum or still holds what it held before the call (never a
    sum of a part of the segment), at least one segment -- as many as `total` has room for -- is served, the empty ones get the
    identity, and the guards around `out`, the poison around `data` and `data` itself are as they were.  One length per list:
    4, 16 and 64 lanes, workgroup, long with two chunks and long with sixteen."""
    dt, op = 3, 0
    nonempty = 64
    rng = np.random.default_rng(600)
    d = make_data(rng, length, dt, op)
    o = [0, length] * nonempty + [0]
    untouched = np.uint32(GUARD_BYTE * 0x01010101)
    want = np.uint32(d.sum(dtype=np.uint64) & 0xFFFFFFFF)
    assert want != untouched
    red = G.Reduce(dt, op)
    got = run_offsets(G, red, d, dt, o, shift=4, poison=np.uint32(0xFFFFFFFF))[:, 0]
    assert (got[1::2] == 0).all(), "an empty segment did not get the identity"
    served = got[0::2] == want
    assert (served | (got[0::2] == untouched)).all(), got[0::2][~served]
    assert served.any()
    counts = red.read_batch()
    assert 1 <= counts["wave"] + counts["block"] + counts["long"] <= nonempty


def test_argument_checks(G):
    import ctypes

    import torch

    red = G.Reduce(G.DataType_UVec4, G.ReduceOperator_Sum)
    dtn = torch.zeros(4096, dtype=torch.int32, device="cuda")
    otn = torch.ones(64, dtype=torch.int32, device="cuda")
    off = torch.zeros(8, dtype=torch.int32, device="cuda")
    dp, op, fp = dtn.data_ptr(), otn.data_ptr(), off.data_ptr()
    L, vp = G.lib(), ctypes.c_void_p
    bad = [
        lambda: G.check(L.glu_reduce_run_batch_ptr(None, vp(dp), vp(op), 8, 4, None)),              # NULL reduce
        lambda: G.check(L.glu_reduce_run_batch_offsets_ptr(None, vp(dp), vp(op), 64, vp(fp), 4, None)),
        lambda: G.check(L.glu_reduce_prepare_batch(None, 64, 4)),
        lambda: G.check(L.glu_reduce_read_batch(None, None, None, None)),
        lambda: red.run_batch_ptr(None, op, 8, 4),                                                  # NULL data with a non-zero size
        lambda: red.run_batch_ptr(dp, None, 8, 4),                                                  # NULL out
        lambda: red.run_batch_ptr(dp, None, 0, 4),                                                  # NULL out, empty partitions
        lambda: red.run_batch_offsets_ptr(None, op, 64, fp, 4),
        lambda: red.run_batch_offsets_ptr(dp, None, 64, fp, 4),
        lambda: red.run_batch_offsets_ptr(dp, op, 64, None, 4),                                     # NULL offsets
        lambda: red.run_batch_offsets_ptr(dp, op, 64, fp + 2, 4),                                   # misaligned offsets
        lambda: red.run_batch_ptr(dp + 4, op, 8, 4),                                                # 16-byte elements 4 bytes off
        lambda: red.run_batch_ptr(dp, op + 8, 8, 4),
        lambda: red.run_batch_offsets_ptr(dp + 4, op, 64, fp, 4),
        lambda: red.run_batch_offsets_ptr(dp, op + 8, 64, fp, 4),
        lambda: red.run_batch_ptr(dp, op, 1, 1 << 31),                                              # num_partitions not below 2^31
        lambda: red.run_batch_ptr(dp, op, 1 << 40, 1 << 30),                                        # count * num_partitions overflows
        lambda: red.run_batch_offsets_ptr(dp, op, 1 << 32, fp, 4),                                  # total not below 2^32
        lambda: red.run_batch_offsets_ptr(dp, op, 64, fp, (1 << 24) + 1),                           # num_segments beyond 2^24
        lambda: red.prepare_batch(1 << 32, 4),
        lambda: red.prepare_batch(64, (1 << 24) + 1),
        lambda: red.run_batch_ptr(dp, dp + 64, 8, 4),                                               # out inside data
        lambda: red.run_batch_offsets_ptr(dp, dp, 64, fp, 4),
        lambda: G.plan_reduce_batch(8, 12),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, i
        assert e.value.message, i
    red.run_batch_ptr(None, None, 8, 0)  # nothing to do: NULL arrays are fine
    red.run_batch_offsets_ptr(None, None, 64, None, 0)
    assert red.read_batch() == {"wave": 0, "block": 0, "long": 0}
    red.run_batch_ptr(None, op, 0, 4)  # empty partitions read no data
    torch.cuda.synchronize()
    assert (otn.cpu().numpy()[:16] == 0).all() and (otn.cpu().numpy()[16:] == 1).all()  # four uvec4 identities of Sum
    otn.fill_(1)
    red.run_batch_offsets_ptr(None, op, 0, fp, 4)
    torch.cuda.synchronize()
    assert (otn.cpu().numpy()[:16] == 0).all() and (otn.cpu().numpy()[16:] == 1).all()


def test_prepared_batch_allocates_nothing_and_replays_from_a_graph(G):
    """After prepare_batch one run_batch_offsets_ptr call is captured on a side stream and replayed three times on new data and on
    DIFFERENT offsets in the same device arrays (the segments are binned on the device in every replay).  The prepared scratch does
    not change: a prepared call leaves the device's free memory as it found it (the object's scratch is the only thing the call
    could grow), and the capture itself refuses any allocation inside the captured call."""
    import torch

    dt, op = 3, 0
    rng = np.random.default_rng(14)
    total, nseg = 3_000_000, 771

    def draw_offsets():
        lens = mixed_lengths(rng, 4, extra=[0, 0, 0, 0, 0, 0])
        assert lens.size == nseg
        return np.minimum(np.concatenate([[0], np.cumsum(lens)]), total)

    red = G.Reduce(dt, op)
    kt = torch.empty(total, dtype=torch.int32, device="cuda")
    out = torch.empty(nseg, dtype=torch.int32, device="cuda")
    ot = torch.zeros(nseg + 1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def fill(d, offsets):
        kt.copy_(torch.from_numpy(d.view(np.int32)))
        ot.copy_(torch.from_numpy(offsets.astype(np.uint32).view(np.int32)))
        out.fill_(-1)

    def verify(d, offsets):
        want = expected_segments(d, dt, op, offsets)
        assert (out.cpu().numpy().view(np.uint32) == want[:, 0]).all()
        assert (kt.cpu().numpy().view(np.uint32) == d).all()
        lens = np.diff(offsets)
        rb = red.read_batch()
        assert rb["wave"] + rb["block"] + rb["long"] == int((lens > 0).sum()) and rb["long"] >= 2

    with torch.cuda.stream(side):
        d, offsets = make_data(rng, total, dt, op), draw_offsets()
        fill(d, offsets)
        side.synchronize()
        red.prepare_batch(total, nseg)
        red.run_batch_offsets_ptr(kt.data_ptr(), out.data_ptr(), total, ot.data_ptr(), nseg, side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(d, offsets)
        held = torch.cuda.mem_get_info()[0]
        out.fill_(-1)
        red.run_batch_offsets_ptr(kt.data_ptr(), out.data_ptr(), total, ot.data_ptr(), nseg, side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        verify(d, offsets)
        with torch.cuda.graph(graph, stream=side):
            red.run_batch_offsets_ptr(kt.data_ptr(), out.data_ptr(), total, ot.data_ptr(), nseg, torch.cuda.current_stream().cuda_stream)
        for rep in range(3):
            d, offsets = make_data(rng, total, dt, op), draw_offsets()
            fill(d, offsets)
            graph.replay()
            side.synchronize()
            verify(d, offsets)


def test_one_long_segment_of_2_28(G):
    import torch

    n = 1 << 28
    gen = torch.Generator(device="cuda").manual_seed(5)
    data = torch.randint(-(1 << 31), 1 << 31, (n,), generator=gen, device="cuda", dtype=torch.int32)
    want = int(data.cpu().numpy().view(np.uint32).sum(dtype=np.uint64)) & 0xFFFFFFFF
    out = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    ot = device_offsets([0, n])
    red = G.Reduce(G.DataType_Uint, G.ReduceOperator_Sum)
    red.run_batch_ptr(data.data_ptr(), out.data_ptr(), n, 1, sync_stream())
    torch.cuda.synchronize()
    assert red.read_batch() == {"wave": 0, "block": 0, "long": 1}
    red.run_batch_offsets_ptr(data.data_ptr(), out.data_ptr() + 4, n, ot.data_ptr(), 1, sync_stream())
    torch.cuda.synchronize()
    assert red.read_batch() == {"wave": 0, "block": 0, "long": 1}
    got = out.cpu().numpy().view(np.uint32)
    assert int(got[0]) == want and int(got[1]) == want and int(got[2]) == 0xFFFFFFFF and int(got[3]) == 0xFFFFFFFF
    del data
    torch.cuda.empty_cache()


def test_equal_partitions_beyond_32_bit_indices(G):
    """Two partitions of 2^31 + 5 int32: element indices need 64 bits.  Sum, and Max with the maximum in the very last element."""
    import torch

    count, parts = (1 << 31) + 5, 2
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * (1 << 30):
        pytest.skip("needs 24 GiB of free HBM")
    gen = torch.Generator(device="cuda").manual_seed(3)
    data = torch.empty(count * parts, dtype=torch.int32, device="cuda")
    step = 1 << 28
    for lo in range(0, count * parts, step):
        m = min(step, count * parts - lo)
        data[lo:lo + m] = torch.randint(-(1 << 20), 1 << 20, (m,), generator=gen, device="cuda", dtype=torch.int32)
    data[count * parts - 1] = (1 << 20) + 5
    data[count - 1] = (1 << 20) + 3

    def exact_sum(lo, hi):
        total, at = 0, lo
        while at < hi:
            m = min(step, hi - at)
            total += int(data[at:at + m].sum(dtype=torch.int64))
            at += m
        return ((total + (1 << 31)) % (1 << 32)) - (1 << 31)  # int32 wrap

    out = torch.zeros(parts, dtype=torch.int32, device="cuda")
    for op, want in ((G.ReduceOperator_Max, [(1 << 20) + 3, (1 << 20) + 5]),
                     (G.ReduceOperator_Sum, [exact_sum(0, count), exact_sum(count, 2 * count)])):
        red = G.Reduce(G.DataType_Int, op)
        red.run_batch_ptr(data.data_ptr(), out.data_ptr(), count, parts, sync_stream())
        torch.cuda.synchronize()
        assert out.cpu().tolist() == want, (op, out.cpu().tolist(), want)
        assert red.read_batch() == {"wave": 0, "block": 0, "long": 2}
    del data
    torch.cuda.empty_cache()


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_batch_reduce_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
