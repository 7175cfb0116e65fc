"""GPU tests of the batched reduce (glu_reduce_run_batch_ptr / glu_reduce_run_batch_offsets_ptr): out[s] = the reduction of
segment s, every segment on its own, the input only read.  Expected results come from numpy: oracle.reduce_expected /
oracle.dtype_info applied to every segment's slice, the operator's identity for an empty one.  Inputs are built the way
test_reduce_every_type_and_operator builds them (float sums that are exact in any order, products of mostly ones), so `==` is the
check for every type; the floats that do round have a test of their own against math.fsum."""
import gc
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


def packed_float_types():
    """The float types with several elements to a 16-byte pack (float, vec2, double): for them the lane an element goes to depends
    on where the 16-byte boundaries lie."""
    out = []
    for dt in range(12):
        npdt, comps = O.dtype_info(dt)
        if np.issubdtype(npdt, np.floating) and npdt().itemsize * comps < 16:
            out.append(dt)
    return out


PACKED_FLOATS = packed_float_types()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all()


def check_rounded(got, d, dt, op, offsets):
    """Sum: every component of every segment within n * eps * sum|x| of math.fsum (test_float_sums_that_round says why).  Product:
    within n * eps * |exact product|, the same bound in relative form: each of the n - 1 multiplications is off by a factor of at
    most 1 + eps / 2 whatever the order, (1 + eps / 2)^(n - 1) - 1 = (n - 1) * eps / 2 * (1 + O(n eps)), and the bound is twice
    that.  The centre is the product in numpy's longest float, float64 at the least: where that is float64 itself (and the
    element type is double) the centre can be off by as much as the result, (n - 1) * eps / 2, and the doubled bound still holds
    both.  Empty segments: the identity, exactly."""
    npdt, comps = O.dtype_info(dt)
    eps = float(np.finfo(npdt).eps)
    rows = d.reshape(-1, comps)
    for s, (b, e) in enumerate(zip(offsets[:-1], offsets[1:])):
        n = int(e - b)
        for c in range(comps):
            x = rows[b:e, c]
            value = float(got[s, c])
            if n == 0:
                assert value == float(identity(npdt, op)), (s, value)
            elif op == 0:
                exact = math.fsum(x.astype(np.float64).tolist())
                bound = n * eps * math.fsum(np.abs(x).astype(np.float64).tolist())
                assert abs(value - exact) <= bound, (s, n, value, exact, bound)
            else:
                exact = float(np.prod(x.astype(np.longdouble)))
                bound = n * eps * abs(exact)
                assert abs(value - exact) <= bound, (s, n, value, exact, bound)


@pytest.mark.parametrize("dt", PACKED_FLOATS)
@pytest.mark.parametrize("op", [0, 1])
def test_long_float_bits_do_not_depend_on_the_order_of_binning(G, dt, op):
    """The twin of the batched scan's test of this name.  Three long segments of 3, 5 and 9 chunks among 900 short ones, more than
    256 segments apart, so that different workgroups of the binning kernel hand out their chunk slots in whatever order they
    arrive.  A segment's run of partials then starts at a slot that depends on that order -- and whatever the order, at least
    one run starts at an odd slot (the chunk counts are odd).  Full-mantissa values (Sum: normal; Product: exp(N(0, 0.01)), whose
    longest product has a logarithm of standard deviation 0.01 * sqrt(9 * 65536) = 7.7, against 87 where float32 ends), so another
    order of combination shows in the bits.  The whole `out` must be bit for bit the same from call to call, every long
    segment's result bit for bit what a batch of that segment alone gives on the same array (its partials at slot 0), and every
    result within the bound of check_rounded."""
    npdt, comps = O.dtype_info(dt)
    es = npdt().itemsize * comps
    wave, block = class_limits(G, es)
    chunk = block  # (a long segment's chunks are as long as the longest workgroup segment: checked through the plan below)
    rng = np.random.default_rng(700 + dt * 4 + op)
    lens = rng.integers(0, 40, 900)
    long_at = {10: 3, 400: 5, 800: 9}  # segment index: chunks
    for s, chunks in long_at.items():
        lens[s] = chunks * chunk - 7
        assert G.plan_reduce_batch(int(lens[s]), es) == (3, chunks)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = rng.standard_normal(int(offsets[-1]) * comps)
    if op == 1:
        d = np.exp(0.01 * d)
    d = d.astype(npdt)
    if op == 1:  # far from overflow and underflow: every prefix of the longest segment's product, in float64
        b, e = int(offsets[800]), int(offsets[801])
        logs = np.cumsum(np.log(d.reshape(-1, comps)[b:e].astype(np.float64)), axis=0)
        assert np.abs(logs).max() < 0.5 * math.log(float(np.finfo(np.float32).max)), np.abs(logs).max()
    red = G.Reduce(dt, op)
    runs = []
    for _ in range(3):
        runs.append(run_offsets(G, red, d, dt, offsets))
        assert red.read_batch()["long"] == 3
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2]), "the same call gave different bits"
    for s in long_at:
        b, e = int(offsets[s]), int(offsets[s + 1])
        alone = run_offsets(G, red, d, dt, [b, e])
        assert red.read_batch() == {"wave": 0, "block": 0, "long": 1}
        print("segment %d (%d chunks): in the batch %r, alone %r" % (s, long_at[s], runs[0][s].tolist(), alone[0].tolist()))
        assert same_bits(alone[0], runs[0][s]), (s, long_at[s], runs[0][s].tolist(), alone[0].tolist())
    check_rounded(runs[0], d, dt, op, offsets)


def parent_order_of_partials(p, head, vec):
    """What a workgroup made of a run of at most 16 partials before the partials were laid out from the run's first element:
    `head` elements in front of the 16-byte boundary one to a lane, then packs of `vec` elements, pack i to lane i, the elements
    behind the last pack one to a lane again; then the lanes of the wave combined at distances 32, 16, ... 1.  In p's type."""
    assert len(p) <= 16
    acc = [None] * 64

    def fold(lane, v):
        acc[lane] = v if acc[lane] is None else acc[lane] + v

    head = min(head, len(p))
    for t in range(head):
        fold(t, p[t])
    npacks = (len(p) - head) // vec
    for i in range(npacks):
        for k in range(vec):
            fold(i, p[head + i * vec + k])
    for t in range(head + npacks * vec, len(p)):
        fold(t - head - npacks * vec, p[t])
    off = 32
    while off:
        new = list(acc)
        for lane in range(64 - off):
            if acc[lane + off] is not None:
                new[lane] = acc[lane + off] if acc[lane] is None else acc[lane] + acc[lane + off]
        acc, off = new, off // 2
    return acc[0]


# partials whose sum depends on the order of addition, in units of (B, 1) with B = 2 / eps (B + 1 rounds to B): by elements to a
# 16-byte pack and chunks.  Two elements to a pack and three chunks: both layouts add (p0 + p1) + p2, no set can tell them apart.
ORDER_SENSITIVE = {
    (4, 3): "B 1 -B", (4, 5): "B B 1 -B -B", (4, 7): "B B 1 -B 1 1 -B",
    (2, 3): "B 1 -B", (2, 5): "B B 1 1 -B", (2, 7): "B B B 1 1 -B -B",
}


@pytest.mark.parametrize("dt", PACKED_FLOATS)
def test_equal_partitions_of_identical_data_give_identical_bits(G, dt):
    """Four equal partitions that hold the same long segment, of 3, 5 and 7 chunks: their runs of partials start at slots 0, c,
    2c, 3c, which for an odd c are all residues modulo the elements of a 16-byte pack.  The segment is a multiple of 16 bytes
    long, so every copy has the same alignment, and the four results must have the same bits -- those of the segment alone
    through the offsets form.  Two data sets: random normal values, and chunks of +0.0 with one non-zero element each at a random
    place (so every partial is that element, exactly) chosen so that the order of their addition decides the sum;
    parent_order_of_partials, on the CPU, shows that they tell the earlier layouts apart."""
    npdt, comps = O.dtype_info(dt)
    es = npdt().itemsize * comps
    vec = 16 // es
    wave, block = class_limits(G, es)
    chunk, parts = block, 4
    rng = np.random.default_rng(800 + dt)
    red = G.Reduce(dt, 0)
    big = npdt(2) / np.finfo(npdt).eps
    for chunks in (3, 5, 7):
        count = chunks * chunk - 3 * vec
        assert G.plan_reduce_batch(count, es) == (3, chunks) and count * es % 16 == 0
        assert sorted((p * chunks) % vec for p in range(parts)) == sorted(p % vec for p in range(parts))
        partials = [{"B": big, "-B": -big, "1": npdt(1)}[w] for w in ORDER_SENSITIVE[vec, chunks].split()]
        assert len(partials) == chunks
        by_head = [parent_order_of_partials(partials, head, vec) for head in range(vec)]
        print("type %d (%s), %d chunks: the earlier layouts gave %r" % (dt, npdt.__name__, chunks, [float(v) for v in by_head]))
        assert len(set(float(v) for v in by_head)) >= 2 or (vec == 2 and chunks < 5), "the partials do not tell the layouts apart"
        engineered = np.zeros((count, comps), dtype=npdt)
        for c, value in enumerate(partials):
            at = c * chunk + rng.integers(0, min(chunk, count - c * chunk), comps)
            engineered[at, np.arange(comps)] = [value, -value][:comps]  # (a second component: the negated set)
        for name, one in (("normal", rng.standard_normal(count * comps).astype(npdt)), ("engineered", engineered.reshape(-1))):
            got = run_equal(G, red, np.tile(one, parts), dt, count, parts)
            assert red.read_batch() == {"wave": 0, "block": 0, "long": parts}
            alone = run_offsets(G, red, one, dt, [0, count])
            print("type %d, %d chunks, %s: partitions %r, alone %r" % (dt, chunks, name, got.tolist(), alone[0].tolist()))
            for p in range(parts):
                assert same_bits(got[p], got[0]), (chunks, name, p, got.tolist())
            assert same_bits(got[0], alone[0]), (chunks, name, got[0].tolist(), alone[0].tolist())
            if name == "engineered":  # (whatever the order, the sum of these is one of a few integers)
                exact = math.fsum(float(v) for v in partials)
                assert abs(float(got[0, 0]) - exact) <= chunks and float(got[0, comps - 1]) == (-1) ** (comps - 1) * float(got[0, 0])


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("shift", [0, 1])
def test_a_result_depends_on_alignment_length_and_data_only(G, dt, shift):
    """float and double Sum, one segment length per list (4, 16 and 64 lanes, workgroup, long with two chunks), each a multiple of
    16 bytes: the same random normal segment five times in one array, filler segments of other multiples of 16 bytes between the
    copies -- none, a few, more than a binning workgroup holds -- so that the copies have the same address modulo 16 and
    different segment indices, list positions and neighbours.  The five results have the same bits, and the bits of the five
    copies laid back to back as equal partitions.  With the array on a 16-byte boundary and one element behind it."""
    npdt, comps = O.dtype_info(dt)
    es = npdt().itemsize
    vec = 16 // es
    wave, block = class_limits(G, es)
    two = next(c for c in range(block + 1, 4 * block + 4) if G.plan_reduce_batch(c, es)[1] == 3) - 1  # last length on two workgroups
    rng = np.random.default_rng(900 + dt * 2 + shift)
    red = G.Reduce(dt, 0)
    lists = []
    for length in (16, 64, wave, block, two):
        length -= length % vec
        seg = rng.standard_normal(length).astype(npdt)
        lens, copies = [], []
        for fillers in (0, 3, 300, 17, 64):
            lens += (vec * rng.integers(0, 50, fillers)).tolist()
            copies.append(len(lens))
            lens.append(length)
        lens.append(vec * 5)
        offsets = np.concatenate([[0], np.cumsum(lens)])
        d = rng.standard_normal(int(offsets[-1])).astype(npdt)
        for s in copies:
            d[offsets[s]:offsets[s + 1]] = seg
        got = run_offsets(G, red, d, dt, offsets, shift=shift)
        lists.append(G.plan_reduce_batch(length, es))
        equal = run_equal(G, red, np.tile(seg, 5), dt, length, 5, shift=shift)
        print("%s, %d elements, shift %d: %r, as equal partitions %r" % (npdt.__name__, length, shift, got[copies, 0].tolist(), equal[:, 0].tolist()))
        for s in copies:
            assert same_bits(got[s], got[copies[0]]), (length, s, got[copies, 0].tolist())
        for p in range(5):
            assert same_bits(equal[p], got[copies[0]]), (length, p, equal[:, 0].tolist(), got[copies[0]].tolist())
        exact = math.fsum(seg.astype(np.float64).tolist())
        assert abs(float(got[copies[0], 0]) - exact) <= length * float(np.finfo(npdt).eps) * math.fsum(np.abs(seg).astype(np.float64).tolist())
    assert lists == [(1, 1), (1, 1), (1, 1), (2, 1), (3, 2)] and 16 < 64 < wave  # (up to 16 / up to 64 elements / longer: 4 / 16 / 64 lanes)


def test_a_run_of_partials_longer_than_one_round_of_the_workgroup(G):
    """Two equal partitions of the same 1601 chunks of doubles (random normal, made on the device): 800 packs of two partials and
    one partial behind them, so the lanes of the workgroup that folds the run take one, three or four packs each, through the
    loop with four loads in flight and the one behind it.  Partition 0's run lies on a 16-byte boundary and is read with
    16-byte loads, partition 1's starts at slot 1601 and is read element by element: the same bits, those of the segment alone
    through the offsets form, within n * eps * sum|x| of the sum torch takes in float64 on the device (pairwise in blocks: its
    own error is far inside the bound)."""
    import torch

    dt, chunks = 1, 1601
    wave, block = class_limits(G, 8)
    count = chunks * block - 2
    assert G.plan_reduce_batch(count, 8) == (3, chunks)
    gen = torch.Generator(device="cuda").manual_seed(17)
    one = torch.randn(count, generator=gen, device="cuda", dtype=torch.float64)
    data = torch.cat([one, one])
    out = torch.full((5,), -1.0, dtype=torch.float64, device="cuda")
    ot = device_offsets([0, count])
    red = G.Reduce(dt, 0)
    red.run_batch_ptr(data.data_ptr(), out.data_ptr(), count, 2, sync_stream())
    torch.cuda.synchronize()
    assert red.read_batch() == {"wave": 0, "block": 0, "long": 2}
    red.run_batch_offsets_ptr(data.data_ptr(), out.data_ptr() + 16, count, ot.data_ptr(), 1, sync_stream())
    torch.cuda.synchronize()
    assert red.read_batch() == {"wave": 0, "block": 0, "long": 1}
    got = out.cpu().numpy()
    exact, scale = float(one.sum()), float(one.abs().sum())
    print("partitions %r, alone %r, torch %r" % (got[:2].tolist(), float(got[2]), exact))
    assert same_bits(got[0:1], got[1:2]) and same_bits(got[0:1], got[2:3]), got[:3].tolist()
    assert (got[3:] == -1.0).all()
    assert abs(float(got[0]) - exact) <= count * float(np.finfo(np.float64).eps) * scale
    del data, one
    torch.cuda.empty_cache()


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
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
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
