"""GPU tests of the batched scan (glu_scan_run_batch_offsets_ptr): every segment [offsets[s], offsets[s+1]) of an array replaced by
its own exclusive `+` scan, in place, everything else left alone.  Expected values come from numpy (a cumulative sum per segment,
in uint64 / float64).  Integer inputs are random words (sums wrap modulo 2^32); float inputs are k x 0.125 with integer k bounded
per segment so that length x max|k| < 2^24: every partial sum is then exact in float32 in any order, so `==` is the check for
every type.  Floats that do round have a test of their own against math.fsum.  The class limits are read from plan_scan_batch."""
import gc
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8  # elements of poison in front of and behind the array, inside the allocation


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return built


def elem_bytes(dt):
    npdt, comps = O.dtype_info(dt)
    return npdt().itemsize * comps


def class_limits(G, es):
    """Last length of the wave class, last length of the workgroup class and the chunk of the long class, from plan_scan_batch."""
    def last_where(pred):
        lo, hi = 0, 1 << 40  # pred(lo) and not pred(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if pred(mid):
                lo = mid
            else:
                hi = mid
        return lo
    wave = last_where(lambda c: G.plan_scan_batch(c, es)[0] <= 1)
    block = last_where(lambda c: G.plan_scan_batch(c, es)[0] <= 2)
    w0 = G.plan_scan_batch(block + 1, es)[1]
    chunk = last_where(lambda c: c <= block or G.plan_scan_batch(c, es)[1] <= w0) // w0
    assert G.plan_scan_batch(wave, es)[0] == 1 and G.plan_scan_batch(wave + 1, es)[0] == 2
    assert G.plan_scan_batch(block, es)[0] == 2 and G.plan_scan_batch(block + 1, es)[0] == 3
    assert G.plan_scan_batch(3 * chunk, es)[1] in (1, 3) and G.plan_scan_batch(3 * chunk + 1, es) == (3, 4)
    return wave, block, chunk


def poison_of(npdt):
    """A pattern no scan produces: a NaN with a payload for floats, a fixed word for integers."""
    if npdt == np.float32:
        return np.array([0x7FC5A5A5], dtype=np.uint32).view(np.float32)[0]
    if npdt == np.float64:
        return np.array([0x7FF8A5A5A5A5A5A5], dtype=np.uint64).view(np.float64)[0]
    return np.array([0xA5A5A5A5], dtype=np.uint32).view(npdt)[0]


def make_data(rng, dt, offsets, total):
    """total * components scalars; floats: k * 0.125 with |k| * length < 2^24 inside every segment."""
    npdt, comps = O.dtype_info(dt)
    if not np.issubdtype(npdt, np.floating):
        return rng.integers(0, 2**32, total * comps, dtype=np.uint32).view(npdt)
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.diff(offsets)
    kmax = np.minimum(4000, ((1 << 24) - 1) // np.maximum(lens, 1))
    per_elem = np.full(total, 4000, dtype=np.int64)
    per_elem[offsets[0]:offsets[-1]] = np.repeat(kmax, lens)
    per_scalar = np.repeat(per_elem, comps)
    k = np.floor(rng.random(total * comps) * (2 * per_scalar + 1)).astype(np.int64) - per_scalar
    return (k * 0.125).astype(npdt)


def expected_scan(d, dt, offsets):
    """d with every segment replaced by its exclusive cumulative sum (non-decreasing offsets); the rest as it was."""
    npdt, comps = O.dtype_info(dt)
    rows = d.reshape(-1, comps)
    out = rows.copy()
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.diff(offsets)
    assert (lens >= 0).all()
    b, e = int(offsets[0]), int(offsets[-1])
    if np.issubdtype(npdt, np.floating):
        wide = rows[b:e].astype(np.float64)
    else:
        wide = rows[b:e].view(np.uint32).astype(np.uint64)
    cum = np.zeros((e - b + 1, comps), dtype=wide.dtype)
    np.cumsum(wide, axis=0, out=cum[1:])
    excl = cum[:-1] - np.repeat(cum[offsets[:-1] - b], lens, axis=0)
    if np.issubdtype(npdt, np.floating):
        out[b:e] = excl.astype(npdt)
    else:
        out[b:e] = (excl & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(npdt)
    return out.reshape(-1)


class Array:
    """`d` on the device, `shift` elements behind the start of an allocation that holds poison in front of and behind it."""

    def __init__(self, d, dt, shift=0):
        import torch

        npdt, comps = O.dtype_info(dt)
        self.npdt, self.comps, self.es = npdt, comps, npdt().itemsize * comps
        self.front = (GUARD + shift) * comps
        self.host = np.concatenate([np.full(self.front, poison_of(npdt), dtype=npdt), d, np.full(GUARD * comps, poison_of(npdt), dtype=npdt)])
        self.n = d.size // comps
        self.t = torch.from_numpy(self.host.view(np.uint8).copy()).cuda()
        self.ptr = self.t.data_ptr() + (GUARD + shift) * self.es

    def result(self):
        """The array after the call; asserts that the poison around it is intact."""
        raw = self.t.cpu().numpy()
        want = self.host.view(np.uint8)
        lo, hi = self.front * self.npdt().itemsize, (self.front + self.n * self.comps) * self.npdt().itemsize
        assert (raw[:lo] == want[:lo]).all() and (raw[hi:] == want[hi:]).all(), "the call wrote outside the array"
        return raw[lo:hi].copy().view(self.npdt)


def device_offsets(offsets):
    import torch

    return torch.from_numpy(np.asarray(offsets, dtype=np.uint32).view(np.int32).copy()).cuda()


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all()


def run(G, scan, d, dt, offsets, shift=0, total=None):
    import torch

    arr = Array(d, dt, shift)
    ot = device_offsets(offsets)
    scan.run_batch_offsets_ptr(arr.ptr, arr.n if total is None else total, ot.data_ptr(), len(offsets) - 1, stream())
    torch.cuda.synchronize()
    return arr.result()


def first_difference(got, want, offsets, comps):
    bad = np.nonzero(got.view(np.uint8).reshape(-1, got.itemsize * comps) != want.view(np.uint8).reshape(-1, want.itemsize * comps))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    s = int(np.searchsorted(np.asarray(offsets), i, side="right")) - 1
    return {"element": i, "segment": s, "length": int(offsets[s + 1] - offsets[s]) if 0 <= s < len(offsets) - 1 else None}


@pytest.mark.parametrize("dt", range(12))
def test_every_type_across_the_class_boundaries(G, dt):
    npdt, comps = O.dtype_info(dt)
    es = elem_bytes(dt)
    wave, block, chunk = class_limits(G, es)
    rng = np.random.default_rng(100 + dt)
    lens = [0, 1, 2, 3, 63, 64, 65]
    for limit in (wave, block):
        lens += [limit - 1, limit, limit + 1]
    lens.append(3 * chunk + 1)
    lens += [n + more for n in (4, 8, 16, 32, 128, 256, 512) if n < wave for more in (0, 1)]  # (wherever the lanes per segment step)
    lens = [lens[i] for i in rng.permutation(len(lens))]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = make_data(rng, dt, offsets, int(offsets[-1]))
    scan = G.BlellochScan(dt)
    got = run(G, scan, d, dt, offsets)
    want = expected_scan(d, dt, offsets)
    assert same_bits(got, want), (dt, first_difference(got, want, offsets, comps))
    rb = scan.read_batch()
    paths = [G.plan_scan_batch(n, es)[0] for n in lens]
    assert [rb["wave"], rb["block"], rb["long"]] == [paths.count(p) for p in (1, 2, 3)]
    assert rb["wave"] > 0 and rb["block"] > 0 and rb["long"] > 0


def mixed_lengths(rng, es, extra=()):
    """Zeros, ones, geometric around 40, uniform up to 3000, a few workgroup-sized and long ones, shuffled."""
    lens = np.concatenate([np.zeros(20, np.int64), np.ones(20, np.int64), rng.geometric(1 / 40.0, 600), rng.integers(0, 3001, 120),
                           np.asarray([20000 // es * 4, 65536 // es, 65536 // es + 1, 1000000 // es * 4, 3 * 65536 // es + 7], dtype=np.int64),
                           np.asarray(extra, dtype=np.int64)])
    rng.shuffle(lens)
    return lens


@pytest.mark.parametrize("dt", [3, 0, 7])
def test_untouched_surroundings(G, dt):
    """offsets[0] > 0 and offsets[n] < total: the elements of the array in front of the first and behind the last segment hold
    poison (a NaN payload for floats), like the allocation around the array; all of it is intact after the call, bit for bit."""
    npdt, comps = O.dtype_info(dt)
    es = elem_bytes(dt)
    rng = np.random.default_rng(200 + dt)
    lens = np.concatenate([[0, 0, 1], mixed_lengths(rng, es), [1, 0, 0]])
    head, tail = 777, 1234
    offsets = np.concatenate([[0], np.cumsum(lens)]) + head
    total = int(offsets[-1]) + tail
    d = make_data(rng, dt, offsets, total)
    d[:head * comps] = poison_of(npdt)
    d[int(offsets[-1]) * comps:] = poison_of(npdt)
    scan = G.BlellochScan(dt)
    got = run(G, scan, d, dt, offsets, shift=1)
    want = expected_scan(d, dt, offsets)
    assert same_bits(got[:head * comps], d[:head * comps]) and same_bits(got[int(offsets[-1]) * comps:], d[int(offsets[-1]) * comps:])
    assert same_bits(got, want), first_difference(got, want, offsets, comps)
    rb = scan.read_batch()
    paths = [G.plan_scan_batch(int(n), es)[0] for n in lens]
    assert [rb["wave"], rb["block"], rb["long"]] == [paths.count(p) for p in (1, 2, 3)]


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_bases(G, shift):
    """uint32 arrays that start 4, 8 and 12 bytes behind a 16-byte boundary; the batch holds segments of every class that start
    at every address modulo 16 bytes (the lengths 1, 2, 3 between them move the starts around)."""
    dt = 3
    wave, block, chunk = class_limits(G, 4)
    rng = np.random.default_rng(300 + shift)
    lens, at = [], 0
    for n in (5, 33, 200, wave, wave + 1, 5000, block, block + 1, 2 * chunk + 3):
        for residue in (0, 1, 2, 3):  # a segment of 0 .. 3 elements in front moves the start to every residue modulo 4 elements
            pad = (residue - at) % 4
            lens += [pad, n]
            at += pad + n
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    for n in set(lens[1::2]):
        assert {int(s) % 4 for s, m in zip(starts[1::2], lens[1::2]) if m == n} == {0, 1, 2, 3}, n
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = make_data(rng, dt, offsets, int(offsets[-1]))
    got = run(G, G.BlellochScan(dt), d, dt, offsets, shift=shift)
    want = expected_scan(d, dt, offsets)
    assert same_bits(got, want), first_difference(got, want, offsets, 1)


def test_a_million_tiny_segments(G):
    """2^20 segments of 0 .. 7 elements: binning and list walking at scale."""
    dt = 3
    rng = np.random.default_rng(13)
    lens = rng.integers(0, 8, 1 << 20)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = make_data(rng, dt, offsets, int(offsets[-1]))
    scan = G.BlellochScan(dt)
    got = run(G, scan, d, dt, offsets)
    assert same_bits(got, expected_scan(d, dt, offsets))
    assert scan.read_batch() == {"wave": int((lens > 0).sum()), "block": 0, "long": 0}


@pytest.mark.parametrize("dt", [0, 1])
def test_float_sums_that_round(G, dt):
    """float32 / float64, random normal values (full mantissas), one segment per class.  For every element
    |got - exact| <= gamma * sum|x_j| over that element's prefix, gamma = (n - 1) u / (1 - (n - 1) u) with n the number of values
    in the prefix and u = 2^-24 / 2^-53: the standard bound of summation in ANY order (Higham, Accuracy and Stability of Numerical
    Algorithms, section 4.2), derived and not tuned.  The exact prefix sums are carried as Python fractions (what math.fsum of
    the prefix rounds); rounding them to float64 for the comparison adds 2^-53 of their magnitude to the bound.  A second
    identical call gives identical bits."""
    import torch

    npdt, _ = O.dtype_info(dt)
    es = npdt().itemsize
    wave, block, chunk = class_limits(G, es)
    lens = [wave - 3, block - 5, 3 * chunk + 11]
    assert [G.plan_scan_batch(n, es)[0] for n in lens] == [1, 2, 3]
    rng = np.random.default_rng(400 + dt)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = rng.standard_normal(int(offsets[-1])).astype(npdt)
    u = 2.0 ** -24 if dt == 0 else 2.0 ** -53
    scan = G.BlellochScan(dt)
    runs = []
    for _ in range(2):
        arr = Array(d, dt)
        ot = device_offsets(offsets)
        scan.run_batch_offsets_ptr(arr.ptr, arr.n, ot.data_ptr(), len(lens), stream())
        torch.cuda.synchronize()
        runs.append(arr.result())
    assert same_bits(runs[0], runs[1]), "the same call gave different bits"
    for b, e in zip(offsets[:-1], offsets[1:]):
        x = d[b:e].astype(np.float64)
        got = runs[0][b:e].astype(np.float64)
        n = np.arange(e - b, dtype=np.float64)  # element i: the sum of i values
        abs_sum = np.concatenate([[0.0], np.cumsum(np.abs(x))[:-1]])
        gamma = np.maximum(n - 1, 0) * u / (1 - np.maximum(n - 1, 0) * u)
        exact = np.empty(e - b, dtype=np.float64)
        acc = Fraction(0)
        for i, v in enumerate(x.tolist()):
            exact[i] = float(acc)
            acc += Fraction(v)
        err = np.abs(got - exact)
        bound = gamma * abs_sum + np.abs(exact) * 2.0 ** -53  # (+ the rounding of float(acc) itself)
        worst = int(np.argmax(err))
        print("n = %d: largest error at element %d: |got - exact| = %.3e, bound there %.3e" % (e - b, worst, err[worst], bound[worst]))
        assert got[0] == 0
        assert (err <= bound).all(), (int(e - b), worst, float(err[worst]), float(bound[worst]))


def test_float_bits_do_not_depend_on_the_order_of_binning(G):
    """Several long float32 segments in one batch: 3, 5 and 9 chunks, more than 256 segments apart, so that different workgroups
    of the binning kernel hand out their chunk slots in whatever order they arrive.  A segment's run of partials then starts at
    a slot that depends on that order -- and whatever the order, at least one run starts at an odd slot (the chunk counts are
    odd).  Random full-mantissa values, so a different order of addition shows in the bits.  Every long segment must come out
    bit for bit as it does when it is the only segment of a batch on the same array (its partials at slot 0), and the whole
    array bit for bit the same from call to call."""
    import torch

    dt = 0
    wave, block, chunk = class_limits(G, 4)
    rng = np.random.default_rng(16)
    lens = rng.integers(0, 40, 900)
    long_at = {10: 3, 400: 5, 800: 9}  # segment index: chunks
    for s, chunks in long_at.items():
        lens[s] = chunks * chunk - 7
        assert G.plan_scan_batch(int(lens[s]), 4) == (3, chunks)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    d = rng.standard_normal(int(offsets[-1])).astype(np.float32)
    scan = G.BlellochScan(dt)
    runs = []
    for _ in range(3):
        runs.append(run(G, scan, d, dt, offsets))
        assert scan.read_batch()["long"] == 3
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2]), "the same call gave different bits"
    for s in long_at:
        b, e = int(offsets[s]), int(offsets[s + 1])
        alone = run(G, scan, d, dt, [b, e])
        assert scan.read_batch() == {"wave": 0, "block": 0, "long": 1}
        assert same_bits(alone[b:e], runs[0][b:e]), (s, first_difference(alone[b:e], runs[0][b:e], [0, e - b], 1))
        assert same_bits(alone[:b], d[:b]) and same_bits(alone[e:], d[e:])


def test_integer_results_equal_the_single_scan(G):
    """For a handful of segments of every class: the batched result equals glu_scan_run_ptr on that slice alone."""
    import torch

    dt = 3
    wave, block, chunk = class_limits(G, 4)
    rng = np.random.default_rng(15)
    lens = [7, 64, 1000, wave + 1, 5001, block, block + 1, 5 * chunk + 17]
    offsets = np.concatenate([[3], 3 + np.cumsum(lens)])
    d = make_data(rng, dt, offsets, int(offsets[-1]) + 5)
    scan = G.BlellochScan(dt)
    got = run(G, scan, d, dt, offsets)
    single = G.BlellochScan(dt)
    for b, e in zip(offsets[:-1], offsets[1:]):
        t = torch.from_numpy(d[b:e].view(np.int32).copy()).cuda()
        single.run_ptr(t.data_ptr(), int(e - b), 1, stream())
        torch.cuda.synchronize()
        assert (t.cpu().numpy().view(np.uint32) == got[b:e]).all(), int(e - b)


def test_a_long_segment_whose_partials_take_two_steps_of_their_scan(G):
    """The partials of a long segment -- one per chunk -- are scanned by one workgroup, tile after tile of 4096 uint32 (the tile
    of the medium class: 256 threads x 4 groups x a 16-byte pack, ScanCfg::CHUNK).  With the first long segment's partials at
    the start of the (aligned) partials array, 4096 of them are one tile and 4097 need a second step: the smallest such count
    is 4096 chunks + 1 element, 4096 * 8192 + 1 = 2^25 + 1 uint32 with the 32 KiB chunk (read from plan_scan_batch)."""
    import torch

    dt = 3
    tile = 4096
    _, _, chunk = class_limits(G, 4)
    n = tile * chunk + 1
    assert n <= 1 << 26 and G.plan_scan_batch(n, 4) == (3, tile + 1) and G.plan_scan_batch(n - 1, 4) == (3, tile)
    gen = torch.Generator(device="cuda").manual_seed(7)
    data = torch.randint(-(1 << 31), 1 << 31, (n,), generator=gen, device="cuda", dtype=torch.int32)
    host = data.cpu().numpy().view(np.uint32)
    want = np.zeros(n, dtype=np.uint64)
    np.cumsum(host[:-1], dtype=np.uint64, out=want[1:])
    ot = device_offsets([0, n])
    scan = G.BlellochScan(dt)
    scan.run_batch_offsets_ptr(data.data_ptr(), n, ot.data_ptr(), 1, stream())
    torch.cuda.synchronize()
    assert scan.read_batch() == {"wave": 0, "block": 0, "long": 1}
    got = data.cpu().numpy().view(np.uint32)
    bad = np.nonzero(got != (want & np.uint64(0xFFFFFFFF)).astype(np.uint32))[0]
    assert bad.size == 0, (int(bad[0]), int(bad[0]) // chunk)
    del data
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", ["descending", "beyond_total", "all_ones", "mixed"])
def test_malformed_offsets_touch_nothing_outside_the_array(G, case):
    """Descending pairs, ends beyond `total`, all-0xFFFFFFFF: the call returns GLU_OK and the poison in front of and behind the
    array is intact.  Nothing is asserted about the contents of [0, total)."""
    dt = 3
    total = 200000
    offsets = {
        "descending": [total, 150000, 100000, 70000, 100, 0],
        "beyond_total": [0, total + 1, total + 70000, 2**32 - 1, 5, total + 5, 100, 2 * total],
        "all_ones": [0xFFFFFFFF] * 9,
        "mixed": [0, 100, 60, 200, total + 50, 300, 300, 5000, 5000 + 70000, total, total + 1, 2**32 - 1, 7, 40, 0, total, 0, total],
    }[case]
    rng = np.random.default_rng(500)
    d = rng.integers(0, 2**32, total, dtype=np.uint32)
    scan = G.BlellochScan(dt)
    got = run(G, scan, d, dt, offsets, shift=1)  # (GluError if the status is not GLU_OK; result() checks the poison)
    assert got.size == total
    rb = scan.read_batch()
    well_formed = sum(1 for b, e in zip(offsets[:-1], offsets[1:]) if b < e <= total)
    assert rb["wave"] + rb["block"] + rb["long"] <= well_formed


def test_argument_checks(G):
    import ctypes

    import torch

    scan = G.BlellochScan(G.DataType_UVec4)
    dtn = torch.zeros(4096, dtype=torch.int32, device="cuda")
    off = torch.zeros(8, dtype=torch.int32, device="cuda")
    dp, fp = dtn.data_ptr(), off.data_ptr()
    L, vp = G.lib(), ctypes.c_void_p
    bad = [
        (lambda: G.check(L.glu_scan_run_batch_offsets_ptr(None, vp(dp), 64, vp(fp), 4, None)), "scan is NULL"),
        (lambda: G.check(L.glu_scan_prepare_batch(None, 64, 4)), "scan is NULL"),
        (lambda: G.check(L.glu_scan_read_batch(None, None, None, None)), "scan is NULL"),
        (lambda: scan.run_batch_offsets_ptr(None, 64, fp, 4), "Invalid data buffer"),
        (lambda: scan.run_batch_offsets_ptr(dp, 64, None, 4), "Invalid offsets array"),
        (lambda: scan.run_batch_offsets_ptr(dp, 64, fp + 2, 4), "offsets array is not aligned"),
        (lambda: scan.run_batch_offsets_ptr(dp + 4, 64, fp, 4), "data is not aligned"),
        (lambda: scan.run_batch_offsets_ptr(dp, 1 << 32, fp, 4), "fewer than 2^32"),
        (lambda: scan.run_batch_offsets_ptr(dp, 64, fp, (1 << 24) + 1), "exceeds 2^24"),
        (lambda: scan.prepare_batch(1 << 32, 4), "fewer than 2^32"),
        (lambda: scan.prepare_batch(64, (1 << 24) + 1), "exceeds 2^24"),
        (lambda: G.plan_scan_batch(8, 12), "elem_bytes"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, i
        assert message in e.value.message, (i, e.value.message)
    scan.run_batch_offsets_ptr(None, 64, None, 0)  # nothing to do: NULL arrays are fine
    assert scan.read_batch() == {"wave": 0, "block": 0, "long": 0}
    scan.run_batch_offsets_ptr(None, 0, fp, 4)  # an array of no elements: every segment is empty
    torch.cuda.synchronize()
    assert scan.read_batch() == {"wave": 0, "block": 0, "long": 0}
    assert (dtn.cpu().numpy() == 0).all()


def test_prepared_batch_allocates_nothing_and_replays_from_a_graph(G):
    """After prepare_batch a call leaves the device's free memory as it found it, and one call captured on a side stream is
    replayed three times on new data and on DIFFERENT offsets in the same device arrays (the segments are binned on the device
    in every replay)."""
    import torch

    dt = 3
    rng = np.random.default_rng(14)
    total, nseg = 3_000_000, 771

    def draw_offsets():
        lens = mixed_lengths(rng, 4, extra=[0, 0, 0, 0, 0, 0])
        assert lens.size == nseg
        return np.minimum(np.concatenate([[0], np.cumsum(lens)]), total)

    scan = G.BlellochScan(dt)
    kt = torch.empty(total, dtype=torch.int32, device="cuda")
    ot = torch.zeros(nseg + 1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def fill(d, offsets):
        kt.copy_(torch.from_numpy(d.view(np.int32)))
        ot.copy_(torch.from_numpy(offsets.astype(np.uint32).view(np.int32)))

    def verify(d, offsets):
        assert (kt.cpu().numpy().view(np.uint32) == expected_scan(d, dt, offsets)).all()
        rb = scan.read_batch()
        assert rb["wave"] + rb["block"] + rb["long"] == int((np.diff(offsets) > 0).sum()) and rb["long"] >= 2

    def draw():
        offsets = draw_offsets()
        return make_data(rng, dt, offsets, total), offsets

    with torch.cuda.stream(side):
        d, offsets = draw()
        fill(d, offsets)
        side.synchronize()
        scan.prepare_batch(total, nseg)
        scan.run_batch_offsets_ptr(kt.data_ptr(), total, ot.data_ptr(), nseg, side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(d, offsets)
        fill(d, offsets)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        scan.run_batch_offsets_ptr(kt.data_ptr(), total, ot.data_ptr(), nseg, side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        verify(d, offsets)
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            scan.run_batch_offsets_ptr(kt.data_ptr(), total, ot.data_ptr(), nseg, torch.cuda.current_stream().cuda_stream)
        for rep in range(3):
            d, offsets = draw()
            fill(d, offsets)
            graph.replay()
            side.synchronize()
            verify(d, offsets)


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_batch_scan_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
