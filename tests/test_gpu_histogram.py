"""GPU tests of histogram (glu_histogram_run_even_ptr, glu_histogram_run_edges_ptr): uint32 counts of the samples per bin.  The oracle
is always numpy's restatement of the contract and every comparison is `==`:
  even integers  (x.astype(int64) - lo) // W, then bincount
  even floats    minimum(((x.astype(float64) - lo) * scale).astype(int64), bins - 1), NaN dropped
  edges          searchsorted(edges, x, side="right") - 1, NaN samples removed first
Every array a call writes sits inside an allocation with poison in front of it and behind it and is itself filled with poison first;
the inputs are checked unchanged; last() is checked against plan_histogram; sum(out) is the number of samples in range.  Sizes come
from plan_histogram.  The scheme is that of test_gpu_merge.py."""
import ctypes
import gc
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # bytes of poison in front of and behind an array, inside its allocation
POISON = 0xA5
POISON32 = 0xA5A5A5A5
LDS, GLOBAL = 0, 1


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def want_even(x, lo, hi, bins):
    """(counts, samples in range) by the contract's restatement."""
    if x.dtype.kind == "f":
        d = x.astype(np.float64)
        flo, fhi = np.float64(lo), np.float64(hi)
        scale = np.float64(bins) / (fhi - flo)
        d = d[(d >= flo) & (d < fhi)]
        b = np.minimum(((d - flo) * scale).astype(np.int64), bins - 1)
    else:
        w, rem = divmod(int(hi) - int(lo), bins)
        assert rem == 0 and w >= 1
        wide = x.astype(np.int64)
        wide = wide[(wide >= lo) & (wide < hi)]
        b = (wide - int(lo)) // w
    return np.bincount(b, minlength=bins).astype(np.uint32), b.size


def want_edges(x, e):
    bins = e.size - 1
    if x.dtype.kind == "f":
        x = x[~np.isnan(x)]
    b = np.searchsorted(e, x, side="right") - 1
    b = b[(b >= 0) & (b < bins)]
    return np.bincount(b, minlength=bins).astype(np.uint32), b.size


def plan_of(G, count, bins, key_type, mode, accumulate=False):
    """(path, groups, kernels) that last() must state: the plan's, with the header's rule for a call that accumulates."""
    path, _, _, groups, kernels, _ = G.plan_histogram(count, bins, key_type, mode)
    if accumulate and (path == GLOBAL or count == 0):
        kernels -= 1
    return path, groups, kernels


def check_even(G, h, x, lo, hi, bins, shift=0, out_shift=0, prior=None):
    """One even call on poisoned (prior None) or known (`prior`: accumulate) counts."""
    import torch

    key_type = str(x.dtype)
    xa = Array(bits(x), shift)
    out = Array.poisoned(4 * bins, out_shift) if prior is None else Array(prior, out_shift)
    assert xa.ptr % 16 == shift and out.ptr % 16 == out_shift
    h.run_even_ptr(xa.ptr if x.size else None, x.size, lo, hi, bins, out.ptr, key_type, prior is not None, stream())
    torch.cuda.synchronize()
    what = ("even", key_type, x.size, lo, hi, bins, shift)
    assert h.last() == plan_of(G, x.size, bins, key_type, "even", prior is not None), (what, h.last())
    want, inside = want_even(x, lo, hi, bins)
    got = out.result(np.uint32)
    assert (xa.result() == bits(x)).all(), "the call wrote to its samples"
    if prior is not None:
        want = want + prior  # (modulo 2^32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    if prior is None:
        assert int(got.sum(dtype=np.uint64)) == inside
    return got


def check_edges(G, h, x, e, shift=0, edge_shift=0, prior=None):
    import torch

    key_type, bins = str(x.dtype), e.size - 1
    assert e.dtype == x.dtype
    xa, ea = Array(bits(x), shift), Array(bits(e), edge_shift)
    out = Array.poisoned(4 * bins) if prior is None else Array(prior)
    h.run_edges_ptr(xa.ptr if x.size else None, x.size, ea.ptr, bins, out.ptr, key_type, prior is not None, stream())
    torch.cuda.synchronize()
    what = ("edges", key_type, x.size, bins, shift)
    assert h.last() == plan_of(G, x.size, bins, key_type, "edges", prior is not None), (what, h.last())
    want, inside = want_edges(x, e)
    got = out.result(np.uint32)
    assert (xa.result() == bits(x)).all() and (ea.result() == bits(e)).all(), "the call wrote to its inputs"
    if prior is not None:
        want = want + prior
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    if prior is None:
        assert int(got.sum(dtype=np.uint64)) == inside
    return got


def tile_and_groups_max(G, key_type, mode):
    """The tile, and the most workgroups the counting kernel takes (the plan of a count that needs more)."""
    tile = G.plan_histogram(1, 1, key_type, mode)[2]
    return tile, G.plan_histogram(2 ** 32 - 1, 1, key_type, mode)[3]


def samples_of(rng, n, key_type, lo, hi):
    """n samples of the type spread over [lo - 10 %, hi + 10 %) of the range"""
    dtype = np.dtype(key_type)
    span = float(hi) - float(lo)
    v = rng.random(n) * span * 1.2 + float(lo) - 0.1 * span
    if dtype.kind != "f":
        info = np.iinfo(dtype)
        v = np.clip(np.floor(v), info.min, info.max)
    return v.astype(dtype)


EVEN_RANGES = {"uint32": (1000, 1000 + 7 * 640), "int32": (-3000, -3000 + 7 * 640), "float32": (-1.5, 2.25), "float64": (-1.5, 2.25)}


@pytest.mark.parametrize("key_type", ["uint32", "int32", "float32", "float64"])
def test_even_counts_around_the_tile_and_the_stride(G, key_type):
    """Counts 0, 1, tile - 1, tile, tile + 1 and groups_max * tile + 1 (the stride over the tiles wraps), 640 bins."""
    rng = np.random.default_rng(21)
    h = G.Histogram()
    tile, most = tile_and_groups_max(G, key_type, "even")
    lo, hi = EVEN_RANGES[key_type]
    for n in (0, 1, tile - 1, tile, tile + 1, most * tile + 1):
        check_even(G, h, samples_of(rng, n, key_type, lo, hi), lo, hi, 640)
    assert G.plan_histogram(most * tile + 1, 640, key_type)[3] == most and G.plan_histogram(most * tile, 640, key_type)[3] == most
    assert G.plan_histogram(tile + 1, 640, key_type)[3] == 2


@pytest.mark.parametrize("key_type", ["uint32", "int32", "float32", "uint64", "int64", "float64"])
def test_edges_counts_around_the_tile_and_the_stride_for_every_type(G, key_type):
    rng = np.random.default_rng(22)
    h = G.Histogram()
    tile, most = tile_and_groups_max(G, key_type, "edges")
    dtype = np.dtype(key_type)
    lo, hi = (-50000, 50000) if dtype.kind != "u" else (1000, 101000)
    e = np.sort(samples_of(rng, 34, key_type, lo, hi))
    e[5] = e[4]  # (an empty bin)
    for n in (0, 1, tile - 1, tile, tile + 1, most * tile + 1):
        x = samples_of(rng, n, key_type, lo, hi)
        if n > 100:
            x[:34] = e  # (samples exactly on every edge)
        check_edges(G, h, x, e)


@pytest.mark.parametrize("key_type", ["uint32", "float64", "uint64"])
def test_samples_behind_a_sixteen_byte_boundary(G, key_type):
    """Samples 4, 8 and 12 bytes (8-byte types: 8) behind a boundary: the head and the tail of the packs are masked, and the poison
    in front of and behind the samples (0xA5A5... is a value in range of the integer cases) is not counted."""
    rng = np.random.default_rng(23)
    h = G.Histogram()
    dtype = np.dtype(key_type)
    mode = "edges" if key_type == "uint64" else "even"
    tile, _ = tile_and_groups_max(G, key_type, mode)
    for shift in (4, 8, 12):
        if shift % dtype.itemsize:
            continue
        for n in (1, 3, tile - 1, tile, 3 * tile + 1):
            if key_type == "uint32":
                x = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
                check_even(G, h, x, 0, 2 ** 32 - 1, 255, shift, out_shift=shift)  # (W = 16843009; the poison is bin 165)
            elif key_type == "float64":
                check_even(G, h, samples_of(rng, n, key_type, -1.0, 1.0), -1.0, 1.0, 100, shift, out_shift=4)
            else:
                e = np.array([0, 2 ** 40, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)  # (the poison lies in bin 2)
                check_edges(G, h, rng.integers(0, 2 ** 64, n, dtype=np.uint64), e, shift, edge_shift=8)


@pytest.mark.parametrize("bins", [1, 2, 63, 64, 65, 8191, 8192, 8193, 2 ** 20])
def test_even_bins_on_both_paths(G, bins):
    """1 .. 8192 bins in LDS (8192: the last LDS size), 8193 and 2^20 by global atomics."""
    rng = np.random.default_rng(24 + bins)
    h = G.Histogram()
    tile, _ = tile_and_groups_max(G, "uint32", "even")
    n = 5 * tile + 77
    assert G.plan_histogram(n, bins)[0] == (LDS if bins <= 8192 else GLOBAL)
    assert G.plan_histogram(n, bins)[5] == (6 * bins * 4 if bins <= 8192 else 0)
    x = rng.integers(0, 4 * bins, n, dtype=np.uint32)
    check_even(G, h, x, bins, 4 * bins, bins)  # (W = 3, a quarter of the samples below lo)
    f = rng.random(n).astype(np.float32) * np.float32(1.25)
    check_even(G, h, f, 0.0, 1.0, bins)
    # accumulate on both paths: onto known contents, and twice gives twice
    prior = rng.integers(0, 2 ** 32, bins, dtype=np.uint32)  # (the sum wraps modulo 2^32)
    once = check_even(G, h, x, bins, 4 * bins, bins, prior=prior)
    twice = check_even(G, h, x, bins, 4 * bins, bins, prior=once)
    assert (twice - prior == 2 * (once - prior)).all()


def test_the_full_int32_range_in_65535_bins_of_width_65537(G):
    rng = np.random.default_rng(25)
    h = G.Histogram()
    lo, hi, bins, w = -2 ** 31, 2 ** 31 - 1, 65535, 65537
    k = rng.integers(0, bins + 1, 30000)
    near = np.concatenate([lo + k * w + d for d in (-1, 0, 1)])
    near = near[(near >= lo) & (near <= hi)]
    x = np.concatenate([near, rng.integers(lo, hi, 70001, endpoint=True), [lo, hi, hi - 1, 0, -1]]).astype(np.int32)
    got = check_even(G, h, x, lo, hi, bins)
    assert int(got.sum()) == x.size - int((x == hi).sum())
    # and the widest word: one bin over everything but the largest key
    u = np.concatenate([rng.integers(0, 2 ** 32, 9000, dtype=np.uint32), np.array([0, 2 ** 32 - 1, 2 ** 32 - 2], dtype=np.uint32)])
    check_even(G, h, u, 0, 2 ** 32 - 1, 1)
    check_even(G, h, u, 0, 2 ** 32 - 1, 3)  # (W = 1431655765)


@pytest.mark.parametrize("bins", [1, 2, 8192])
def test_edges_bins_with_repeats_and_samples_on_every_edge(G, bins):
    rng = np.random.default_rng(26 + bins)
    h = G.Histogram()
    for key_type in ("uint32", "float32", "int64", "float64"):
        tile, _ = tile_and_groups_max(G, key_type, "edges")
        dtype = np.dtype(key_type)
        lo, hi = (-10 ** 6, 10 ** 6) if dtype.kind != "u" else (10, 2 * 10 ** 6)
        e = np.sort(samples_of(rng, bins + 1, key_type, lo, hi))
        if bins == 8192:
            e[100:104] = e[100]  # (repeated edges: empty bins)
            e[-3:] = e[-1]
        x = np.concatenate([e, samples_of(rng, 2 * tile + 5, key_type, lo, hi), e[::-1]])
        if dtype.kind == "f":
            x[bins + 1:bins + 7] = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=dtype)
        got = check_edges(G, h, x, e)
        if bins == 8192:
            assert (got[100:103] == 0).all() and got[-1] == 0 and got[-2] == 0


@pytest.mark.parametrize("mode", ["even", "edges", "global"])
def test_skewed_data(G, mode):
    """Every sample equal (one add per wave), every sample out of range, two alternating bins, a wave's worth of equal samples
    followed by distinct ones, and one equal run that ends inside a thread's packs."""
    rng = np.random.default_rng(27)
    h = G.Histogram()
    bins = 1 << 16 if mode == "global" else 500
    lo, hi = 100, 100 + 2 * bins
    tile, _ = tile_and_groups_max(G, "uint32", "edges" if mode == "edges" else "even")
    n = 3 * tile + 19
    e = (lo + 2 * np.arange(bins + 1)).astype(np.uint32)
    distinct = (lo + rng.permutation(2 * bins)[:min(n, 2 * bins)]).astype(np.uint32)
    cases = {
        "equal": np.full(n, lo + 77, dtype=np.uint32),
        "equal, last bin": np.full(n, hi - 1, dtype=np.uint32),
        "all below": np.full(n, lo - 1, dtype=np.uint32),
        "all above": np.full(n, hi, dtype=np.uint32),
        "alternating": np.where(np.arange(n) % 2 == 0, lo + 4, lo + 901).astype(np.uint32),
        "alternating packs": np.where((np.arange(n) // 4) % 2 == 0, lo + 4, lo + 901).astype(np.uint32),
        "wave then distinct": np.concatenate([np.full(64 * 16, lo + 10, dtype=np.uint32), np.resize(distinct, n - 64 * 16)]),
        "run ends in a pack": np.concatenate([np.full(tile + 6, lo + 10, dtype=np.uint32), np.full(n - tile - 6, lo + 13, dtype=np.uint32)]),
        "equal but one": np.concatenate([np.full(n - 1, lo + 10, dtype=np.uint32), np.array([lo + 400], dtype=np.uint32)]),
        "in range only at the ends": np.concatenate([[lo], np.full(n - 2, hi + 5), [hi - 1]]).astype(np.uint32),
    }
    for name, x in cases.items():
        for shift in (0, 4):
            if mode == "edges":
                check_edges(G, h, x, e, shift)
            else:
                check_even(G, h, x, lo, hi, bins, shift)


@pytest.mark.parametrize("key_type", ["float32", "float64"])
def test_floats_with_nan_infinities_and_both_zeros(G, key_type):
    rng = np.random.default_rng(28)
    h = G.Histogram()
    dtype = np.dtype(key_type).type
    tile, _ = tile_and_groups_max(G, key_type, "even")
    x = (rng.random(2 * tile + 9) * 4 - 2).astype(dtype)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, np.nextafter(dtype(1), dtype(-np.inf)), 1.0, -1.0,
                        np.nextafter(dtype(-1), dtype(-np.inf)), np.finfo(dtype).tiny, -np.finfo(dtype).tiny], dtype=dtype)
    x[rng.choice(x.size, 20 * special.size, replace=False)] = np.tile(special, 20)
    for bins in (49, 2 ** 24 if key_type == "float32" else 4096):
        got = check_even(G, h, x, -1.0, 1.0, bins)
        assert got.sum() < x.size
    e = np.array([-np.inf, -1.0, -0.0, 0.0, 0.5, np.inf], dtype=dtype)  # (bin 2 = [-0.0, 0.0) is empty: the zeros are equal)
    got = check_edges(G, h, x, e)
    assert got[2] == 0 and got[3] >= 40 and got.sum() == x.size - 60  # (NaNs and +inf dropped; -inf is bin 0's)
    # the whole array NaN: nothing counted, every count written
    assert (check_even(G, h, np.full(tile + 1, np.nan, dtype=dtype), -1.0, 1.0, 7) == 0).all()
    assert (check_edges(G, h, np.full(tile + 1, np.nan, dtype=dtype), e) == 0).all()


def test_python_bounds_of_float32_samples_are_rounded_to_float32(G):
    """lo = 0.1 for float32 samples is np.float32(0.1), as numpy stores it; an integer bound that the type does not hold is refused."""
    rng = np.random.default_rng(32)
    h = G.Histogram()
    x = rng.random(5000).astype(np.float32)
    xa, out = Array(bits(x)), Array.poisoned(4 * 10)
    h.run_even_ptr(xa.ptr, x.size, 0.1, 0.7, 10, out.ptr, "float32", False, stream())
    G.synchronize()
    assert (out.result(np.uint32) == want_even(x, np.float32(0.1), np.float32(0.7), 10)[0]).all()
    for lo, hi, key_type in ((-1, 9, "uint32"), (0, 2 ** 32, "uint32"), (0, 2 ** 31, "int32"), (0.5, 10, "uint32")):
        with pytest.raises(G.GluError) as e:
            h.run_even_ptr(xa.ptr, x.size, lo, hi, 10, out.ptr, key_type)
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT and "is not a value of" in e.value.message


def test_count_zero_in_both_modes(G):
    """No samples, NULL pointer: zeros everywhere (LDS: the sum over zero rows; GLOBAL: the clear), nothing touched under accumulate."""
    h = G.Histogram()
    e = np.arange(11, dtype=np.uint32)
    prior = np.arange(10, dtype=np.uint32) + np.uint32(7)
    empty = np.zeros(0, dtype=np.uint32)
    assert (check_even(G, h, empty, 0, 10, 10) == 0).all() and h.last() == (LDS, 0, 1)
    assert (check_even(G, h, empty, 0, 10, 10, prior=prior) == prior).all() and h.last() == (LDS, 0, 0)
    assert (check_edges(G, h, empty, e) == 0).all() and h.last() == (LDS, 0, 1)
    assert (check_edges(G, h, empty, e, prior=prior) == prior).all() and h.last() == (LDS, 0, 0)
    big = np.arange(10000, dtype=np.uint32)
    assert (check_even(G, h, empty, 0, 10000, 10000) == 0).all() and h.last() == (GLOBAL, 0, 1)
    assert (check_even(G, h, empty, 0, 10000, 10000, prior=big) == big).all() and h.last() == (GLOBAL, 0, 0)


def test_prepared_captured_replayed(G):
    """After prepare a call leaves the device's free memory as it found it; an even call, an edges call and a GLOBAL call captured
    on one side stream replay on other samples and other device edges: the launch sequence does not depend on the data."""
    import torch

    tile, _ = tile_and_groups_max(G, "uint32", "even")
    n, bins, gbins = 9 * tile + 5, 300, 20000
    rng = np.random.default_rng(29)
    h = G.Histogram()
    xt = torch.empty(n, dtype=torch.int32, device="cuda")
    et = torch.empty(bins + 1, dtype=torch.int32, device="cuda")
    out_even, out_edges = torch.empty(bins, dtype=torch.int32, device="cuda"), torch.empty(bins, dtype=torch.int32, device="cuda")
    out_global = torch.empty(gbins, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()

    def contents(spread):
        x = rng.integers(0, spread, n, dtype=np.uint32)
        e = np.sort(rng.integers(0, spread, bins + 1, dtype=np.uint32))
        return x, e

    def fill(x, e):
        xt.copy_(torch.from_numpy(x.view(np.int32)))
        et.copy_(torch.from_numpy(e.view(np.int32)))
        for o in (out_even, out_edges, out_global):
            o.fill_(-1515870811)

    def verify(x, e):
        assert (out_even.cpu().numpy().view(np.uint32) == want_even(x, 0, 3 * bins, bins)[0]).all()
        assert (out_edges.cpu().numpy().view(np.uint32) == want_edges(x, e)[0]).all()
        assert (out_global.cpu().numpy().view(np.uint32) == want_even(x, 0, gbins, gbins)[0]).all()

    def call(s):
        h.run_even_ptr(xt.data_ptr(), n, 0, 3 * bins, bins, out_even.data_ptr(), "uint32", False, s)
        h.run_edges_ptr(xt.data_ptr(), n, et.data_ptr(), bins, out_edges.data_ptr(), "uint32", False, s)
        h.run_even_ptr(xt.data_ptr(), n, 0, gbins, gbins, out_global.data_ptr(), "uint32", False, s)

    with torch.cuda.stream(side):
        data = contents(2 ** 32)
        fill(*data)
        side.synchronize()
        h.prepare(n, bins)
        call(side.cuda_stream)  # warm-up (loads the kernels)
        side.synchronize()
        verify(*data)
        fill(*data)
        side.synchronize()
        held = torch.cuda.mem_get_info()[0]
        call(side.cuda_stream)
        side.synchronize()
        assert torch.cuda.mem_get_info()[0] == held, "a prepared call changed the device memory in use"
        verify(*data)
        gc.collect()  # (a dead cycle that holds an operator object is finalised here, not inside the capture: destroying one waits for the device)
        with torch.cuda.graph(graph, stream=side):
            call(torch.cuda.current_stream().cuda_stream)
        for spread in (2 ** 32, 30000, 1000, 2):  # mostly out of range, spread over the global bins, dense, two values
            data = contents(spread)
            fill(*data)
            graph.replay()
            side.synchronize()
            verify(*data)


def test_the_same_input_gives_the_same_bits(G):
    rng = np.random.default_rng(30)
    h = G.Histogram()
    x = (rng.zipf(1.3, 200000) % 50000).astype(np.uint32)
    first = [check_even(G, h, x, 0, 50000, bins) for bins in (500, 50000)]
    for _ in range(2):
        again = [check_even(G, h, x, 0, 50000, bins) for bins in (500, 50000)]
        assert all((a == b).all() for a, b in zip(first, again))


def test_argument_errors(G):
    """Each refusal of the contract with its message; a witness buffer (out_counts lies in it) shows that nothing was written."""
    import torch

    h = G.Histogram()
    n = 4096
    x = np.arange(n, dtype=np.uint32)
    xt = torch.from_numpy(x.view(np.int32).copy()).cuda()
    et = torch.from_numpy(np.arange(0, 4 * 130, 4, dtype=np.int32)).cuda()
    wt = torch.full((4 * n,), -1515870811, dtype=torch.int32, device="cuda")  # the witness, poison
    xp, ep, wp = xt.data_ptr(), et.data_ptr(), wt.data_ptr()
    L, vp = G.lib(), ctypes.c_void_p
    lo32, hi32 = ctypes.c_uint32(0), ctypes.c_uint32(100)

    def even(samples=xp, count=64, lo=0, hi=100, bins=10, out=wp, key_type="uint32", acc=False):
        h.run_even_ptr(samples, count, lo, hi, bins, out, key_type, acc)

    def edges(samples=xp, count=64, e=ep, bins=10, out=wp, key_type="uint32"):
        h.run_edges_ptr(samples, count, e, bins, out, key_type)

    def raw_even(obj=None, key_type=0, lo=ctypes.byref(lo32), hi=ctypes.byref(hi32)):
        G.check(L.glu_histogram_run_even_ptr(obj, vp(xp), 64, key_type, lo, hi, 10, vp(wp), 0, None))

    bad = [
        (lambda: raw_even(None), "histogram is NULL"),
        (lambda: G.check(L.glu_histogram_run_edges_ptr(None, vp(xp), 64, 0, vp(ep), 10, vp(wp), 0, None)), "histogram is NULL"),
        (lambda: G.check(L.glu_histogram_prepare(None, 64, 10)), "histogram is NULL"),
        (lambda: G.check(L.glu_histogram_last(None, None, None, None)), "histogram is NULL"),
        (lambda: G.check(L.glu_histogram_create(None)), "out is NULL"),
        (lambda: even(samples=None), "Invalid samples buffer"),
        (lambda: edges(samples=None), "Invalid samples buffer"),
        (lambda: even(out=None), "Invalid out_counts buffer"),
        (lambda: edges(out=None), "Invalid out_counts buffer"),
        (lambda: edges(e=None), "Invalid edges buffer"),
        (lambda: raw_even(h._h, lo=None), "lo is NULL"),
        (lambda: raw_even(h._h, hi=None), "hi is NULL"),
        (lambda: even(samples=xp + 2), "samples is not aligned"),
        (lambda: even(samples=xp + 4, key_type="float64", lo=0.0, hi=1.0), "samples is not aligned"),
        (lambda: edges(samples=xp + 4, key_type="int64"), "samples is not aligned"),
        (lambda: even(out=wp + 2), "out_counts is not aligned"),
        (lambda: edges(e=ep + 4, key_type="uint64"), "edges is not aligned"),
        (lambda: raw_even(h._h, 6), "Invalid key type"),
        (lambda: raw_even(h._h, -1), "Invalid key type"),
        (lambda: even(key_type="uint64"), "glu_histogram_run_edges_ptr"),
        (lambda: even(key_type="int64"), "has no even bins"),
        (lambda: even(count=1 << 32), "count below 2^32"),
        (lambda: edges(count=1 << 32), "count below 2^32"),
        (lambda: h.prepare(1 << 32, 10), "count below 2^32"),
        (lambda: even(bins=0), "bins must be 1 .. 16777216"),
        (lambda: even(bins=(1 << 24) + 1, hi=(1 << 24) + 1), "bins must be 1 .. 16777216"),
        (lambda: edges(bins=0), "bins must be 1 .. 8192"),
        (lambda: edges(bins=8193), "bins must be 1 .. 8192"),
        (lambda: edges(bins=8193), "sort the samples, search the edges"),
        (lambda: h.prepare(64, 0), "bins must be"),
        (lambda: even(lo=0, hi=10, bins=3), "glu_histogram_run_edges_ptr"),  # (W = 10 / 3: the message points to the edges form)
        (lambda: even(lo=0, hi=10, bins=3), "(hi - lo) / bins must be a whole number"),
        (lambda: even(lo=0, hi=5, bins=10), "(hi - lo) / bins must be a whole number"),
        (lambda: even(lo=10, hi=10, bins=1), "(hi - lo) / bins must be a whole number"),
        (lambda: even(lo=-5, hi=-15, bins=10, key_type="int32"), "(hi - lo) / bins must be a whole number"),
        (lambda: even(lo=1.0, hi=1.0, key_type="float32"), "lo and hi must be finite with lo < hi"),
        (lambda: even(lo=2.0, hi=1.0, key_type="float64"), "lo and hi must be finite with lo < hi"),
        (lambda: even(lo=0.0, hi=float("inf"), key_type="float32"), "lo and hi must be finite"),
        (lambda: even(lo=-1.7e308, hi=1.7e308, key_type="float64"), "finite in double"),
        (lambda: even(out=xp), "out_counts overlaps samples"),
        (lambda: even(out=xp + 252), "out_counts overlaps samples"),
        (lambda: even(out=xp - 36), "out_counts overlaps samples"),
        (lambda: edges(out=ep + 40), "out_counts overlaps edges"),
        (lambda: edges(out=ep - 36), "out_counts overlaps edges"),
    ]
    for i, (call, message) in enumerate(bad):
        with pytest.raises(G.GluError) as e:
            call()
        assert e.value.status == G.GLU_ERROR_INVALID_ARGUMENT, (i, e.value.message)
        assert message in e.value.message, (i, e.value.message)
    torch.cuda.synchronize()
    assert (wt.cpu().numpy().view(np.uint32) == POISON32).all(), "a refused call wrote something"
    assert (xt.cpu().numpy().view(np.uint32) == x).all()
    # arrays that only touch are fine: the counts lie between the samples and the edges in one buffer
    one = np.concatenate([np.arange(100, dtype=np.uint32) % 7, np.full(10, POISON32, dtype=np.uint32), np.arange(11, dtype=np.uint32)])
    big = torch.from_numpy(one.view(np.int32).copy()).cuda()
    h.run_edges_ptr(big.data_ptr(), 100, big.data_ptr() + 440, 10, big.data_ptr() + 400, "uint32", False, stream())
    torch.cuda.synchronize()
    got = big.cpu().numpy().view(np.uint32)
    assert (got[:100] == one[:100]).all() and (got[110:] == one[110:]).all()
    assert (got[100:110] == np.bincount(one[:100], minlength=10)).all()


def test_unsorted_edges_and_nan_edges_stay_inside_the_arrays(G):
    """Edges that break the contract give unspecified counts: the poison around the counts is intact, the inputs are unchanged and no
    count exceeds the samples."""
    import torch

    rng = np.random.default_rng(31)
    h = G.Histogram()
    for key_type in ("float32", "uint64"):
        dtype = np.dtype(key_type)
        e = rng.permutation(8193).astype(dtype)
        if dtype.kind == "f":
            e[::5] = np.nan
        x = rng.permutation(40000).astype(dtype)
        xa, ea, out = Array(bits(x)), Array(bits(e)), Array.poisoned(4 * 8192)
        h.run_edges_ptr(xa.ptr, x.size, ea.ptr, 8192, out.ptr, key_type, False, stream())
        torch.cuda.synchronize()
        got = out.result(np.uint32)
        assert int(got.sum(dtype=np.uint64)) <= x.size
        assert (xa.result() == bits(x)).all() and (ea.result() == bits(e)).all()


def test_equi_depth_bins_from_a_sorted_sample_never_leave_the_device(G):
    """The loop the operator closes: the library's sort orders a copy of the samples, every k-th key becomes an edge by a device copy,
    and every bin of the histogram over those edges holds k samples (the last one k - 1: its right edge is the largest key)."""
    import torch

    bins, depth = 128, 517
    n = bins * depth
    x = (np.arange(n, dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32)  # (a bijection: all different)
    xt = torch.from_numpy(x.view(np.int32).copy()).cuda()
    st = xt.clone()
    vt = torch.arange(n, dtype=torch.int32, device="cuda")
    s = stream()
    G.RadixSort().sort_typed_ptr(st.data_ptr(), vt.data_ptr(), n, "uint32", s)
    et = torch.cat([st[::depth], st[-1:]]).contiguous()
    assert et.numel() == bins + 1
    out = Array.poisoned(4 * bins)
    h = G.Histogram()
    h.run_edges_ptr(xt.data_ptr(), n, et.data_ptr(), bins, out.ptr, "uint32", False, s)
    torch.cuda.synchronize()
    want = np.full(bins, depth, dtype=np.uint32)
    want[-1] -= 1
    assert (out.result(np.uint32) == want).all()


def test_cpp_program(built):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_histogram_api")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0
    assert "0 failure(s)" in p.stdout
